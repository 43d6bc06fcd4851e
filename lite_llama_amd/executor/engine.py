"""One-shot batch generation: the prefill routes, ``score`` and the hipGraph-captured decode step (see the package docstring)."""

from __future__ import annotations

import contextlib
from dataclasses import dataclass

import torch

from .. import _lib as L
from ..sampling import (MAX_TOP_LOGPROBS, Sampler, TokenLogprobs, _extras, _extras_off, _penalise, _penalty_off,
                        apply_penalties, apply_repetition_penalty, greedy_argmax, resolve_sampling, sample_with_filters,
                        seeded_uniform, token_logprobs)
from .chunking import plan_prefill_chunks
from .constraints import ConstrainedRows, constrained_argmax, constraint_advance, constraint_mask
from .kv_pool import KVPool
from .metadata import AttentionMetadata
from .paged_kv import PagedKVPool
from .speculative import SpecState, Speculation, SpeculationStats, spec_accept, spec_draft
from .stopping import RunningWatch, StopCriteria, StopState, redirect_finished, stop_advance


@dataclass
class _Span:
    """The reference's GeneratedSpan (sampler.py:64-75): padded generated tokens + validity mask."""

    token_ids: torch.Tensor
    mask: torch.Tensor


# DecodeEngine.score: the lm_head runs over this many bytes of logits at a time (the [B x L x vocab] matrix is never formed)
SCORE_LOGITS_BYTES = 256 << 20
# ... in lm_head calls of exactly this many rows each (the last one padded): whatever kernel serves that shape serves every
# row, so a row's logits do not depend on how many rows are scored or on how they are grouped into chunks
SCORE_GEMM_ROWS = 256


def _check_logprobs(logprobs) -> int | None:
    if logprobs is None:
        return None
    k = int(logprobs)
    if not 0 <= k <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be None or the number of alternatives to report, 0 .. {MAX_TOP_LOGPROBS}; got {logprobs}")
    return k


class DecodeEngine:
    """One-shot batch generation: padded-grid prefill, then lockstep greedy decode.

    ``prefill`` mirrors ModelRunner.prefill_alloc_kv_cache/_init_req_tokens_table
    (model_runner.py:153-198): the ``[batch, max_prompt_len]`` grid is flattened row-major,
    ``b_start_loc[i] = i * max_prompt_len``; ``decode`` mirrors decode_alloc_kv_cache (:200-218):
    after every forward the next B rows are bump-allocated, ``b_seq_len += 1`` and the table is
    updated, so at ``flash_decoding`` time ``b_seq_len`` already counts the token being fed.

    :class:`KVPool` and :class:`PagedKVPool` serve one interface; the engine asks which one it has only where they launch
    different things (:meth:`_advance`) and where only one of them can do what is asked (``fork``, a scattered context).
    """

    def __init__(self, model, max_batch: int, max_seq_len: int, device="cuda", kv_dtype=torch.float16,
                 kv_block_size: int | None = None, kv_scales: tuple = (1.0, 1.0), kv_share_blocks: bool = False):
        """``kv_block_size`` (extension): hand the KV pool out in blocks of that many rows from a device-side
        free stack (:class:`PagedKVPool`) instead of the reference's bump allocator; the kernels read the same per-token
        table either way, so the generated tokens are identical.  ``kv_share_blocks`` (with ``kv_block_size``): the pool
        keeps a share count per block, so requests can name the same full blocks -- ``prefill(shared_prefix_ids=...)`` and
        ``prefill(num_samples=...)`` on the paged pool."""
        if kv_share_blocks and kv_block_size is None:
            raise ValueError("kv_share_blocks needs kv_block_size: share counts are kept per block of the paged pool")
        geo = model.geo
        self.model = model
        self.device = device
        self.max_batch = max_batch
        self.max_seq_len = max_seq_len
        at0 = model.layers[0].self_attn
        self.paged = kv_block_size is not None
        self.share_blocks = bool(kv_share_blocks)
        if kv_block_size is not None:
            per_req = (max_seq_len + kv_block_size - 1) // kv_block_size
            self.pool = PagedKVPool(geo.num_layers, max_batch * per_req + 1, kv_block_size, at0.num_kv_heads, geo.head_dim,
                                    device, max_batch, max_seq_len, kv_dtype, share_blocks=self.share_blocks)
        else:
            self.pool = KVPool(geo.num_layers, max_batch * max_seq_len, at0.num_kv_heads, geo.head_dim, device, kv_dtype)
        self.info = AttentionMetadata(kv_buffer=self.pool.kv_buffer, kv_scales=tuple(float(v) for v in kv_scales))
        self.info.b_req_tokens_table = torch.zeros(max_batch, max_seq_len, dtype=torch.int32, device=device)
        self._warm_stream = None  # ONE warm-up stream per engine, made by the first captured decode
        self._positions, self._batch = None, 0  # what a prefill leaves for the decode beside ``info`` (_set_decode_ready)
        # log-probabilities (extension): of the token prefill returned / of every token of the last decode, when asked for
        self.first_logprobs: TokenLogprobs | None = None
        self.last_logprobs: TokenLogprobs | None = None
        self._prefill_logprobs = None
        # stopping (extension): per-row lengths / finish reasons / the steps run of the last decode, when it had ``stop``
        self.last_lengths = self.last_finish_reasons = self.last_steps_run = None
        # ---- the state of ONE decode: what the caller asked for, set by :meth:`decode` before :meth:`_begin_decode` ... ----
        self._sampling = None
        self._seeds = None  # per-row seeds of the draw (``sampling.seed``); None: the draw is ``torch.rand``
        self._logprobs_k = None
        self._stop: StopState | None = None
        # constrained decoding (extension): the rows' automaton states of the running prefill / decode, when it has ``constraint``
        self._constraint: ConstrainedRows | None = None
        # ... and the device tensors _begin_decode makes for it (one that a step writes belongs in :meth:`_step_tensors` too)
        self._input_ids = self._out = self._step = self._row_base = None
        self._lp: TokenLogprobs | None = None
        # speculative decoding (extension): the prompt grid and lengths the last plain prefill was given (references, no
        # copy) or why there is none; the state of the running speculative decode; the statistics of the last one
        self._prompt, self._no_prompt = None, "no prefill has run"
        self._spec: SpecState | None = None
        self.last_speculation: SpeculationStats | None = None
        if hasattr(model, "rotary_emb") and torch.device(device).type == "cuda":
            model.rotary_emb.ensure(max_seq_len + 1, device, model.embed_tokens.weight.dtype)

    # ------------------------------------------------------------------ prefill ----- #
    @torch.no_grad()
    def prefill(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None = None, sampling=None,
                chunk_size: int | None = None, shared_prefix_ids: torch.Tensor | None = None,
                num_samples: int | None = None, logprobs: int | None = None,
                constraint: ConstrainedRows | None = None) -> torch.Tensor:
        """``prompt_ids [B, Lp]`` (right-padded) -> next token per row ``[B]``: greedy, or -- with ``sampling`` -- drawn by
        the same sampler as every later token (llm_engine.py:168-176: the prefill step samples like a decode step; no
        token has been generated yet, so the repetition penalty has nothing to act on).  ``chunk_size`` (extension): run
        the grid as successive chunk steps ``[B, <= chunk_size]`` (:func:`plan_prefill_chunks`), each attending over
        what the earlier ones cached; the engine is left as the one-step prefill leaves it.  ``shared_prefix_ids`` (extension,
        int64 ``[P]``): every row's prompt is these tokens followed by its row of ``prompt_ids`` (its own tail, at least one
        token) -- the prefix is prefilled and cached once, see :meth:`_prefill_shared`.  ``num_samples`` (extension, needs
        ``kv_share_blocks``): ``n`` continuations of every prompt -- ``[B * n]`` tokens, row ``i * n + s`` = sample ``s`` of
        prompt ``i``; every prompt is prefilled and cached once, see :meth:`_prefill_samples`.  ``logprobs`` (extension, an
        integer ``k >= 0``): ``self.first_logprobs`` is left holding the log-probability of every returned token and the
        ``k`` most likely alternatives (``T = 1``), under the model's own distribution -- the log-softmax of the raw logits,
        before temperature and nucleus filter; on every route, since all of them end in :meth:`_first_tokens`.
        ``constraint`` (extension, :class:`ConstrainedRows` with one row per returned token -- ``B * n`` with
        ``num_samples``): the rows are put back to their start states, the returned token is the best (greedy) or a drawn
        (``sampling``) token among those the start state allows, and the states are advanced once; pass the same object to
        :meth:`decode` to continue.  On every route too."""
        b = prompt_ids.shape[0]
        self._constraint = None
        if constraint is not None:
            constraint.validate(self.model.geo.vocab_size, b * (int(num_samples) if num_samples is not None else 1))
        self._prefill_logprobs = _check_logprobs(logprobs)
        if num_samples is not None:
            if shared_prefix_ids is not None:
                raise ValueError("num_samples cannot be combined with shared_prefix_ids: the decode route serves one shared "
                                 "prefix per batch, not one per prompt on top of a common one")
            if not self.share_blocks:
                raise ValueError("num_samples needs kv_share_blocks (and kv_block_size): the samples of a prompt name the "
                                 "prompt's KV blocks, which takes per-block share counts")
            if int(num_samples) < 1 or b * int(num_samples) > self.max_batch:
                raise ValueError(f"num_samples {num_samples} x {b} prompts must give between 1 and max_batch "
                                 f"{self.max_batch} rows")
        self._reset_prefill_extras()
        if constraint is not None:
            constraint.reset()
            self._constraint = constraint
        if num_samples is not None:
            self._no_prompt = "prefill(num_samples=...): the rows share KV blocks of one prompt"
            return self._prefill_samples(prompt_ids, prompt_lens, sampling, chunk_size, int(num_samples))
        if shared_prefix_ids is not None:
            self._no_prompt = "prefill(shared_prefix_ids=...): the rows share the prefix's KV rows"
            return self._first_tokens(self._prefill_shared(shared_prefix_ids, prompt_ids, prompt_lens, chunk_size), sampling)
        last = self._prefill_grid(prompt_ids, prompt_lens, chunk_size)
        self._prompt = (prompt_ids, self.info.b_seq_len)  # what a speculative decode seeds its token history from
        return self._first_tokens(last, sampling)

    def _reset_prefill_extras(self) -> None:
        """What only some prefill routes set, back to "not set": called on entry by everything that fills the pool
        (:meth:`prefill`, :meth:`score`, :meth:`synthetic_context`), so no route has to undo another's."""
        info = self.info
        info.shared_prefix_len, info.shared_prefix_req = 0, 0
        info.b_ctx_len, info.max_ctx_len = None, 0
        self.first_logprobs = None
        self._prompt, self._no_prompt = None, "the pool was last filled by score() or synthetic_context(), not by a prefill"

    def _requests(self, n: int, stride: int = 1) -> torch.Tensor:
        idx = torch.arange(n, dtype=torch.int32, device=self.device)
        return idx if stride == 1 else idx * stride                # requests 0, stride, 2 stride, ...

    def _set_decode_ready(self, req_idx: torch.Tensor, lens: torch.Tensor, width: int) -> None:
        """The state a one-step prefill of a ``[B, width]`` grid with these lengths leaves -- what :meth:`_begin_decode`,
        graph capture and ``steps_per_graph`` start from, whatever route filled the pool."""
        info, b = self.info, req_idx.numel()
        info.b_req_idx = req_idx
        info.b_seq_len = lens.to(device=self.device, dtype=torch.int32).clone()
        info.b_start_loc = self._requests(b) * width
        info.max_actual_seq_len = width
        self._positions = info.b_seq_len.long().view(b, 1)
        self._batch = b

    def _prefill_grid(self, prompt_ids, prompt_lens, chunk_size: int | None, **kw) -> torch.Tensor:
        if chunk_size is not None:
            return self._prefill_chunked(prompt_ids, prompt_lens, int(chunk_size), **kw)
        return self._prefill_one_step(prompt_ids, prompt_lens, **kw)

    def _prefill_one_step(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None, req_stride: int = 1,
                          collect=None) -> torch.Tensor:
        """The whole padded grid in one step; returns the logits of every sequence's last prompt token ``[B, vocab]``.
        ``req_stride``: prompt ``i`` is request ``i * req_stride`` (room for its samples; paged pool only).  ``collect``
        (:meth:`score`): called with ``(first column, final hidden states [B, width, hidden])`` in place of the lm_head;
        nothing is returned then."""
        b, lp = prompt_ids.shape
        dev, info = self.device, self.info
        self.pool.reset()
        if prompt_lens is None:
            prompt_lens = torch.full((b,), lp, dtype=torch.int32, device=dev)
        self._set_decode_ready(self._requests(b, req_stride), prompt_lens, lp)  # the step itself reads the same metadata
        # rows for the whole grid; table cells (paged pool: blocks) for the valid tokens only -- pads write junk K/V nobody reads
        info.cur_select_index = self.pool.admit(info.b_req_idx, info.b_seq_len, lp, info.b_req_tokens_table)
        position_ids = torch.arange(lp, device=dev).unsqueeze(0).expand(b, lp)
        if collect is not None:
            collect(0, self.model.final_hidden_states(prompt_ids, position_ids, info))
            return None
        rows = torch.arange(b, device=dev) * lp + (prompt_lens.long() - 1)
        return self.model(prompt_ids, position_ids, info, logits_rows=rows)

    def _prefill_samples(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None, sampling, chunk_size: int | None,
                         n: int) -> torch.Tensor:
        """``n`` samples per prompt on the shared paged pool: prompt ``i`` is prefilled once, as request ``i * n``; requests
        ``i * n + 1 .. i * n + n - 1`` are forked from it (they name its full blocks and get a copy of the partial last
        one); the last-token logits are repeated per sample and every row draws its own first token.  The engine is left in
        the state a one-step prefill of the prompts each repeated ``n`` times leaves.  One prompt with several samples: they
        share ``(len // block_size) * block_size`` positions, which the decode steps read once (``info.shared_prefix_len``;
        several prompts are several prefixes, which the decode route does not serve: 0 then, as with ``n = 1``, where
        nothing is shared and the engine does exactly what it does without ``num_samples``)."""
        b, lp = prompt_ids.shape
        last = self._prefill_grid(prompt_ids, prompt_lens, chunk_size, req_stride=n)
        info = self.info
        lens = info.b_seq_len                                   # int32 [B], the prompts' lengths
        rows = self._requests(b * n)
        if n > 1:
            parents = info.b_req_idx.repeat_interleave(n - 1).contiguous()
            children = rows[rows % n != 0].contiguous()
            self.pool.fork(parents, children, lens.repeat_interleave(n - 1).contiguous(), info.b_req_tokens_table)
        self._set_decode_ready(rows, lens.repeat_interleave(n), lp)
        if b == 1 and n > 1:
            bs = self.pool.block_size
            info.shared_prefix_len, info.shared_prefix_req = (int(lens[0]) // bs) * bs, 0
        return self._first_tokens(last.repeat_interleave(n, dim=0), sampling)

    def _first_tokens(self, last: torch.Tensor, sampling) -> torch.Tensor:
        rows = self._constraint
        greedy = sampling is None or sampling.temperature == 0.0
        # no token has been generated yet: of the penalties and the bias only ``sampling.logit_bias`` has something to act
        # on -- the raw logits, before a constraint's mask, greedy or not; ``sampling.seed`` draws at counter 0
        scored, seeds = last, None
        if sampling is not None:
            sampling, seeds = resolve_sampling(sampling, last.shape[0], last.shape[1], self.device)
            bias = getattr(sampling, "logit_bias", None)
            if bias is not None:
                scored = apply_penalties(last, None, None, logit_bias=bias)
        if rows is not None and greedy:
            tokens = constrained_argmax(scored, rows)
        elif greedy:
            tokens = greedy_argmax(scored)
        else:
            uniform = torch.rand(last.shape[0], device=self.device) if seeds is None else seeded_uniform(seeds)
            drawn_from = scored if rows is None else constraint_mask(scored, rows)
            if scored is last:
                tokens = Sampler().sample(drawn_from, sampling, None, uniform=uniform).view(-1)
            else:  # the bias is in ``scored`` already
                tokens = sample_with_filters(drawn_from, sampling, uniform).view(-1)
            if rows is not None:
                constraint_advance(rows, tokens)
        if self._prefill_logprobs is not None:
            self.first_logprobs = token_logprobs(last, tokens, self._prefill_logprobs)
        return tokens

    def _prefill_shared(self, prefix_ids: torch.Tensor, tail_ids: torch.Tensor, tail_lens: torch.Tensor | None,
                        chunk_size: int | None) -> torch.Tensor:
        """One prompt prefix for the whole batch: the prefix is prefilled once, as one sequence, into ``P`` fresh pool rows
        named by table row 0; rows ``1 .. B-1`` of the table get the same ``P`` entries; the tails run as chunk steps with
        ``b_ctx_len = P`` (positions ``P + j``), attending over the shared rows through their own table rows.  The pool
        then holds ``P + B x tail grid`` rows instead of ``B x (P + ...)``, and the engine is in the state a one-step
        prefill of the concatenated prompts leaves, with ``info.shared_prefix_len = P``.  Returns the logits of every
        sequence's last prompt token ``[B, vocab]``.

        On the paged pool (``kv_share_blocks``) request 0 is admitted with the ``P`` prefix tokens and requests ``1 .. B-1``
        are forked from it: they name its ``P // block_size`` full blocks and get a private copy of the partial last one,
        so the rows agree over ``(P // block_size) * block_size`` positions only -- that is ``info.shared_prefix_len``
        then -- and no shared block is written by the tails or the decode steps (they write at positions >= ``P``)."""
        if self.paged and not self.share_blocks:
            raise ValueError("shared_prefix_ids needs the bump pool: sharing blocks of a paged pool (kv_block_size) would "
                             "need per-block reference counts")
        dev = self.device
        b, lt = tail_ids.shape
        prefix_ids = prefix_ids.reshape(-1).to(dev)
        p = prefix_ids.numel()
        if p < 1:
            raise ValueError("shared_prefix_ids is empty")
        if tail_lens is None:
            tail_lens = torch.full((b,), lt, dtype=torch.int32, device=dev)
        lens = [int(v) for v in tail_lens.tolist()]
        if lt < 1 or min(lens) < 1:
            raise ValueError("every row needs a tail of at least one token after the shared prefix")
        if p + max(lens) > self.max_seq_len:
            raise ValueError(f"prefix {p} + tail {max(lens)} exceeds max_seq_len {self.max_seq_len}")
        info = self.info
        table = info.b_req_tokens_table
        self.pool.reset()
        # 1. the prefix as one sequence (table row 0); its logits are not needed beyond one row for the lm_head
        self._set_decode_ready(self._requests(1), torch.full((1,), p, dtype=torch.int32, device=dev), p)
        info.cur_select_index = self.pool.admit(info.b_req_idx, info.b_seq_len, p, table)
        self.model(prefix_ids.view(1, p), torch.arange(p, device=dev).view(1, p), info,
                   logits_rows=torch.tensor([p - 1], device=dev))
        # 2. every row names the same P pool rows
        if b > 1 and self.paged:
            self.pool.fork(torch.zeros(b - 1, dtype=torch.int32, device=dev),
                           torch.arange(1, b, dtype=torch.int32, device=dev),
                           torch.full((b - 1,), p, dtype=torch.int32, device=dev), table)
        elif b > 1:
            table[1:b, :p] = table[0, :p]
        # 3. the tails, as chunk steps on top of the cached prefix
        last = self._prefill_chunked(tail_ids, tail_lens, lt if chunk_size is None else int(chunk_size), ctx0=p)
        # 4. the state a one-step prefill of the concatenated prompts leaves
        self._set_decode_ready(info.b_req_idx, tail_lens.to(dev) + p, p + lt)
        # the rows agree over whole blocks only (the bump pool's block is one row)
        info.shared_prefix_len, info.shared_prefix_req = p // self.pool.block_size * self.pool.block_size, 0
        return last

    def _prefill_chunked(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None, chunk_size: int,
                         ctx0: int = 0, req_stride: int = 1, collect=None) -> torch.Tensor:
        """Chunk steps over the prompt grid; returns the logits of every sequence's last prompt token ``[B, vocab]``.
        ``ctx0``: every sequence already holds that many cached positions (a shared prefix the table rows name); the pool is
        then left as it is and the grid's column ``j`` is position ``ctx0 + j``.  ``req_stride``: as in
        :meth:`_prefill_one_step`; so is ``collect``."""
        b, lp = prompt_ids.shape
        dev, info = self.device, self.info
        if ctx0 == 0:
            self.pool.reset()
        if prompt_lens is None:
            prompt_lens = torch.full((b,), lp, dtype=torch.int32, device=dev)
        plans = plan_prefill_chunks(prompt_lens.tolist(), lp, chunk_size)
        info.b_req_idx = self._requests(b, req_stride)
        last = None
        for ch in plans:
            w = ch.width
            info.b_seq_len = ch.b_q_len.to(dev)
            info.b_ctx_len = ch.b_ctx_len.to(dev) + ctx0
            info.b_start_loc = ch.b_start_loc.to(dev)
            info.max_actual_seq_len = w
            info.max_ctx_len = ch.max_ctx_len + ctx0
            # B * width rows; table[req, ctx_i + j] names them (paged pool: blocks up to ctx + n) for valid tokens only
            info.cur_select_index = self.pool.extend_at(info.b_req_idx, info.b_ctx_len, info.b_seq_len, w,
                                                        info.b_req_tokens_table)
            ids = prompt_ids[:, ch.col0:ch.col0 + w].contiguous()
            if collect is not None:
                collect(ch.col0, self.model.final_hidden_states(ids, ch.positions.to(dev) + ctx0, info))
                continue
            # a chunk that ends no sequence still computes one logits row (the lm_head takes no empty batch)
            rows = ch.logits_rows if ch.ends.numel() else torch.zeros(1, dtype=torch.int64)
            logits = self.model(ids, ch.positions.to(dev) + ctx0, info, logits_rows=rows.to(dev))
            logits = logits.view(-1, logits.shape[-1])
            if last is None:
                last = torch.empty(b, logits.shape[-1], dtype=logits.dtype, device=dev)
            if ch.ends.numel():
                last[ch.ends.to(dev)] = logits
        # the state a one-step prefill leaves: decode, graph capture and steps_per_graph run unchanged
        info.b_ctx_len, info.max_ctx_len = None, 0
        self._set_decode_ready(info.b_req_idx, prompt_lens, lp)
        return last

    # ------------------------------------------------------------------ score ------- #
    @torch.no_grad()
    def score(self, token_ids: torch.Tensor, lens: torch.Tensor | None = None, chunk_size: int | None = None,
              top_k: int = 0, logits_rows: int | None = None) -> TokenLogprobs:
        """Log-likelihood of given text (extension): ``token_ids [B, L]`` (right-padded to ``lens``) -> :class:`TokenLogprobs`
        with ``T = L - 1``, entry ``[i, j] = log P(token_ids[i, j + 1] | token_ids[i, :j + 1])`` for ``j + 1 < lens[i]`` and
        ``0.0`` (``top_ids = -1``) on padding: ``cumulative()`` is the sequence log-likelihood, ``-cumulative() / (lens - 1)``
        the per-token negative log-likelihood.  Runs the prefill path (either pool, optionally in chunk steps), then the
        lm_head and the log-probability kernel over the final hidden states ``logits_rows`` rows at a time (rounded down to
        whole lm_head calls of ``SCORE_GEMM_ROWS`` rows; default: ``SCORE_LOGITS_BYTES`` of logits), so the logits stay a
        bounded temporary.  The pool is used as a prefill uses it: call :meth:`prefill` again before :meth:`decode`."""
        k = _check_logprobs(top_k)
        dev = self.device
        b, l = token_ids.shape
        token_ids = token_ids.to(dev)
        lens_t = torch.full((b,), l, dtype=torch.int32, device=dev) if lens is None else lens.to(device=dev, dtype=torch.int32)
        if b > self.max_batch or l > self.max_seq_len:
            raise ValueError(f"token_ids {b} x {l} exceeds max_batch {self.max_batch} x max_seq_len {self.max_seq_len}")
        self._reset_prefill_extras()
        out = TokenLogprobs.blank(b, max(l - 1, 0), k, dev)
        if l < 2:
            return out
        hidden = torch.empty(b, l, self.model.geo.hidden_size, dtype=self.model.norm_weight.dtype, device=dev)

        def collect(col0, h):
            hidden[:, col0:col0 + h.shape[1]] = h.view(b, -1, hidden.shape[-1])

        self._prefill_grid(token_ids, lens_t, chunk_size, collect=collect)
        # position (i, j) predicts token (i, j + 1): the rows with j + 1 < lens[i]
        valid = torch.arange(1, l, device=dev).unsqueeze(0) < lens_t.view(b, 1)
        src = valid.nonzero()                                   # [n, 2], row-major
        n = src.shape[0]
        flat = src[:, 0] * l + src[:, 1]
        targets = token_ids.reshape(-1)[flat + 1].to(torch.int64).contiguous()
        vocab = self.model.lm_head_weight.shape[0]
        g = SCORE_GEMM_ROWS
        step = int(logits_rows) if logits_rows is not None else SCORE_LOGITS_BYTES // (2 * vocab)
        step = max(g, min(step, 4096) // g * g)
        got = TokenLogprobs.blank(n, 1, k, dev)
        hidden = hidden.view(b * l, -1)
        rows_in = torch.zeros(min(step, (n + g - 1) // g * g), hidden.shape[-1], dtype=hidden.dtype, device=dev)
        logits = torch.empty(rows_in.shape[0], vocab, dtype=hidden.dtype, device=dev)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            rows_in[:r1 - r0] = hidden[flat[r0:r1]]
            for g0 in range(0, r1 - r0, g):
                logits[g0:g0 + g] = self.model.logits_from_hidden(rows_in[g0:g0 + g])
            token_logprobs(logits[:r1 - r0], targets[r0:r1], k,
                           out=TokenLogprobs(got.chosen[r0:r1], got.top_logprobs[r0:r1], got.top_ids[r0:r1]))
        out.chosen[src[:, 0], src[:, 1]] = got.chosen[:, 0]
        if k:
            out.top_logprobs[src[:, 0], src[:, 1]] = got.top_logprobs[:, 0]
            out.top_ids[src[:, 0], src[:, 1]] = got.top_ids[:, 0]
        return out

    @torch.no_grad()
    def synthetic_context(self, batch: int, ctx_len: int, seed: int = 0, scattered: bool = False) -> torch.Tensor:
        """Benchmark helper: instead of running a prefill, fill the first ``ctx_len`` cache rows of
        every sequence with seeded random K/V (synthetic data of the prefill's shape) and return
        random first tokens.  Metadata ends up exactly as after ``prefill``.  ``scattered``: the
        table names the context rows in a random permutation (the fragmented-pool case: every K/V
        row of a sequence sits somewhere else) instead of one contiguous run per sequence (bump pool only)."""
        dev, info = self.device, self.info
        self.pool.reset()
        self._reset_prefill_extras()
        g = torch.Generator(device=dev).manual_seed(seed)
        self._set_decode_ready(self._requests(batch), torch.full((batch,), ctx_len, dtype=torch.int32, device=dev), ctx_len)
        rows = self.pool.admit(info.b_req_idx, info.b_seq_len, ctx_len, info.b_req_tokens_table).long()  # fills the table
        if scattered and not self.paged:
            info.b_req_tokens_table[:batch, :ctx_len] = rows[torch.randperm(batch * ctx_len, generator=g, device=dev)].view(
                batch, ctx_len)
        for kv in self.pool.kv_buffer:
            kv[rows] = (torch.randn(batch * ctx_len, kv.shape[1], kv.shape[2], generator=g, device=dev) * 0.5).to(kv.dtype)
        return torch.randint(0, self.model.geo.vocab_size, (batch,), generator=g, device=dev)

    # ------------------------------------------------------------------ decode ------ #
    def _begin_decode(self, first_tokens: torch.Tensor, max_new_tokens: int):
        """The first step's row and this decode's device state, for what :meth:`decode` was asked (``_stop``, ``_logprobs_k``)."""
        b, dev, info = self._batch, self.device, self.info
        # decode_alloc_kv_cache for the first decode step: the row of position seq_len - 1.  The paged pool repeats this
        # launch inside every later step (graph included); the bump pool's later steps take the rows reserved here
        info.b_seq_len = info.b_seq_len + 1
        info.max_actual_seq_len += 1
        info.cur_select_index = self.pool.append(info.b_req_idx, info.b_seq_len, info.b_req_tokens_table)
        self.pool.reserve(b * (max_new_tokens - 1))
        self._input_ids = first_tokens.view(b, 1).clone()
        # column 0 holds the token sampled by the prefill step: it is part of the generated span the repetition
        # penalty looks at from the second token on (llm_engine.py:168-176: GeneratedSpan over tokens[:, :cur_pos])
        # with ``stop`` the columns of steps never run (early exit) read as the pad, like those of finished rows
        pad = 0 if self._stop is None else self._stop.pad
        self._out = torch.full((b, max_new_tokens + 1), pad, dtype=torch.long, device=dev)
        self._out[:, 0] = first_tokens.view(b)
        self._step = torch.ones(1, dtype=torch.long, device=dev)
        self._row_base = torch.arange(b, device=dev) * (max_new_tokens + 1)
        # log-probability buffers laid out like _out (column 0 = the prefill's token, not filled here), so the kernel
        # writes at column _step as it stands
        self._lp = None if self._logprobs_k is None else TokenLogprobs.blank(b, max_new_tokens + 1, self._logprobs_k, dev)

    def _step_tensors(self) -> list:
        """Every tensor a decode step writes, the pool's own aside: what the warm-up step and the captures must not leave
        a trace in.  The log-probability buffers (_lp) have no place here: the warm-up step and the capture write the very
        column (_step, which IS restored) that the first replay writes again, with the same values."""
        info = self.info
        if self._spec is not None:  # a speculative decode: the verify step's state (SpecState lists it)
            return list(self._spec.tensors()) + [info.b_req_tokens_table]
        tensors = [self._input_ids, self._positions, info.cur_select_index, info.b_seq_len, self._step, self._out,
                   info.b_req_tokens_table]
        for part in (self._stop, self._constraint):
            if part is not None:
                tensors += part.tensors()
        return tensors

    def _snapshot(self):
        return [t.clone() for t in self._step_tensors()], self.pool.snapshot()

    def _restore(self, snap) -> None:
        for t, saved in zip(self._step_tensors(), snap[0]):
            t.copy_(saved)
        self.pool.restore(snap[1])

    def _step_body(self):
        """forward -> greedy sample -> record -> advance metadata (all on device); the verify step of a speculative decode."""
        if self._spec is not None:
            return self._spec_step()
        logits = self.model(self._input_ids, self._positions, self.info)[:, -1, :]
        nxt = self._sample(logits)
        if self._lp is not None:
            # the model's own distribution: the raw logits (_sample penalises a copy); before _advance moves _step on
            token_logprobs(logits, nxt, self._logprobs_k, out=self._lp, column=self._step)
        self._advance(nxt)

    def _sample(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy argmax, or -- with ``sampling`` set by :meth:`decode` -- the reference sampler's sequence
        (repetition penalty over the tokens generated so far, then temperature + nucleus sampling) on
        the HIP kernels; the uniform numbers come from ``torch.rand`` (graph-safe Philox) or, with ``sampling.seed``, from
        the rows' own seeds at the counter ``_step``.  With ``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` on,
        ``apply_penalties`` takes the repetition penalty's place (same span, same single pass over the logits)."""
        sp = self._sampling
        rows = self._constraint
        # rows that were finished when the step began keep their automaton state
        finished = None if self._stop is None else self._stop.finished
        if sp is None:
            return greedy_argmax(logits) if rows is None else constrained_argmax(logits, rows, finished)
        b = self._batch
        generated = None
        extras = _extras(sp)
        extras_on = not _extras_off(*extras)
        if sp.repetition_penalty != 1.0 or not (_penalty_off(extras[0]) and _penalty_off(extras[1])):
            span = self._out.shape[1]
            mask = torch.arange(span, device=self.device).unsqueeze(0) < self._step  # [1, span] -> rows share it
            generated = _Span(self._out, mask.expand(b, span))
        uniform = None
        if sp.temperature != 0.0:
            uniform = torch.rand(b, device=self.device) if self._seeds is None else seeded_uniform(self._seeds, self._step)
        if rows is None:
            return Sampler().sample(logits, sp, generated, uniform=uniform).view(-1)
        # constrained: the penalty acts on the raw logits as it does above; greedy rows pick among the allowed tokens of
        # the (penalised) logits in one launch, sampled ones draw from a copy with the disallowed tokens at -inf
        if extras_on:
            logits = _penalise(logits, sp, generated, *extras)
        elif generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, sp.repetition_penalty)
        if sp.temperature == 0.0:
            return constrained_argmax(logits, rows, finished)
        # top_k / min_p of sp act on the masked copy: top-k counts among the allowed tokens
        nxt = sample_with_filters(constraint_mask(logits, rows), sp, uniform).view(-1)  # (not Sampler: no second bias)
        constraint_advance(rows, nxt, finished)
        return nxt

    def _advance(self, nxt: torch.Tensor) -> None:
        """record -> feed back -> positions/lengths/KV rows += -> token table: one launch when the state
        has the engine's own dtypes, else the reference-shaped sequence of tensor ops."""
        info, b = self.info, self._batch
        t = info.b_req_tokens_table
        if self._stop is not None:
            # the same bookkeeping for the rows still running, plus the stop decision: one launch in ll_decode_advance's
            # place (bump pool) / in place of the tensor ops below (paged pool; a finished row's unchanged length pops
            # nothing in the append, and its K/V row is pointed at the junk block)
            if self.paged:
                stop_advance(self._out, self._step, nxt, self._input_ids, self._positions, None, info.b_seq_len, None,
                             None, self._stop)
                self.pool.append(info.b_req_idx, info.b_seq_len, t, out=info.cur_select_index)
                redirect_finished(info.cur_select_index, self._stop, (self.pool.num_blocks - 1) * self.pool.block_size,
                                  self.pool.block_size)
            else:
                stop_advance(self._out, self._step, nxt, self._input_ids, self._positions, info.cur_select_index,
                             info.b_seq_len, info.b_req_idx, t, self._stop)
            return
        if (not self.paged and nxt.dtype == torch.int64 and info.cur_select_index.dtype == torch.int32
                and info.b_seq_len.dtype == torch.int32 and info.b_req_idx.dtype == torch.int32 and t.dtype == torch.int32
                and nxt.is_contiguous() and info.cur_select_index.is_contiguous() and info.b_seq_len.is_contiguous()
                and info.b_req_idx.is_contiguous()):
            L.check(
                L.lib().ll_decode_advance(
                    self._out.data_ptr(), self._out.stride(0), self._step.data_ptr(), nxt.data_ptr(),
                    self._input_ids.data_ptr(), self._positions.data_ptr(), info.cur_select_index.data_ptr(),
                    info.b_seq_len.data_ptr(), info.b_req_idx.data_ptr(), t.data_ptr(), t.stride(0), t.stride(1),
                    b, L.stream_ptr()),
                "decode_advance")
            return
        # the paged pool, and the bump pool on state of other dtypes: the tensor ops, then the pool's own row for the step
        self._out.view(-1).scatter_(0, self._row_base + self._step, nxt)
        self._step += 1
        self._input_ids.copy_(nxt.view(b, 1))
        self._positions += 1
        info.b_seq_len += 1
        self.pool.append(info.b_req_idx, info.b_seq_len, t, out=info.cur_select_index)

    @torch.no_grad()
    def decode(self, first_tokens: torch.Tensor, max_new_tokens: int, use_graph: bool = True,
               warmup_steps: int = 0, on_step=None, sampling=None, steps_per_graph: int = 1,
               logprobs: int | None = None, stop: StopCriteria | None = None,
               constraint: ConstrainedRows | None = None, speculate: Speculation | None = None) -> torch.Tensor:
        """Generate ``max_new_tokens`` greedy tokens per row; returns ``[B, max_new_tokens]``.

        With ``use_graph`` the step is captured once (``max_actual_seq_len`` baked as the final
        context length rounded up to the attention partition size) and replayed per token.
        ``warmup_steps`` of the total are run before ``on_step`` timing hooks fire (bench use).
        ``steps_per_graph`` ("a whole multi-step decode is one graph launch", the counterpart of the loop in
        engine/llm_engine.py:137-213): that many consecutive steps are captured in ONE hipGraph -- every step already
        advances its own metadata on the device, so the steps chain without the host -- and a remainder shorter than the
        group replays a one-step graph; ``on_step(i)`` then fires once per replay with the index of its first step.
        ``logprobs`` (extension; ``None``: the step holds exactly the launches it holds without it): an integer ``k >= 0``
        makes every step record, inside the step (captured with it), the log-probability of the token it emitted and the
        ``k`` most likely alternatives under the model's own distribution (log-softmax of the raw logits: before repetition
        penalty, temperature and nucleus filter); ``self.last_logprobs`` then holds them, column ``t`` describing returned
        token ``[:, t]``.  The returned tokens are the same either way.
        ``stop`` (extension, :class:`StopCriteria`; ``None``: the step holds exactly the launches it holds without it):
        rows end at a stop id, a stop sequence or their ``max_tokens`` -- decided on the device inside the step (captured
        with it, executor/stopping.py).  ``self.last_lengths`` / ``self.last_finish_reasons`` (int32 ``[B]``) then say where
        and why each row ended, the returned tokens hold ``pad_token_id`` at and beyond a row's length (``last_logprobs``
        its initial values there), and the loop ends early once every row has: every ``check_every`` steps the host
        enqueues a copy of the running-row count to pinned memory and waits only for the copy enqueued one interval
        earlier; ``self.last_steps_run`` is the number of steps issued.  Rows still running are not affected by the others'
        stopping: their tokens are those of a decode without ``stop``.
        ``constraint`` (extension, :class:`ConstrainedRows`; ``None``: the step holds exactly the launches it holds without
        it): every row emits only tokens its automaton state allows and the state follows them, inside the step (captured
        with it, executor/constraints.py) -- greedy steps select and advance in one launch in the argmax's place, sampled
        steps mask a copy of the logits, draw, and advance.  The rows continue from ``constraint.states`` (where a
        ``prefill(constraint=...)`` left them); afterwards ``constraint.states`` describes the valid tokens of every row
        (rows finished by ``stop`` no longer move).  ``logprobs`` keeps reporting the model's own distribution.
        ``sampling`` may carry ``top_k`` (int) and ``min_p`` (float in [0, 1]) -- extension; absent, 0 and 0.0 are off and
        the step holds exactly the launches it holds without them: the draw then runs ``ll_sample_filtered`` in
        ``ll_sample_top_p``'s place (sampling.sample_filtered has the rule), here and in :meth:`prefill`; under a
        ``constraint`` the filters see the masked copy, so top-k counts among the allowed tokens.
        ``sampling`` may also carry ``presence_penalty`` / ``frequency_penalty`` (floats), ``logit_bias`` (a ``{token: bias}``
        dict for every row or a list with one dict / ``None`` per row; ``-inf`` bans a token) and ``seed`` (``None``, an int
        ``s`` -- row ``i`` draws from seed ``s + i`` -- or one int per row) -- extension; absent or neutral, the step holds
        exactly the launches it holds without them.  The penalties count the tokens of the span the repetition penalty
        looks at and run with it in ``ll_logit_penalties`` (sampling.apply_penalties has the rule), on the raw logits
        before a ``constraint``'s mask; :meth:`prefill` applies the bias to its token too.  With a seed the step that
        writes column ``c`` of the output (the prefill's token is column 0) draws row ``i``'s number from the row's seed
        and ``c`` alone (sampling.seeded_uniform): eager, captured and ``steps_per_graph`` runs draw the same numbers, and
        a row's stream does not depend on the rows beside it.
        ``speculate`` (extension, :class:`Speculation`; ``None``: every step holds exactly the launches it holds without
        it): greedy speculative decoding on the paged pool, :meth:`_decode_speculative` -- every step verifies up to ``k``
        drafted tokens per row in one forward over a ``[B, k + 1]`` grid and a row advances by every draft the model agrees
        with plus one; ``self.last_speculation`` then holds the acceptance statistics.
        """
        if speculate is not None:
            return self._decode_speculative(first_tokens, max_new_tokens, speculate, use_graph, on_step, sampling,
                                            steps_per_graph, logprobs, stop, constraint)
        self._set_decode_options(first_tokens, sampling, logprobs, stop, constraint)
        self._prompt, self._no_prompt = None, "a decode has already continued the last prefill"
        self._begin_decode(first_tokens, max_new_tokens)
        watch = RunningWatch(self._stop) if stop is not None and stop.check_every > 0 else None
        info = self.info
        final_len = info.max_actual_seq_len + max_new_tokens
        if final_len > self.max_seq_len:
            raise RuntimeError(f"context {final_len} exceeds max_seq_len {self.max_seq_len}")
        graphs, group = {}, 1
        if use_graph:
            info.max_actual_seq_len = (final_len + 127) // 128 * 128  # bucket, fixes the attention grid
            snap = self._warm_up()
            group = max(1, min(int(steps_per_graph), max_new_tokens))
            graphs = {steps: self._capture(steps, snap) for steps in sorted({1, group})}
        steps_run = self._run_steps(max_new_tokens, graphs, group, on_step, watch)
        self._check_device_errors()
        return self._results(max_new_tokens, steps_run)

    def _set_decode_options(self, first_tokens, sampling, logprobs, stop, constraint) -> None:
        """Validate what :meth:`decode` was asked for and make it the running decode's; the last decode's results go."""
        self._constraint = None
        if constraint is not None:
            constraint.validate(self.model.geo.vocab_size, self._batch)
        self._logprobs_k = _check_logprobs(logprobs)
        self.last_logprobs = self.last_lengths = self.last_finish_reasons = self.last_steps_run = None
        self.last_speculation = self._spec = None
        self._stop = None
        if stop is not None:
            stop.validate(self.model.geo.vocab_size, self._batch)
            self._stop = StopState(stop, first_tokens, self.device)
        self._constraint = constraint
        # None = greedy; else an object with temperature / top_p / repetition_penalty [/ top_k / min_p / presence_penalty /
        # frequency_penalty / logit_bias / seed]: the bias is built into its device form and the seeds are laid out here, once
        self._sampling, self._seeds = resolve_sampling(sampling, self._batch, self.model.geo.vocab_size, self.device)

    def _warm_up(self):
        """One eager step on a side stream (workspace growth, library init), fenced both ways (cuda_graph.py:110-115);
        returns the snapshot of the state before it, which is put back."""
        snap = self._snapshot()
        if self._warm_stream is None:
            self._warm_stream = torch.cuda.Stream()  # ONE warm-up stream per engine: eager scratch is kept per stream
        s = self._warm_stream
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step_body()
        torch.cuda.current_stream().wait_stream(s)
        self._restore(snap)
        # The sticky device-side error words are read here once too, right after the eager warm-up step created the
        # scratch they live in: a stale error of an earlier run surfaces before the run starts, and the check's first-use
        # costs in a process (first device-to-host copy: several ms) are paid outside anybody's timed region -- at the end
        # of a 32-step run they read as +0.2 ms per step (round 4).
        self._check_device_errors()
        return snap

    def _capture(self, steps: int, snap):
        """``steps`` consecutive steps in one hipGraph; the state is put back to ``snap`` afterwards."""
        graph = torch.cuda.CUDAGraph()
        try:
            with L.graph_capture(graph):
                for _ in range(steps):
                    self._step_body()
        except Exception:
            # a refused capture (e.g. a collective the backend cannot record) must not leave the stream in capture
            # mode: the caller falls back to eager launches on this very stream
            with contextlib.suppress(Exception):
                if torch.cuda.is_current_stream_capturing():
                    graph.capture_end()
            raise
        finally:
            self._restore(snap)  # capture does not execute, but keep the state explicit
        return graph

    def _run_steps(self, total: int, graphs: dict, group: int, on_step, watch) -> int:
        """Issue ``total`` steps -- replays of the ``group``-step graph while that many remain, then of the one-step graph;
        eager steps without graphs -- and return how many were issued: fewer once ``watch`` has seen every row finish."""
        info, i = self.info, 0
        while i < total:
            if on_step is not None:
                on_step(i)
            if graphs:
                n = group if total - i >= group else 1
                graphs[n].replay()
            else:
                n = 1
                info.max_actual_seq_len = int(info.max_actual_seq_len)  # eager: exact value
                self._step_body()
                info.max_actual_seq_len += 1
            i += n
            if watch is not None and watch.all_finished(i):
                break
        return i

    def _results(self, max_new_tokens: int, steps_run: int) -> torch.Tensor:
        if self._stop is not None:
            st = self._stop
            self.last_lengths, self.last_finish_reasons, self.last_steps_run = st.lengths, st.reasons, steps_run
            if self._lp is not None:
                # finished rows kept computing: their columns at and beyond the length go back to the initial values
                gone = torch.arange(max_new_tokens + 1, device=self.device).unsqueeze(0) > st.lengths.view(-1, 1)
                self._lp.chosen.masked_fill_(gone, 0.0)
                self._lp.top_logprobs.masked_fill_(gone.unsqueeze(-1), 0.0)
                self._lp.top_ids.masked_fill_(gone.unsqueeze(-1), -1)
        if self._lp is not None:
            self.last_logprobs = TokenLogprobs(self._lp.chosen[:, 1:], self._lp.top_logprobs[:, 1:], self._lp.top_ids[:, 1:])
        return self._out[:, 1:]

    # ------------------------------------------------------ speculative decode ------ #
    def _decode_speculative(self, first_tokens, max_new_tokens: int, spec: Speculation, use_graph: bool, on_step, sampling,
                            steps_per_graph: int, logprobs, stop: StopCriteria | None, constraint) -> torch.Tensor:
        """``decode(speculate=...)``: at most ``max_new_tokens`` verify steps, each ONE forward over a ``[B, k + 1]`` grid
        (executor/speculative.py has the rules).  The step is the draft launch, the pool's ``extend_at``, the model's chunk
        step (the attention of a chunked prefill, the decode GEMMs while ``B (k + 1) <= 64``), the argmax over all
        ``B (k + 1)`` logits rows and the accept launch; nothing in it reads a length from the host, so with ``use_graph``
        it is captured once and replayed.  The loop ends early once no row is running (rows also finish at
        ``max_new_tokens``): every ``check_every`` steps, one interval late, as with ``stop``.  ``self.last_speculation``
        holds the statistics, ``self.last_steps_run`` the steps issued; with ``stop`` (stop ids, ``max_tokens``, the pad)
        ``last_lengths`` / ``last_finish_reasons`` are filled and the columns at and beyond a row's length read as the pad.
        Call :meth:`prefill` again before the next decode."""
        self.last_logprobs = self.last_lengths = self.last_finish_reasons = self.last_steps_run = None
        self.last_speculation = None
        self._stop = self._constraint = self._sampling = self._logprobs_k = None
        if not isinstance(spec, Speculation):
            raise ValueError("speculate must be a Speculation")
        if not self.paged:
            raise ValueError("speculative decoding needs the paged pool (kv_block_size): on the bump pool every verify step "
                             "would burn B * (k + 1) fresh rows")
        if self.pool.kv_buffer[0].element_size() == 1:
            raise ValueError("speculative decoding is not served on an e4m3 KV pool")
        for name, given in (("sampling", sampling), ("logprobs", logprobs), ("constraint", constraint)):
            if given is not None:
                raise ValueError(f"speculative decoding is greedy acceptance only: {name} cannot be combined with speculate")
        if int(steps_per_graph) > 1:
            raise ValueError("speculative decoding captures one verify step per graph: steps_per_graph must be 1")
        if self._prompt is None:
            raise ValueError(f"speculative decoding needs the prompt of a plain prefill on this engine: {self._no_prompt}")
        b, info, k = self._batch, self.info, spec.num_draft_tokens
        vocab = self.model.geo.vocab_size
        if stop is not None:
            if stop.stop_sequences:
                raise ValueError("speculative decoding does not serve stop_sequences: a sequence may complete inside an "
                                 "accepted run")
            stop.validate(vocab, b)
        spec.validate(vocab, b)
        if first_tokens.numel() != b:
            raise ValueError(f"first_tokens holds {first_tokens.numel()} tokens for a batch of {b}")
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        width = int(info.max_actual_seq_len)                    # the prompt grid's width bounds every prompt length
        if width + k + 1 > self.max_seq_len:
            raise ValueError(f"a verify step of {k + 1} positions does not fit behind a prompt of {width} in max_seq_len "
                             f"{self.max_seq_len}")
        if width + max_new_tokens > self.max_seq_len:
            raise RuntimeError(f"context {width + max_new_tokens} exceeds max_seq_len {self.max_seq_len}")
        prompt_ids, prompt_lens = self._prompt
        self._prompt, self._no_prompt = None, "a speculative decode has already continued the last prefill"
        st = self._spec = SpecState(spec, stop, prompt_ids, prompt_lens, first_tokens, max_new_tokens, self.max_seq_len,
                                    self.device)
        # the chunk step's metadata: every length is a device tensor the draft launch rewrites, the grid is static
        info.b_seq_len, info.b_ctx_len, info.b_start_loc = st.q_len, st.ctx_len, st.b_start_loc
        info.cur_select_index = st.cur_select_index
        info.max_actual_seq_len, info.max_ctx_len = k + 1, self.max_seq_len
        try:
            graph = None
            if use_graph:
                graph = self._capture(1, self._warm_up())      # _step_body / _step_tensors serve the verify step
            watch = RunningWatch(st) if spec.check_every > 0 else None
            steps_run = 0
            while steps_run < max_new_tokens:
                if on_step is not None:
                    on_step(steps_run)
                if graph is not None:
                    graph.replay()
                else:
                    self._spec_step()
                steps_run += 1
                if watch is not None and watch.all_finished(steps_run):
                    break
        finally:
            info.b_ctx_len, info.max_ctx_len = None, 0
            self._spec = None
        self._check_device_errors()
        self.last_steps_run = steps_run
        self.last_speculation = SpeculationStats(st.verify_steps, st.drafted, st.accepted,
                                                 st.accepted_per_step[:, :steps_run], steps_run)
        if stop is not None:
            self.last_lengths, self.last_finish_reasons = st.lengths, st.reasons
        return st.out[:, 1:]

    def _spec_step(self) -> None:
        """draft -> KV cells -> forward -> argmax -> accept (all on device)."""
        st, info = self._spec, self.info
        spec_draft(st)
        # No rollback of rejected positions: a row's ctx only counts tokens it emitted, so the cells of a rejected draft lie
        # at positions >= the new ctx.  The blocks behind them stay with the row (the pool never shrinks a request), this
        # extend derives the same table cells from them again, and the step's K/V scatter overwrites them before the
        # attention reads -- which, causal over ctx + j, never looks past the cells this very step wrote.
        self.pool.extend_at(info.b_req_idx, st.ctx_len, st.q_len, st.k + 1, info.b_req_tokens_table, out=st.cur_select_index)
        logits = self.model(st.ids, st.positions, info)
        spec_accept(st, greedy_argmax(logits).view(-1))

    def _check_device_errors(self) -> None:
        """Sticky device-side error words, read where the host synchronises anyway (end of a decode): a lost peer of the
        one-shot all-reduce, an exhausted / misused block pool.  Nothing to read (and no synchronisation) otherwise."""
        from ..distributed import parallel_state as ps

        if ps._ONESHOT is not None:
            ps.check_collective_errors()
        if L.gemm_scratch_error(torch.device(self.device)):
            raise RuntimeError("a split-K GEMM merge gave up waiting for a contributor workgroup: its output tile was poisoned "
                               "with NaN and the merge counters are not zero at rest")
        err = self.pool.error  # the bump pool: always 0, and no synchronisation
        if err:
            raise RuntimeError(f"paged KV pool reported error bits {err:#x} (1: a call found too few free blocks, "
                               "2: a request outgrew its block-table / token-table row, 4: a fork "
                               "broke its contract)")
        if self._constraint is not None:
            err = int(self._constraint.error.item())
            if err:
                raise RuntimeError(f"constrained decoding reported error bits {err:#x} (1: a row was to follow a token its "
                                   "automaton state does not allow, 2: a row's state lies outside the automaton)")
