"""Decode-step driver: per-step metadata, the token-attention KV pool and the hipGraph-captured
decode step.  Counterpart of lite_llama/executor/{attention_metadata.py:19-44,
kv_cache_manager.py:197-299, model_runner.py:153-218,310-330, cuda_graph.py:54-249} and of the
one-shot decode loop engine/llm_engine.py:137-213 (greedy, no EOS stop, lockstep batch).

MI355X-first differences from the reference (extensions, not parity changes):
  * the WHOLE step -- forward, greedy argmax, KV-row bump, ``b_seq_len += 1``,
    ``update_kv_index`` and feeding the sampled token back -- is captured in one hipGraph, so a
    decode step is a single ``hipGraphLaunch`` with no host work in between (the reference
    replays only the forward and does 5 host-issued copies + sampler + index update per step);
  * the graph is also captured under tensor parallelism (RCCL all-reduces are capturable);
    the reference disables graphs for TP>1 (model_runner.py:260-266);
  * the reference's loop has no EOS stop; ``decode(stop=StopCriteria(...))`` ends rows at stop ids, stop sequences and
    per-row ``max_tokens`` -- the decision is taken on the device inside the captured step (csrc/decode_stop.hip in
    ``ll_decode_advance``'s place, executor/stopping.py), finished rows are frozen, the results say where and why each
    row ended (``last_lengths`` / ``last_finish_reasons``) and the loop ends early once every row has, without a host
    synchronisation per step.  Without ``stop`` the loop is the reference's: lockstep, ``max_new_tokens`` steps.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import os

import torch

from .. import _lib as L
from ..kernels import update_kv_index
from ..sampling import (MAX_TOP_LOGPROBS, Sampler, TokenLogprobs, apply_repetition_penalty, greedy_argmax,
                        sample_with_filters, token_logprobs)
from .constraints import ConstrainedRows, constrained_argmax, constraint_advance, constraint_mask
from .stopping import RunningWatch, StopCriteria, StopState, redirect_finished, stop_advance


@dataclass
class AttentionMetadata:
    """The struct every attention kernel call reads (same field names as the reference)."""

    kv_buffer: list = field(default_factory=list)        # per layer [max_tokens, 2*Hkv, D]
    cur_select_index: torch.Tensor | None = None          # rows written this step (int32)
    b_req_tokens_table: torch.Tensor | None = None        # [max_requests, max_seq_len] int32
    b_start_loc: torch.Tensor | None = None               # prefill only
    b_req_idx: torch.Tensor | None = None
    b_seq_len: torch.Tensor | None = None
    max_actual_seq_len: int = 0
    # chunk steps (extension): sequence b already holds b_ctx_len[b] tokens in the pool; b_seq_len / max_actual_seq_len
    # then count this step's new tokens only (the queries of prefill_paged_attention), max_ctx_len bounds b_ctx_len
    b_ctx_len: torch.Tensor | None = None
    max_ctx_len: int = 0
    kv_scales: tuple = (1.0, 1.0)                          # fp8 KV pool only (extension): stored value * scale = K / V
    # shared prompt prefix (extension): table[b_req_idx[b], :shared_prefix_len] == table[shared_prefix_req, :shared_prefix_len]
    # for every row of the batch; 0: no sharing.  Decode steps then read the prefix's K/V once per query tile
    # (kernels.shared_prefix_decode_attention) from kernels.attention.SHARED_PREFIX_MIN_LEN positions on
    shared_prefix_len: int = 0
    shared_prefix_req: int = 0


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


class KVPool:
    """Token-granular KV pool: one ``[max_tokens, 2*Hkv, D]`` fp16 tensor per layer (K heads first),
    with the reference's contiguous bump allocator (kv_cache_manager.py:197-216,286-292)."""

    def __init__(self, num_layers: int, max_tokens: int, num_kv_heads: int, head_dim: int, device,
                 dtype=torch.float16):
        self.max_tokens = max_tokens
        self.device = device
        self.kv_buffer = [torch.zeros(max_tokens, 2 * num_kv_heads, head_dim, dtype=dtype, device=device)
                          for _ in range(num_layers)]
        self._next = 0

    def alloc(self, n: int) -> torch.Tensor:
        if self._next + n > self.max_tokens:
            raise RuntimeError(f"KV pool exhausted: need {n} rows, {self.max_tokens - self._next} free")
        idx = torch.arange(self._next, self._next + n, dtype=torch.int32, device=self.device)
        self._next += n
        return idx

    def reset(self) -> None:
        self._next = 0

    def claim(self, num_rows: int) -> None:
        """Hand the first ``num_rows`` rows to an external owner (the slot layout); the bump cursor
        resumes just past them (kv_cache_manager.py:336-353)."""
        if num_rows > self.max_tokens:
            raise ValueError(f"cannot claim {num_rows} rows: the pool holds {self.max_tokens}")
        self._next = max(self._next, num_rows)

    @property
    def used(self) -> int:
        return self._next


class DecodeEngine:
    """One-shot batch generation: padded-grid prefill, then lockstep greedy decode.

    ``prefill`` mirrors ModelRunner.prefill_alloc_kv_cache/_init_req_tokens_table
    (model_runner.py:153-198): the ``[batch, max_prompt_len]`` grid is flattened row-major,
    ``b_start_loc[i] = i * max_prompt_len``; ``decode`` mirrors decode_alloc_kv_cache (:200-218):
    after every forward the next B rows are bump-allocated, ``b_seq_len += 1`` and the table is
    updated, so at ``flash_decoding`` time ``b_seq_len`` already counts the token being fed.
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
        if self.paged:
            from .paged_kv import PagedKVPool

            per_req = (max_seq_len + kv_block_size - 1) // kv_block_size
            self.pool = PagedKVPool(geo.num_layers, max_batch * per_req + 1, kv_block_size, at0.num_kv_heads, geo.head_dim,
                                    device, max_batch, max_seq_len, kv_dtype, share_blocks=self.share_blocks)
        else:
            self.pool = KVPool(geo.num_layers, max_batch * max_seq_len, at0.num_kv_heads, geo.head_dim, device, kv_dtype)
        self.info = AttentionMetadata(kv_buffer=self.pool.kv_buffer, kv_scales=tuple(float(v) for v in kv_scales))
        self.info.b_req_tokens_table = torch.zeros(max_batch, max_seq_len, dtype=torch.int32, device=device)
        self._graph = None
        self._graph_key = None
        self._sampling = None
        # log-probabilities (extension): of the token prefill returned / of every token of the last decode, when asked for
        self.first_logprobs: TokenLogprobs | None = None
        self.last_logprobs: TokenLogprobs | None = None
        self._prefill_logprobs = None
        self._logprobs_k = None
        self._lp = None
        # stopping (extension): per-row lengths / finish reasons / the steps run of the last decode, when it had ``stop``
        self.last_lengths: torch.Tensor | None = None
        self.last_finish_reasons: torch.Tensor | None = None
        self.last_steps_run: int | None = None
        self._stop: StopState | None = None
        # constrained decoding (extension): the rows' automaton states of the running prefill / decode, when it has ``constraint``
        self._constraint: ConstrainedRows | None = None
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
        self.first_logprobs = None
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
        if constraint is not None:
            constraint.reset()
            self._constraint = constraint
        self.info.shared_prefix_len, self.info.shared_prefix_req = 0, 0
        if num_samples is not None:
            return self._prefill_samples(prompt_ids, prompt_lens, sampling, chunk_size, int(num_samples))
        if shared_prefix_ids is not None:
            return self._first_tokens(self._prefill_shared(shared_prefix_ids, prompt_ids, prompt_lens, chunk_size), sampling)
        if chunk_size is not None:
            return self._first_tokens(self._prefill_chunked(prompt_ids, prompt_lens, int(chunk_size)), sampling)
        return self._first_tokens(self._prefill_one_step(prompt_ids, prompt_lens), sampling)

    def _prefill_one_step(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None, req_stride: int = 1,
                          collect=None) -> torch.Tensor:
        """The whole padded grid in one step; returns the logits of every sequence's last prompt token ``[B, vocab]``.
        ``req_stride``: prompt ``i`` is request ``i * req_stride`` (room for its samples; paged pool only).  ``collect``
        (:meth:`score`): called with ``(first column, final hidden states [B, width, hidden])`` in place of the lm_head;
        nothing is returned then."""
        b, lp = prompt_ids.shape
        dev = self.device
        self.pool.reset()
        if prompt_lens is None:
            prompt_lens = torch.full((b,), lp, dtype=torch.int32, device=dev)
        info = self.info
        info.b_req_idx = torch.arange(b, dtype=torch.int32, device=dev)
        if req_stride != 1:
            info.b_req_idx = info.b_req_idx * req_stride
        info.b_seq_len = prompt_lens.to(torch.int32).clone()
        info.max_actual_seq_len = lp
        info.b_start_loc = torch.arange(b, dtype=torch.int32, device=dev) * lp
        if self.paged:
            # blocks for the valid tokens only; the grid's pad positions write their junk K/V into the junk block
            info.cur_select_index = self.pool.admit(info.b_req_idx, info.b_seq_len, lp, info.b_req_tokens_table)
        else:
            info.cur_select_index = self.pool.alloc(b * lp)
            # table[i, j] = row of token j of sequence i on the padded grid, valid tokens only
            # (_init_req_tokens_table, model_runner.py:153-179); a sequence's pad rows hold junk K/V
            # that attention never reads, and its own decode steps name fresh rows
            valid = torch.arange(lp, device=dev).unsqueeze(0) < info.b_seq_len.view(b, 1)
            info.b_req_tokens_table[:b, :lp] = torch.where(valid, info.cur_select_index.view(b, lp),
                                                           info.b_req_tokens_table[:b, :lp])
        position_ids = torch.arange(lp, device=dev).unsqueeze(0).expand(b, lp)
        if collect is not None:
            collect(0, self.model.final_hidden_states(prompt_ids, position_ids, info))
            last = None
        else:
            rows = torch.arange(b, device=dev) * lp + (prompt_lens.long() - 1)
            last = self.model(prompt_ids, position_ids, info, logits_rows=rows)
        self._positions = prompt_lens.long().clone().view(b, 1)
        self._batch = b
        return last

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
        dev = self.device
        if chunk_size is not None:
            last = self._prefill_chunked(prompt_ids, prompt_lens, int(chunk_size), req_stride=n)
        else:
            last = self._prefill_one_step(prompt_ids, prompt_lens, req_stride=n)
        info = self.info
        lens = info.b_seq_len                                   # int32 [B], the prompts' lengths
        if n > 1:
            rows = torch.arange(b * n, dtype=torch.int32, device=dev)
            parents = info.b_req_idx.repeat_interleave(n - 1).contiguous()
            children = rows[rows % n != 0].contiguous()
            self.pool.fork(parents, children, lens.repeat_interleave(n - 1).contiguous(), info.b_req_tokens_table)
        info.b_req_idx = torch.arange(b * n, dtype=torch.int32, device=dev)
        info.b_seq_len = lens.repeat_interleave(n).contiguous()
        info.b_start_loc = torch.arange(b * n, dtype=torch.int32, device=dev) * lp
        info.max_actual_seq_len = lp
        self._positions = info.b_seq_len.long().view(b * n, 1)
        self._batch = b * n
        if b == 1 and n > 1:
            bs = self.pool.block_size
            info.shared_prefix_len, info.shared_prefix_req = (int(lens[0]) // bs) * bs, 0
        return self._first_tokens(last.repeat_interleave(n, dim=0), sampling)

    def _first_tokens(self, last: torch.Tensor, sampling) -> torch.Tensor:
        rows = self._constraint
        greedy = sampling is None or sampling.temperature == 0.0
        if rows is not None and greedy:
            tokens = constrained_argmax(last, rows)
        elif greedy:
            tokens = greedy_argmax(last)
        else:
            uniform = torch.rand(last.shape[0], device=self.device)
            drawn_from = last if rows is None else constraint_mask(last, rows)
            tokens = Sampler().sample(drawn_from, sampling, None, uniform=uniform).view(-1)
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
        info.b_req_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        info.b_seq_len = torch.full((1,), p, dtype=torch.int32, device=dev)
        info.max_actual_seq_len = p
        info.b_start_loc = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.paged:
            info.cur_select_index = self.pool.admit(info.b_req_idx, info.b_seq_len, p, table)
        else:
            info.cur_select_index = self.pool.alloc(p)
            table[0, :p] = info.cur_select_index
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
        total = tail_lens.to(device=dev, dtype=torch.int32) + p
        info.b_seq_len = total.clone()
        info.max_actual_seq_len = p + lt
        info.b_start_loc = torch.arange(b, dtype=torch.int32, device=dev) * (p + lt)
        self._positions = total.long().view(b, 1)
        info.shared_prefix_len, info.shared_prefix_req = p, 0
        if self.paged:
            info.shared_prefix_len = p // self.pool.block_size * self.pool.block_size
        return last

    def _prefill_chunked(self, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor | None, chunk_size: int,
                         ctx0: int = 0, req_stride: int = 1, collect=None) -> torch.Tensor:
        """Chunk steps over the prompt grid; returns the logits of every sequence's last prompt token ``[B, vocab]``.
        ``ctx0``: every sequence already holds that many cached positions (a shared prefix the table rows name); the pool is
        then left as it is and the grid's column ``j`` is position ``ctx0 + j``.  ``req_stride``: as in
        :meth:`_prefill_one_step`; so is ``collect``."""
        from .chunking import plan_prefill_chunks

        b, lp = prompt_ids.shape
        dev = self.device
        if ctx0 == 0:
            self.pool.reset()
        if prompt_lens is None:
            prompt_lens = torch.full((b,), lp, dtype=torch.int32, device=dev)
        plans = plan_prefill_chunks(prompt_lens.tolist(), lp, chunk_size)
        info = self.info
        table = info.b_req_tokens_table
        info.b_req_idx = torch.arange(b, dtype=torch.int32, device=dev)
        if req_stride != 1:
            info.b_req_idx = info.b_req_idx * req_stride
        last = None
        try:
            for ch in plans:
                w = ch.width
                info.b_seq_len = ch.b_q_len.to(dev)
                info.b_ctx_len = ch.b_ctx_len.to(dev) + ctx0
                info.b_start_loc = ch.b_start_loc.to(dev)
                info.max_actual_seq_len = w
                info.max_ctx_len = ch.max_ctx_len + ctx0
                if self.paged:
                    # blocks up to ctx + n only; pads write their junk K/V into the junk block
                    info.cur_select_index = self.pool.extend_at(info.b_req_idx, info.b_ctx_len, info.b_seq_len, w, table)
                else:
                    # B * width fresh rows; table[i, ctx_i + j] names them for valid tokens only (pads hold junk K/V)
                    info.cur_select_index = self.pool.alloc(b * w)
                    table[ch.valid_rows.to(dev), ch.valid_cols.to(dev) + ctx0] = info.cur_select_index[ch.valid_flat.to(dev)]
                if collect is not None:
                    collect(ch.col0, self.model.final_hidden_states(prompt_ids[:, ch.col0:ch.col0 + w].contiguous(),
                                                                    ch.positions.to(dev) + ctx0, info))
                    continue
                # a chunk that ends no sequence still computes one logits row (the lm_head takes no empty batch)
                rows = ch.logits_rows if ch.ends.numel() else torch.zeros(1, dtype=torch.int64)
                logits = self.model(prompt_ids[:, ch.col0:ch.col0 + w].contiguous(), ch.positions.to(dev) + ctx0, info,
                                    logits_rows=rows.to(dev))
                logits = logits.view(-1, logits.shape[-1])
                if last is None:
                    last = torch.empty(b, logits.shape[-1], dtype=logits.dtype, device=dev)
                if ch.ends.numel():
                    last[ch.ends.to(dev)] = logits
        finally:
            info.b_ctx_len, info.max_ctx_len = None, 0
        # the state a one-step prefill leaves: decode, graph capture and steps_per_graph run unchanged
        info.b_seq_len = prompt_lens.to(torch.int32).clone()
        info.max_actual_seq_len = lp
        info.b_start_loc = torch.arange(b, dtype=torch.int32, device=dev) * lp
        self._positions = prompt_lens.long().clone().view(b, 1)
        self._batch = b
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
        out = TokenLogprobs(torch.zeros(b, max(l - 1, 0), dtype=torch.float32, device=dev),
                            torch.zeros(b, max(l - 1, 0), k, dtype=torch.float32, device=dev),
                            torch.full((b, max(l - 1, 0), k), -1, dtype=torch.int64, device=dev))
        if l < 2:
            return out
        self.info.shared_prefix_len, self.info.shared_prefix_req = 0, 0
        hidden = torch.empty(b, l, self.model.geo.hidden_size, dtype=self.model.norm_weight.dtype, device=dev)

        def collect(col0, h):
            hidden[:, col0:col0 + h.shape[1]] = h.view(b, -1, hidden.shape[-1])

        if chunk_size is not None:
            self._prefill_chunked(token_ids, lens_t, int(chunk_size), collect=collect)
        else:
            self._prefill_one_step(token_ids, lens_t, collect=collect)
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
        got = TokenLogprobs(torch.empty(n, 1, dtype=torch.float32, device=dev),
                            torch.empty(n, 1, k, dtype=torch.float32, device=dev),
                            torch.empty(n, 1, k, dtype=torch.int64, device=dev))
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
        row of a sequence sits somewhere else) instead of one contiguous run per sequence."""
        dev = self.device
        self.pool.reset()
        info = self.info
        info.shared_prefix_len, info.shared_prefix_req = 0, 0
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        info.b_req_idx = torch.arange(batch, dtype=torch.int32, device=dev)
        if self.paged:
            lens = torch.full((batch,), ctx_len, dtype=torch.int32, device=dev)
            rows = self.pool.admit(info.b_req_idx, lens, ctx_len, info.b_req_tokens_table).long()  # fills the table
            for kv in self.pool.kv_buffer:
                kv[rows] = (torch.randn(batch * ctx_len, kv.shape[1], kv.shape[2], generator=g, device=dev) * 0.5).to(kv.dtype)
        else:
            rows = self.pool.alloc(batch * ctx_len)
            if scattered:
                rows = rows[torch.randperm(batch * ctx_len, generator=g, device=dev)]
            info.b_req_tokens_table[:batch, :ctx_len] = rows.view(batch, ctx_len)
            for kv in self.pool.kv_buffer:
                kv[: batch * ctx_len].copy_(
                    (torch.randn(batch * ctx_len, kv.shape[1], kv.shape[2], generator=g, device=dev) * 0.5).to(kv.dtype))
        info.b_seq_len = torch.full((batch,), ctx_len, dtype=torch.int32, device=dev)
        info.max_actual_seq_len = ctx_len
        self._positions = torch.full((batch, 1), ctx_len, dtype=torch.long, device=dev)
        self._batch = batch
        return torch.randint(0, self.model.geo.vocab_size, (batch,), generator=g, device=dev)

    # ------------------------------------------------------------------ decode ------ #
    def _begin_decode(self, first_tokens: torch.Tensor, max_new_tokens: int):
        b, dev, info = self._batch, self.device, self.info
        # decode_alloc_kv_cache for the first decode step
        info.b_seq_len = info.b_seq_len + 1
        info.max_actual_seq_len += 1
        if self.paged:
            # the row of position seq_len - 1 (a block is popped on the device when the position opens one); every
            # later step repeats this launch inside the step (graph included) -- nothing is reserved ahead
            info.cur_select_index = self.pool.append(info.b_req_idx, info.b_seq_len, info.b_req_tokens_table)
        else:
            info.cur_select_index = self.pool.alloc(b)
            update_kv_index(info.b_req_tokens_table, info.b_req_idx, info.b_seq_len, info.cur_select_index)
            # reserve the rows of all remaining steps now: the bump allocator hands out the next B
            # rows each step, which the graph reproduces on device as ``cur_select_index += B``
            if max_new_tokens > 1:
                self.pool.alloc(b * (max_new_tokens - 1))
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
        k = self._logprobs_k
        self._lp = None if k is None else TokenLogprobs(
            torch.zeros(b, max_new_tokens + 1, dtype=torch.float32, device=dev),
            torch.zeros(b, max_new_tokens + 1, k, dtype=torch.float32, device=dev),
            torch.full((b, max_new_tokens + 1, k), -1, dtype=torch.int64, device=dev))

    def _step_body(self):
        """forward -> greedy sample -> record -> advance metadata (all on device)."""
        info, b = self.info, self._batch
        logits = self.model(self._input_ids, self._positions, info)[:, -1, :]
        nxt = self._sample(logits)
        if self._lp is not None:
            # the model's own distribution: the raw logits (_sample penalises a copy); before _advance moves _step on
            token_logprobs(logits, nxt, self._logprobs_k, out=self._lp, column=self._step)
        self._advance(nxt)

    def _sample(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy argmax, or -- with ``sampling`` set by :meth:`decode` -- the reference sampler's sequence
        (repetition penalty over the tokens generated so far, then temperature + nucleus sampling) on
        the HIP kernels; the uniform numbers come from ``torch.rand`` (graph-safe Philox)."""
        sp = self._sampling
        rows = self._constraint
        # rows that were finished when the step began keep their automaton state
        finished = None if self._stop is None else self._stop.finished
        if sp is None:
            return greedy_argmax(logits) if rows is None else constrained_argmax(logits, rows, finished)
        b = self._batch
        generated = None
        if sp.repetition_penalty != 1.0:
            span = self._out.shape[1]
            mask = torch.arange(span, device=self.device).unsqueeze(0) < self._step  # [1, span] -> rows share it
            generated = _Span(self._out, mask.expand(b, span))
        uniform = torch.rand(b, device=self.device) if sp.temperature != 0.0 else None
        if rows is None:
            return Sampler().sample(logits, sp, generated, uniform=uniform).view(-1)
        # constrained: the penalty acts on the raw logits as it does above; greedy rows pick among the allowed tokens of
        # the (penalised) logits in one launch, sampled ones draw from a copy with the disallowed tokens at -inf
        if generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, sp.repetition_penalty)
        if sp.temperature == 0.0:
            return constrained_argmax(logits, rows, finished)
        # top_k / min_p of sp act on the masked copy: top-k counts among the allowed tokens
        nxt = sample_with_filters(constraint_mask(logits, rows), sp, uniform).view(-1)
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
        if self.paged:
            self._out.view(-1).scatter_(0, self._row_base + self._step, nxt)
            self._step += 1
            self._input_ids.copy_(nxt.view(b, 1))
            self._positions += 1
            info.b_seq_len += 1
            self.pool.append(info.b_req_idx, info.b_seq_len, t, out=info.cur_select_index)
            return
        if (nxt.dtype == torch.int64 and info.cur_select_index.dtype == torch.int32 and info.b_seq_len.dtype == torch.int32
                and info.b_req_idx.dtype == torch.int32 and t.dtype == torch.int32 and nxt.is_contiguous()
                and info.cur_select_index.is_contiguous() and info.b_seq_len.is_contiguous()
                and info.b_req_idx.is_contiguous()):
            L.check(
                L.lib().ll_decode_advance(
                    self._out.data_ptr(), self._out.stride(0), self._step.data_ptr(), nxt.data_ptr(),
                    self._input_ids.data_ptr(), self._positions.data_ptr(), info.cur_select_index.data_ptr(),
                    info.b_seq_len.data_ptr(), info.b_req_idx.data_ptr(), t.data_ptr(), t.stride(0), t.stride(1),
                    b, L.stream_ptr()),
                "decode_advance")
            return
        self._out.view(-1).scatter_(0, self._row_base + self._step, nxt)
        self._step += 1
        self._input_ids.copy_(nxt.view(b, 1))
        self._positions += 1
        info.cur_select_index += b
        info.b_seq_len += 1
        update_kv_index(info.b_req_tokens_table, info.b_req_idx, info.b_seq_len, info.cur_select_index)

    @torch.no_grad()
    def decode(self, first_tokens: torch.Tensor, max_new_tokens: int, use_graph: bool = True,
               warmup_steps: int = 0, on_step=None, sampling=None, steps_per_graph: int = 1,
               logprobs: int | None = None, stop: StopCriteria | None = None,
               constraint: ConstrainedRows | None = None) -> torch.Tensor:
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
        """
        self._constraint = None
        if constraint is not None:
            constraint.validate(self.model.geo.vocab_size, self._batch)
        self._logprobs_k = _check_logprobs(logprobs)
        self.last_logprobs = None
        self.last_lengths = self.last_finish_reasons = self.last_steps_run = None
        self._stop = None
        if stop is not None:
            stop.validate(self.model.geo.vocab_size, self._batch)
            self._stop = StopState(stop, first_tokens, self.device)
        self._constraint = constraint
        self._sampling = sampling  # None = greedy; else an object with temperature / top_p / repetition_penalty [/ top_k / min_p]
        self._begin_decode(first_tokens, max_new_tokens)
        watch = RunningWatch(self._stop) if stop is not None and stop.check_every > 0 else None
        steps_run = max_new_tokens
        info = self.info
        final_len = info.max_actual_seq_len + max_new_tokens
        if final_len > self.max_seq_len:
            raise RuntimeError(f"context {final_len} exceeds max_seq_len {self.max_seq_len}")
        if use_graph:
            info.max_actual_seq_len = (final_len + 127) // 128 * 128  # bucket, fixes the attention grid
            # warm-up on a side stream (workspace growth, library init), fenced both ways
            # (cuda_graph.py:110-115); state is restored afterwards
            snap = self._snapshot()
            s = getattr(self, "_warm_stream", None)  # ONE warm-up stream per engine: eager scratch is kept per stream
            if s is None:
                s = self._warm_stream = torch.cuda.Stream()
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
            graph = torch.cuda.CUDAGraph()
            try:
                with L.graph_capture(graph):
                    self._step_body()
            except Exception:
                # a refused capture (e.g. a collective the backend cannot record) must not leave the stream in capture
                # mode: the caller falls back to eager launches on this very stream
                try:
                    if torch.cuda.is_current_stream_capturing():
                        graph.capture_end()
                except Exception:
                    pass
                self._restore(snap)
                raise
            self._restore(snap)  # capture does not execute, but keep the state explicit
            self._graph = graph
            group = max(1, min(int(steps_per_graph), max_new_tokens))
            multi = None
            if group > 1:
                multi = torch.cuda.CUDAGraph()
                with L.graph_capture(multi):
                    for _ in range(group):
                        self._step_body()
                self._restore(snap)
                self._graph_multi = multi
            i = 0
            while i < max_new_tokens:
                if on_step is not None:
                    on_step(i)
                if multi is not None and max_new_tokens - i >= group:
                    multi.replay()
                    i += group
                else:
                    graph.replay()
                    i += 1
                if watch is not None and watch.all_finished(i):
                    steps_run = i
                    break
        else:
            for i in range(max_new_tokens):
                if on_step is not None:
                    on_step(i)
                info.max_actual_seq_len = int(info.max_actual_seq_len)  # eager: exact value
                self._step_body()
                info.max_actual_seq_len += 1
                if watch is not None and watch.all_finished(i + 1):
                    steps_run = i + 1
                    break
        self._check_device_errors()
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

    def _check_device_errors(self) -> None:
        """Sticky device-side error words, read where the host synchronises anyway (end of a decode): a lost peer of the
        one-shot all-reduce, an exhausted / misused block pool.  Nothing to read (and no synchronisation) otherwise."""
        from ..distributed import parallel_state as ps

        if ps._ONESHOT is not None:
            ps.check_collective_errors()
        if L.gemm_scratch_error(torch.device(self.device)):
            raise RuntimeError("a split-K GEMM merge gave up waiting for a contributor workgroup: its output tile was poisoned "
                               "with NaN and the merge counters are not zero at rest")
        if self.paged:
            err = self.pool.error
            if err:
                raise RuntimeError(f"paged KV pool reported error bits {err:#x} (1: a call found too few free blocks, "
                                   "2: a request outgrew its block-table / token-table row, 4: a fork "
                                   "broke its contract)")
        if self._constraint is not None:
            err = int(self._constraint.error.item())
            if err:
                raise RuntimeError(f"constrained decoding reported error bits {err:#x} (1: a row was to follow a token its "
                                   "automaton state does not allow, 2: a row's state lies outside the automaton)")

    def _snapshot(self):
        # The log-probability buffers (_lp) have no place here: the warm-up step and the capture write the very column
        # (_step, which IS restored) that the first replay writes again, with the same values.
        info = self.info
        return (self._input_ids.clone(), self._positions.clone(), info.cur_select_index.clone(),
                info.b_seq_len.clone(), self._step.clone(), self._out.clone(),
                info.b_req_tokens_table.clone(), self.pool.snapshot() if self.paged else None,
                None if self._stop is None else [t.clone() for t in self._stop.tensors()],
                None if self._constraint is None else [t.clone() for t in self._constraint.tensors()])

    def _restore(self, snap):
        info = self.info
        self._input_ids.copy_(snap[0])
        self._positions.copy_(snap[1])
        info.cur_select_index.copy_(snap[2])
        info.b_seq_len.copy_(snap[3])
        self._step.copy_(snap[4])
        self._out.copy_(snap[5])
        info.b_req_tokens_table.copy_(snap[6])
        if self.paged:
            self.pool.restore(snap[7])
        if self._stop is not None:
            for t, saved in zip(self._stop.tensors(), snap[8]):
                t.copy_(saved)
        if self._constraint is not None:
            for t, saved in zip(self._constraint.tensors(), snap[9]):
                t.copy_(saved)


from .chunking import ChunkPlan, plan_prefill_chunks  # noqa: E402,F401
from .slots import DEFAULT_BATCH_SIZES, DEFAULT_SEQ_LEN_BUCKETS, SlotBatch, SlotRunner, StepGraphs, slot_advance  # noqa: E402,F401
from .kv_cache_manager import KVCacheManager  # noqa: E402,F401
from .stopping import MAX_STOP_SEQUENCE_LEN, MAX_STOP_SEQUENCES, MAX_STOP_TOKEN_IDS  # noqa: E402,F401
from .constraints import TokenAutomaton, from_choices, from_transitions, union  # noqa: E402,F401
