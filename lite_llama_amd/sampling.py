"""Sampling step after the hot path -- mirror of lite_llama/engine/sampler.py: greedy argmax
(:227-228,264), HuggingFace-style repetition penalty (:77-115) and temperature + nucleus sampling
(:118-137), as HIP kernels so the decode step stays on one stream (the reference's nucleus path is
softmax + a full-vocabulary sort + cumsum + multinomial per step).  ``token_logprobs`` (extension: the reference
reports no probabilities) is the third kernel of the row: log-probability of a token and the top-k alternatives."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib as L


def greedy_argmax(logits: torch.Tensor) -> torch.Tensor:
    """``[..., V] -> [...]`` int64 token ids (first maximum, like ``torch.argmax``)."""
    L.require_cuda(logits)
    v = logits.shape[-1]
    flat = logits.reshape(-1, v)
    if flat.stride(-1) != 1:
        flat = flat.contiguous()
    out = torch.empty(flat.shape[0], dtype=torch.int64, device=logits.device)
    rows = flat.shape[0]
    if v >= 16384 and rows < 1024:
        # vocabulary-sized rows at decode batch: spread each row over several workgroups
        chunks = max(1, min(64, 2048 // max(rows, 1), v // 4096))
        scratch = torch.empty(rows * chunks * 2, dtype=torch.int64, device=logits.device)
        L.check(
            L.lib().ll_argmax_split(out.data_ptr(), flat.data_ptr(), rows, v, flat.stride(0),
                                    L.dtype_code(logits.dtype), scratch.data_ptr(), chunks, L.stream_ptr()),
            "greedy_argmax",
        )
        return out.view(logits.shape[:-1])
    L.check(
        L.lib().ll_argmax(out.data_ptr(), flat.data_ptr(), flat.shape[0], v, flat.stride(0),
                          L.dtype_code(logits.dtype), L.stream_ptr()),
        "greedy_argmax",
    )
    return out.view(logits.shape[:-1])

MAX_TOP_LOGPROBS = 20


@dataclass
class TokenLogprobs:
    """Log-probabilities of ``T`` tokens per row under the model's own distribution (log-softmax of the raw logits).
    ``chosen [rows, T]`` fp32: the named token's (None when none was named); ``top_logprobs [rows, T, k]`` fp32 and
    ``top_ids [rows, T, k]`` int64: the ``k`` most likely tokens, ordered by (logit descending, token id ascending)."""

    chosen: torch.Tensor | None
    top_logprobs: torch.Tensor
    top_ids: torch.Tensor

    @classmethod
    def blank(cls, rows: int, t: int, k: int, device) -> "TokenLogprobs":
        """Buffers for ``t`` tokens per row and ``k`` alternatives, at the values of "nothing reported": 0.0 / 0.0 / id -1."""
        return cls(torch.zeros(rows, t, dtype=torch.float32, device=device),
                   torch.zeros(rows, t, k, dtype=torch.float32, device=device),
                   torch.full((rows, t, k), -1, dtype=torch.int64, device=device))

    def cumulative(self, lengths: torch.Tensor | None = None) -> torch.Tensor:
        """``[rows]``: the sum of ``chosen`` over the first ``lengths[i]`` columns of row ``i`` (all columns by default) --
        a sample's cumulative log-probability, a scored text's log-likelihood."""
        if self.chosen is None:
            raise ValueError("no token was named: there is no chosen log-probability to add up")
        if lengths is None:
            return self.chosen.sum(dim=1)
        cols = torch.arange(self.chosen.shape[1], device=self.chosen.device).unsqueeze(0)
        keep = cols < lengths.to(self.chosen.device).reshape(-1, 1)
        return torch.where(keep, self.chosen, torch.zeros_like(self.chosen)).sum(dim=1)


def token_logprobs(logits: torch.Tensor, token_ids: torch.Tensor | None = None, top_k: int = 0, *,
                   out: TokenLogprobs | None = None, column: torch.Tensor | None = None) -> TokenLogprobs:
    """``logits [rows, vocab]`` (fp16 / bf16 / fp32) -> :class:`TokenLogprobs` of ``token_ids [rows]`` (int64, optional)
    and the ``top_k`` (0 .. 20) most likely tokens, in one read of the logits (csrc/logprobs.hip).  Without ``out`` the
    result has ``T = 1``.  ``out``: buffers ``[rows, T]`` / ``[rows, T, top_k]`` to write into, at the column held by the
    one-element int64 device tensor ``column`` (column 0 without it) -- the column is read on the device, so a launch
    captured in a hipGraph follows a counter that the graph itself advances.  An id outside ``[0, vocab)`` gives NaN."""
    top_k = int(top_k)
    if not 0 <= top_k <= MAX_TOP_LOGPROBS:
        raise ValueError(f"top_k must be in 0 .. {MAX_TOP_LOGPROBS}, got {top_k}")
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be [rows, vocab]")
    rows, vocab = logits.shape
    if top_k > vocab:
        raise ValueError(f"top_k {top_k} exceeds the vocabulary {vocab}")
    if token_ids is None and top_k == 0:
        raise ValueError("nothing to compute: name token_ids, ask for top_k > 0, or both")
    if token_ids is not None and (token_ids.dtype != torch.int64 or token_ids.numel() != rows):
        raise ValueError(f"token_ids must be int64 with one id per row of logits ({rows})")
    if column is not None and (column.dtype != torch.int64 or column.numel() != 1):
        raise ValueError("column must be a one-element int64 tensor")
    if column is not None and out is None:
        raise ValueError("column addresses the buffers of out")
    if out is not None:
        ch, tl, ti = out.chosen, out.top_logprobs, out.top_ids
        if token_ids is not None and (ch is None or ch.dim() != 2 or ch.shape[0] != rows or ch.dtype != torch.float32
                                      or ch.stride(1) != 1):
            raise ValueError("out.chosen must be float32 [rows, T] with unit column stride")
        t = ch.shape[1] if token_ids is not None else tl.shape[1]
        if top_k > 0 and (tl.shape != (rows, t, top_k) or ti.shape != (rows, t, top_k) or tl.dtype != torch.float32
                          or ti.dtype != torch.int64 or tl.stride()[1:] != (top_k, 1) or ti.stride()[1:] != (top_k, 1)):
            raise ValueError("out.top_logprobs (float32) / out.top_ids (int64) must be [rows, T, top_k], columns packed")
        if t < 1:
            raise ValueError("out has no column")
    L.require_cuda(logits, token_ids, column, *(() if out is None else (out.chosen, out.top_logprobs, out.top_ids)))
    code = L.dtype_code(logits.dtype)
    dev = logits.device
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    if out is None:
        t = 1
        out = TokenLogprobs(torch.empty(rows, 1, dtype=torch.float32, device=dev) if token_ids is not None else None,
                            torch.empty(rows, 1, top_k, dtype=torch.float32, device=dev),
                            torch.empty(rows, 1, top_k, dtype=torch.int64, device=dev))
    if rows == 0:
        return out
    ids = None if token_ids is None else token_ids.reshape(-1).contiguous()
    need = L.lib().ll_token_logprobs_scratch_bytes(rows, vocab, top_k)
    if need < 0:
        L.check(int(need), "token_logprobs")
    scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
    ch = out.chosen if token_ids is not None else None
    L.check(
        L.lib().ll_token_logprobs(L.ptr(ch), out.top_logprobs.data_ptr() if top_k else 0,
                                  out.top_ids.data_ptr() if top_k else 0, logits.data_ptr(), L.ptr(ids), L.ptr(column),
                                  rows, vocab, logits.stride(0), top_k, t, ch.stride(0) if ch is not None else 0,
                                  out.top_logprobs.stride(0) if top_k else 0, out.top_ids.stride(0) if top_k else 0,
                                  code, scratch.data_ptr(), need, L.stream_ptr()),
        "token_logprobs")
    return out


def apply_repetition_penalty(logits: torch.Tensor, token_ids: torch.Tensor, mask: torch.Tensor, penalty) -> torch.Tensor:
    """``apply_repetition_penalty(logits, GeneratedSpan(token_ids, mask), penalty)`` of the reference:
    new ``[batch, vocab]`` logits, generated tokens divided by ``penalty`` when >= 0 and multiplied when
    negative (each token once).  ``penalty``: Python scalar (result keeps the logits dtype) or a
    ``[batch, 1]`` / ``[batch]`` float32 tensor (result float32 for fp16 logits -- torch's promotion)."""
    L.require_cuda(logits, token_ids, mask)
    if logits.dim() != 2 or token_ids.shape != mask.shape or token_ids.shape[0] != logits.shape[0]:
        raise ValueError("logits [batch, vocab], token_ids / mask [batch, span]")
    batch, vocab = logits.shape
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    ids = token_ids.to(torch.int64).contiguous()
    msk = mask.to(torch.bool).contiguous()
    if torch.is_tensor(penalty):
        L.require_cuda(penalty)
        pen_rows = penalty.reshape(-1).to(torch.float32).contiguous()
        if pen_rows.numel() != batch:
            raise ValueError("a tensor penalty needs one entry per row")
        out_dtype = torch.promote_types(logits.dtype, penalty.dtype)
        scalar = 1.0
    else:
        pen_rows, out_dtype, scalar = None, logits.dtype, float(penalty)
    out = torch.empty((batch, vocab), dtype=out_dtype, device=logits.device)
    L.check(
        L.lib().ll_repetition_penalty(
            out.data_ptr(), logits.data_ptr(), ids.data_ptr(), msk.data_ptr(), L.ptr(pen_rows), scalar, batch, vocab,
            ids.shape[1], logits.stride(0), out.stride(0), ids.stride(0), msk.stride(0),
            L.dtype_code(logits.dtype), L.dtype_code(out_dtype), L.stream_ptr()),
        "apply_repetition_penalty")
    return out


def sample_top_p(logits: torch.Tensor, temperature, top_p, uniform: torch.Tensor | None = None,
                 greedy: torch.Tensor | None = None) -> torch.Tensor:
    """Temperature + nucleus sampling of ``[batch, vocab]`` logits -> int64 ``[batch, 1]`` ids, the
    reference's ``sample_top_p(softmax(logits / temperature), top_p)`` in one launch and without the
    sort.  ``temperature`` / ``top_p``: scalars or per-row tensors; ``uniform``: one number in [0, 1)
    per row (default ``torch.rand``): the draw is the inverse CDF over the nucleus in token order;
    ``greedy`` (bool per row, optional): those rows return the first argmax instead."""
    L.require_cuda(logits, uniform, greedy)
    if logits.dim() != 2:
        raise ValueError("logits must be [batch, vocab]")
    batch, vocab = logits.shape
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    dev = logits.device

    def rows(v):
        if torch.is_tensor(v):
            t = v.reshape(-1).to(device=dev, dtype=torch.float32)
            return t.expand(batch).contiguous() if t.numel() == 1 else t.contiguous()
        return torch.full((batch,), float(v), dtype=torch.float32, device=dev)

    t, p = rows(temperature), rows(top_p)
    u = torch.rand(batch, device=dev) if uniform is None else uniform.reshape(-1).to(torch.float32).contiguous()
    g = None if greedy is None else greedy.reshape(-1).to(torch.bool).contiguous()
    if t.numel() != batch or p.numel() != batch or u.numel() != batch or (g is not None and g.numel() != batch):
        raise ValueError("per-row sampling knobs need one entry per row")
    out = torch.empty(batch, dtype=torch.int64, device=dev)
    L.check(
        L.lib().ll_sample_top_p(out.data_ptr(), logits.data_ptr(), t.data_ptr(), p.data_ptr(), u.data_ptr(), L.ptr(g),
                                batch, vocab, logits.stride(0), L.dtype_code(logits.dtype), L.stream_ptr()),
        "sample_top_p")
    return out.view(batch, 1)


def _filter_off(top_k, min_p) -> bool:
    """Both filters off for every row, decided on the host without reading a tensor: ``None`` or Python scalars only."""
    k_off = top_k is None or (not torch.is_tensor(top_k) and int(top_k) <= 0)
    return k_off and (min_p is None or (not torch.is_tensor(min_p) and float(min_p) == 0.0))


def sample_filtered(logits: torch.Tensor, temperature, top_p, top_k=0, min_p=0.0, uniform: torch.Tensor | None = None,
                    greedy: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`sample_top_p` with a top-k and a min-p filter in the same single launch (csrc/sampler_filters.hip) -> int64
    ``[batch, 1]``.  Per row: the ``top_k`` largest stored logits survive, with every token tied with the k-th
    (``<= 0`` or ``>= vocab``: off); the nucleus of ``top_p`` is chosen among the survivors; a kept token whose probability
    is below ``min_p`` times the largest one is then dropped (``0``: off); the draw is the inverse CDF in token order over
    what is left.  ``top_k`` (int) and ``min_p`` (float in [0, 1]): scalars, per-row tensors, or ``None`` for off (the
    entries of a tensor are not validated: a ``min_p`` entry that is negative or NaN is off, one above 1 counts as 1); the
    other arguments as in :func:`sample_top_p`.  A row with both filters off draws the token ``sample_top_p`` draws."""
    L.require_cuda(logits, uniform, greedy)
    if logits.dim() != 2:
        raise ValueError("logits must be [batch, vocab]")
    batch, vocab = logits.shape
    if not torch.is_tensor(min_p) and min_p is not None and not 0.0 <= float(min_p) <= 1.0:
        raise ValueError(f"min_p must be in [0, 1], got {min_p}")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    dev = logits.device

    def rows(v, dtype=torch.float32):
        if v is None:
            return None
        if torch.is_tensor(v):
            t = v.reshape(-1).to(device=dev, dtype=dtype)
            return t.expand(batch).contiguous() if t.numel() == 1 else t.contiguous()
        return torch.full((batch,), v, dtype=dtype, device=dev)

    t, p, mp = rows(temperature), rows(top_p), rows(min_p)
    if top_k is not None and not torch.is_tensor(top_k):
        top_k = max(0, min(int(top_k), vocab))  # beyond the vocabulary is off, like vocab itself: fits int32
    k = rows(top_k, torch.int32)
    u = torch.rand(batch, device=dev) if uniform is None else uniform.reshape(-1).to(torch.float32).contiguous()
    g = None if greedy is None else greedy.reshape(-1).to(torch.bool).contiguous()
    if any(x is not None and x.numel() != batch for x in (t, p, k, mp, u, g)):
        raise ValueError("per-row sampling knobs need one entry per row")
    out = torch.empty(batch, dtype=torch.int64, device=dev)
    L.check(
        L.lib().ll_sample_filtered(out.data_ptr(), logits.data_ptr(), t.data_ptr(), p.data_ptr(), L.ptr(k), L.ptr(mp),
                                   u.data_ptr(), L.ptr(g), batch, vocab, logits.stride(0), L.dtype_code(logits.dtype),
                                   L.stream_ptr()),
        "sample_filtered")
    return out.view(batch, 1)


def sample_with_filters(logits, params, uniform, greedy=None) -> torch.Tensor:
    """The draw of :class:`Sampler`: ``top_k`` / ``min_p`` are read from ``params`` with the defaults 0 and 0.0 (the
    reference's parameter objects lack them; ``None`` is off too); with both off this is :func:`sample_top_p`, the launch it has always been."""
    top_k, min_p = getattr(params, "top_k", 0), getattr(params, "min_p", 0.0)
    if _filter_off(top_k, min_p):
        return sample_top_p(logits, params.temperature, params.top_p, uniform, greedy=greedy)
    return sample_filtered(logits, params.temperature, params.top_p, top_k, min_p, uniform, greedy=greedy)


class Sampler:
    """``Sampler.sample`` / ``sample_batched`` of the reference (sampler.py:199-270) on the kernels above.
    ``params``: any object with ``temperature``, ``top_p``, ``repetition_penalty`` (scalars for
    ``sample``; ``[batch, 1]`` tensors plus ``greedy`` / ``all_greedy`` / ``any_penalty`` for
    ``sample_batched``) and, optionally, ``top_k`` / ``min_p`` (extension, default off: scalars or per-row tensors);
    ``generated``: object with ``token_ids`` and ``mask``."""

    @torch.no_grad()
    def sample(self, logits, params, generated=None, uniform=None):
        if logits.dim() == 3:
            logits = logits[:, -1, :]
        if params.repetition_penalty != 1.0 and generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, params.repetition_penalty)
        if params.temperature == 0.0:
            return greedy_argmax(logits).view(-1, 1)
        return sample_with_filters(logits, params, uniform)

    @torch.no_grad()
    def sample_batched(self, logits, params, generated=None, uniform=None):
        if logits.dim() == 3:
            logits = logits[:, -1, :]
        if params.any_penalty and generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, params.repetition_penalty)
        if params.all_greedy:
            return greedy_argmax(logits).view(-1, 1)
        return sample_with_filters(logits, params, uniform, greedy=params.greedy)
