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


class LogitBias:
    """A sparse additive bias on the logits, per row, as the device CSR ``ll_logit_penalties`` reads: ``offsets`` int32
    ``[batch + 1]``, ``ids`` int32 and ``values`` fp32 ``[offsets[-1]]``.  Built once per call from ``bias``: one
    ``{token: bias}`` dict for every row, or a list of ``batch`` dicts / ``None``s (``None``: that row has no bias).
    Validated on the host: ids inside ``[0, vocab)``, values finite or ``-inf`` (a ban; ``+inf`` and NaN are refused)."""

    def __init__(self, bias, batch: int, vocab: int, device):
        per_row = [bias] * batch if bias is None or isinstance(bias, dict) else list(bias)
        if len(per_row) != batch:
            raise ValueError(f"logit_bias names {len(per_row)} rows for a batch of {batch}")
        offsets, ids, values = [0], [], []
        checked = set()  # a dict that serves every row is checked once
        for row in per_row:
            if row is not None and not isinstance(row, dict):
                raise ValueError("logit_bias must be a {token: bias} dict, or a list of such dicts and Nones")
            if row and id(row) not in checked:
                checked.add(id(row))
                for tok, val in row.items():
                    if isinstance(tok, bool) or not isinstance(tok, int) or not 0 <= tok < vocab:
                        raise ValueError(f"logit_bias names token {tok!r} outside the vocabulary of {vocab}")
                    val = float(val)
                    if val != val or val == float("inf"):
                        raise ValueError(f"logit_bias of token {tok} is {val}: it must be finite or -inf")
            if row:
                ids.extend(int(t) for t in row)
                values.extend(float(v) for v in row.values())
            offsets.append(len(ids))
        self.batch, self.vocab = batch, vocab
        self.offsets = torch.tensor(offsets, dtype=torch.int32, device=device)
        # never empty: the kernel is handed valid pointers even when no row names a token
        self.ids = torch.tensor(ids or [0], dtype=torch.int32, device=device)
        self.values = torch.tensor(values or [0.0], dtype=torch.float32, device=device)

    @classmethod
    def of(cls, bias, batch: int, vocab: int, device) -> "LogitBias | None":
        """``bias`` as a :class:`LogitBias` for ``[batch, vocab]`` logits: ``None`` stays ``None``, one already built is
        checked against the shape, a dict or a list is built."""
        if bias is None:
            return None
        if isinstance(bias, cls):
            if bias.batch != batch or bias.vocab != vocab:
                raise ValueError(f"the LogitBias was built for {bias.batch} x {bias.vocab} logits, not {batch} x {vocab}")
            return bias
        return cls(bias, batch, vocab, device)


def apply_penalties(logits: torch.Tensor, token_ids: torch.Tensor | None, mask: torch.Tensor | None,
                    repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None) -> torch.Tensor:
    """New ``[batch, vocab]`` logits after the repetition, presence and frequency penalties over the generated span
    ``token_ids`` / ``mask`` ``[batch, span]`` and the additive ``logit_bias`` (a :class:`LogitBias`, a dict or a list of
    dicts), in one launch and one read of the logits (csrc/sampler_penalties.hip).  With ``c[v]`` the number of masked-in
    span entries equal to ``v``, every token's value is computed in fp32 from the stored logit ``z[v]``:
    ``x = z[v] + bias[v]``; if ``c[v] > 0``: ``x = x * r if x < 0 else x / r``; ``x = x - f * c[v] - (p if c[v] > 0 else 0)``.
    Each penalty is a Python scalar or a ``[batch]`` / ``[batch, 1]`` tensor; the result dtype is that of
    :func:`apply_repetition_penalty`: scalars keep the logits dtype, any tensor penalty promotes.  ``token_ids`` / ``mask``
    may be ``None`` when only a bias is given.  With ``p = f = 0`` and no bias the result is bit-equal to
    :func:`apply_repetition_penalty`'s, which stays the route for repetition-only calls."""
    L.require_cuda(logits, token_ids, mask)
    if logits.dim() != 2:
        raise ValueError("logits must be [batch, vocab]")
    batch, vocab = logits.shape
    if (token_ids is None) != (mask is None):
        raise ValueError("token_ids and mask come together")
    if token_ids is not None and (token_ids.shape != mask.shape or token_ids.dim() != 2 or token_ids.shape[0] != batch):
        raise ValueError("logits [batch, vocab], token_ids / mask [batch, span]")
    if not torch.is_tensor(repetition_penalty) and not float(repetition_penalty) > 0.0:
        raise ValueError(f"repetition_penalty must be positive, got {repetition_penalty}")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    bias = LogitBias.of(logit_bias, batch, vocab, logits.device)
    ids = msk = None
    span = 0
    if token_ids is not None and token_ids.shape[1] > 0:
        ids = token_ids.to(torch.int64).contiguous()
        msk = mask.to(torch.bool).contiguous()
        span = ids.shape[1]
    out_dtype = logits.dtype
    rows, scalars = [], []
    for pen, neutral in ((repetition_penalty, 1.0), (presence_penalty, 0.0), (frequency_penalty, 0.0)):
        if torch.is_tensor(pen):
            L.require_cuda(pen)
            t = pen.reshape(-1).to(torch.float32).contiguous()
            if t.numel() != batch:
                raise ValueError("a tensor penalty needs one entry per row")
            out_dtype = torch.promote_types(out_dtype, pen.dtype)
            rows.append(t)
            scalars.append(neutral)
        else:
            rows.append(None)
            scalars.append(float(pen))
    out = torch.empty((batch, vocab), dtype=out_dtype, device=logits.device)
    L.check(
        L.lib().ll_logit_penalties(
            out.data_ptr(), logits.data_ptr(), L.ptr(ids), L.ptr(msk), L.ptr(rows[0]), scalars[0], L.ptr(rows[1]),
            scalars[1], L.ptr(rows[2]), scalars[2], L.ptr(bias.offsets if bias else None),
            L.ptr(bias.ids if bias else None), L.ptr(bias.values if bias else None), batch, vocab, span,
            logits.stride(0), out.stride(0), ids.stride(0) if span else 0, msk.stride(0) if span else 0,
            L.dtype_code(logits.dtype), L.dtype_code(out_dtype), L.stream_ptr()),
        "apply_penalties")
    return out


def seeded_uniform(seeds: torch.Tensor, column: torch.Tensor | None = None) -> torch.Tensor:
    """``seeds [batch]`` (int64) -> fp32 ``[batch]`` in ``[0, 1)``: row ``b``'s number is the top 24 bits of the first
    Philox4x32-10 word at key ``seeds[b]`` and counter ``column`` (a one-element int64 device tensor, read on the device
    so a captured launch follows a counter the graph advances; ``None``: 0).  A row's numbers depend on its seed and the
    counter alone -- not on the batch it sits in, nor on what else has drawn random numbers."""
    L.require_cuda(seeds, column)
    if seeds.dtype != torch.int64 or seeds.dim() != 1:
        raise ValueError("seeds must be an int64 [batch] tensor")
    if column is not None and (column.dtype != torch.int64 or column.numel() != 1):
        raise ValueError("column must be a one-element int64 tensor")
    seeds = seeds.contiguous()
    out = torch.empty(seeds.numel(), dtype=torch.float32, device=seeds.device)
    L.check(L.lib().ll_seeded_uniform(out.data_ptr(), seeds.data_ptr(), L.ptr(column), seeds.numel(), L.stream_ptr()),
            "seeded_uniform")
    return out


def row_seeds(seed, batch: int, device) -> torch.Tensor | None:
    """``SamplingParams.seed`` as the int64 ``[batch]`` seeds of :func:`seeded_uniform`: ``None`` stays ``None``, an int
    ``s`` gives row ``i`` the seed ``s + i`` (wrapping to int64), a sequence gives one seed per row."""
    if seed is None:
        return None
    if isinstance(seed, int):
        values = [seed + i for i in range(batch)]
    else:
        values = [int(s) for s in (seed.tolist() if torch.is_tensor(seed) else seed)]
        if len(values) != batch:
            raise ValueError(f"seed names {len(values)} rows for a batch of {batch}")
    return torch.tensor([(v + 2 ** 63) % 2 ** 64 - 2 ** 63 for v in values], dtype=torch.int64, device=device)


@dataclass
class SamplingParams:
    """The sampling options :class:`Sampler` and ``DecodeEngine`` read, in one place (any object with ``temperature``,
    ``top_p`` and ``repetition_penalty`` keeps being accepted).  ``logit_bias``: see :class:`LogitBias`; ``seed``: see
    :func:`row_seeds` -- read by the engine, which owns the draw."""

    temperature: float = 1.0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    top_k: int = 0
    min_p: float = 0.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: object = None
    seed: object = None


def _penalty_off(value) -> bool:
    return value is None or (not torch.is_tensor(value) and float(value) == 0.0)


def _extras_off(presence, frequency, bias) -> bool:
    """Presence penalty, frequency penalty and bias off for every row, decided on the host without reading a tensor."""
    return bias is None and _penalty_off(presence) and _penalty_off(frequency)


def _extras(params):
    return (getattr(params, "presence_penalty", 0.0), getattr(params, "frequency_penalty", 0.0),
            getattr(params, "logit_bias", None))


def resolve_sampling(params, batch: int, vocab: int, device):
    """What an engine does once per call with the caller's parameter object -> ``(params, seeds)``: ``seeds`` are
    :func:`row_seeds` of ``params.seed`` (``None`` without one), and a ``logit_bias`` given as a dict or a list is built
    into its :class:`LogitBias` on a copy of the parameters, so that no step builds it again (a step may be captured).
    An object without ``logit_bias`` and ``seed`` comes back as it is, and nothing is put on the device."""
    if params is None:
        return None, None
    seeds = row_seeds(getattr(params, "seed", None), batch, device)
    presence, frequency, bias = _extras(params)
    if bias is None:
        return params, seeds
    built = LogitBias.of(bias, batch, vocab, device)
    if built is bias:
        return params, seeds
    return SamplingParams(params.temperature, params.top_p, params.repetition_penalty, getattr(params, "top_k", 0),
                          getattr(params, "min_p", 0.0), presence, frequency, built, getattr(params, "seed", None)), seeds


def _penalise(logits, params, generated, presence, frequency, bias) -> torch.Tensor:
    """:func:`apply_penalties` in :func:`apply_repetition_penalty`'s place; with a bias also without a generated span."""
    if generated is None and bias is None:
        return logits
    ids, mask = (None, None) if generated is None else (generated.token_ids, generated.mask)
    return apply_penalties(logits, ids, mask, params.repetition_penalty, 0.0 if presence is None else presence,
                           0.0 if frequency is None else frequency, bias)


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
    ``sample_batched``) and, optionally, ``top_k`` / ``min_p`` (extension, default off: scalars or per-row tensors) and
    ``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` (extension, default off: with any of them on,
    :func:`apply_penalties` takes :func:`apply_repetition_penalty`'s place, and a bias acts without ``generated`` too);
    ``generated``: object with ``token_ids`` and ``mask``."""

    @torch.no_grad()
    def sample(self, logits, params, generated=None, uniform=None):
        if logits.dim() == 3:
            logits = logits[:, -1, :]
        extras = _extras(params)
        if not _extras_off(*extras):
            logits = _penalise(logits, params, generated, *extras)
        elif params.repetition_penalty != 1.0 and generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, params.repetition_penalty)
        if params.temperature == 0.0:
            return greedy_argmax(logits).view(-1, 1)
        return sample_with_filters(logits, params, uniform)

    @torch.no_grad()
    def sample_batched(self, logits, params, generated=None, uniform=None):
        if logits.dim() == 3:
            logits = logits[:, -1, :]
        extras = _extras(params)
        if not _extras_off(*extras):
            logits = _penalise(logits, params, generated, *extras)
        elif params.any_penalty and generated is not None:
            logits = apply_repetition_penalty(logits, generated.token_ids, generated.mask, params.repetition_penalty)
        if params.all_greedy:
            return greedy_argmax(logits).view(-1, 1)
        return sample_with_filters(logits, params, uniform, greedy=params.greedy)
