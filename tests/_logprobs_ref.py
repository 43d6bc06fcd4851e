"""Reference for the token log-probability kernel and everything built on it, written from the contract, not from the
kernel: the fp64 ``log_softmax`` of the stored values; the top-k by a stable sort on (-value, index), i.e. ordered by
(logit descending, token index ascending) -- not ``torch.topk``, whose order among equal values is unspecified."""

import torch

ATOL, RTOL = 2e-5, 1e-6  # |got - ref| <= ATOL + RTOL * |ref| (fp32 accumulation of the kernel, see test_logprobs_gpu.py)
_PLAIN_SORT_MAX = 1 << 22  # rows x vocab up to which the whole matrix is sorted


def _top_ids_plain(z: torch.Tensor, k: int) -> torch.Tensor:
    return torch.sort(-z, dim=-1, stable=True).indices[:, :k]


def _top_ids_prefiltered(z: torch.Tensor, k: int) -> torch.Tensor:
    """The same ids without sorting the vocabulary: only values >= the k-th largest VALUE (which ``torch.topk`` does define)
    can be among the first k of the stable sort; those few are stable-sorted per row."""
    kth = torch.topk(z, k, dim=-1).values[:, -1]
    out = torch.empty(z.shape[0], k, dtype=torch.int64)
    for r in range(z.shape[0]):
        cand = (z[r] >= kth[r]).nonzero().squeeze(1)                      # ascending indices
        order = torch.sort(-z[r, cand], stable=True).indices[:k]
        out[r] = cand[order]
    return out


def ref_top_ids(z: torch.Tensor, k: int, plain: bool | None = None) -> torch.Tensor:
    if plain is None:
        plain = z.numel() <= _PLAIN_SORT_MAX
    return _top_ids_plain(z, k) if plain else _top_ids_prefiltered(z, k)


def ref_logprobs(logits: torch.Tensor, token_ids: torch.Tensor | None = None, top_k: int = 0, row_chunk: int | None = None):
    """``(chosen [rows] fp64 or None, top_logprobs [rows, k] fp64, top_ids [rows, k] int64)`` of ``logits [rows, vocab]``
    in any float dtype (the stored values, exactly, are the input).  A token id outside the vocabulary gives NaN."""
    logits = logits.detach().cpu()
    rows, vocab = logits.shape
    if row_chunk is None:
        row_chunk = max(1, (1 << 23) // vocab)
    chosen = None if token_ids is None else torch.empty(rows, dtype=torch.float64)
    top_lp = torch.empty(rows, top_k, dtype=torch.float64)
    top_ids = torch.empty(rows, top_k, dtype=torch.int64)
    for r0 in range(0, rows, row_chunk):
        z = logits[r0:r0 + row_chunk].to(torch.float64)
        lsm = torch.log_softmax(z, dim=-1)
        if token_ids is not None:
            t = token_ids[r0:r0 + row_chunk].cpu().long()
            ok = (t >= 0) & (t < vocab)
            c = lsm.gather(1, torch.where(ok, t, torch.zeros_like(t)).view(-1, 1)).squeeze(1)
            chosen[r0:r0 + row_chunk] = torch.where(ok, c, torch.full_like(c, float("nan")))
        if top_k:
            ids = ref_top_ids(z, top_k)
            top_ids[r0:r0 + row_chunk] = ids
            top_lp[r0:r0 + row_chunk] = lsm.gather(1, ids)
    return chosen, top_lp, top_ids


def assert_close_logprobs(got: torch.Tensor, ref: torch.Tensor, what=""):
    """Every entry, NaN where and only where the reference has NaN."""
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (what, "NaN pattern")
    err = (got - ref).abs()[~nan]
    bound = (ATOL + RTOL * ref.abs())[~nan]
    worst = float((err - bound).max()) if err.numel() else -1.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e} over {err.numel()} entries")
    assert worst <= 0.0, (what, float(err.max()))
