"""Plain float64 reference of the fused-MoE block and of one grouped GEMM, and comparisons that cannot be vacuous.

``moe_ref64``       sum_k w_k * W2 (silu(W1g x) * (W1u x)) in float64, no intermediate rounding (the routed weight is first cast
                    to the activation dtype, as the kernel and the oracle both do); scales applied per ``(group_n, group_k)``
                    grid PER MATRIX, so the refined grids of a tensor-parallel shard are expressible.
``moe_gemm_ref64``  c[slot] = (w_slot *) W[e_slot] a[slot // top_k] -- one ``ll_moe_gemm`` call.
``moe_error``       max |got - ref| over the rms of the reference ROW: a wrong row cannot hide behind large rows.
``assert_moe_close`` / ``assert_has_signal``: a bound relative to the signal, and a condition on the inputs that fails a test
                    whose reference an all-zero output would pass ``assert_close(rtol = atol = tol)`` on.

Input scaling of every test built on this file: activations ~ N(0, 1), dequantised weights ~ N(0, 1 / K) (fp8: codes ~ N(0, 1)
cast to e4m3, scales (U(0, 1) + 0.5) / sqrt(K)) -- outputs of order 1, not 20 - 100 x below the tolerance.
"""

from __future__ import annotations

import torch

from oracle import oracle as O


# ------------------------------------------------------------------------------------- #
# dequantisation
# ------------------------------------------------------------------------------------- #
def widen64(w: torch.Tensor) -> torch.Tensor:
    """Stored weight values in float64: fp16 as is, uint8 as e4m3 codes, int8 as is."""
    if w.dtype == torch.uint8:
        return w.view(torch.float8_e4m3fn).float().double()
    if w.dtype in (torch.int8, torch.float16):
        return w.double()
    raise ValueError(f"expert weights must be fp16, uint8 (e4m3) or int8, got {w.dtype}")


def dequant64(w: torch.Tensor, scale, group) -> torch.Tensor:
    """``[..., N, K]`` weights times their scale grid ``[..., ceil(N / gn), ceil(K / gk)]`` in float64.  ``group`` is
    ``(group_n, group_k)``; as in the kernels' host code, 0 along N means per row and a ``group_k`` beyond K covers K.
    A scale grid needs a ``group_k``: 0 is refused."""
    v = widen64(w)
    if scale is None:
        return v
    n, k = w.shape[-2:]
    if int(group[1]) <= 0:
        raise ValueError("a scale grid needs group_k > 0 (K, or beyond, for one scale per row)")
    gn = int(group[0]) or 1
    gk = min(int(group[1]), k)
    rows = (torch.arange(n) // gn)[:, None]
    cols = (torch.arange(k) // gk)[None, :]
    return v * scale.double()[..., rows, cols]


# ------------------------------------------------------------------------------------- #
# references
# ------------------------------------------------------------------------------------- #
def moe_gemm_ref64(a, w, flat_ids, top_k: int, *, scale=None, group=(0, 0), slot_weights=None) -> torch.Tensor:
    """``c[slot] = (w_slot *) W[e_slot] a[slot // top_k]`` in float64, ``[num_slots, N]``."""
    flat_ids = flat_ids.reshape(-1).long().cpu()
    a64 = a.cpu().double()
    out = torch.zeros(flat_ids.numel(), w.shape[1], dtype=torch.float64)
    for e in flat_ids.unique().tolist():
        slots = (flat_ids == e).nonzero().flatten()
        we = dequant64(w[e].cpu(), None if scale is None else scale[e].cpu(), group)
        out[slots] = a64[slots // top_k] @ we.T
    if slot_weights is not None:
        out = out * slot_weights.reshape(-1).cpu().double()[:, None]
    return out


def moe_ref64(x, w1, w2, topk_weights, topk_ids, *, w1_scale=None, w2_scale=None, w1_group=(0, 0), w2_group=(0, 0),
              w1_interleaved: bool = False) -> torch.Tensor:
    """The fused-MoE block in float64, ``[tokens, hidden]``; ``w1_interleaved``: rows of ``w1`` are (gate_j, up_j) pairs."""
    x, topk_ids = x.cpu(), topk_ids.cpu().long()
    t, _ = x.shape
    top_k = topk_ids.shape[1]
    inter = w1.shape[1] // 2
    wts = topk_weights.cpu().to(x.dtype).double()  # the one rounding kept: the routed weight in the activation dtype
    x64 = x.double()
    out = torch.zeros(t, w2.shape[1], dtype=torch.float64)
    for e in topk_ids.unique().tolist():
        tok, col = (topk_ids == e).nonzero(as_tuple=True)
        m1 = dequant64(w1[e].cpu(), None if w1_scale is None else w1_scale[e].cpu(), w1_group)
        m2 = dequant64(w2[e].cpu(), None if w2_scale is None else w2_scale[e].cpu(), w2_group)
        gate, up = (m1[0::2], m1[1::2]) if w1_interleaved else (m1[:inter], m1[inter:])
        g = x64[tok] @ gate.T
        h = g * torch.sigmoid(g) * (x64[tok] @ up.T)
        out.index_add_(0, tok, (h @ m2.T) * wts[tok, col][:, None])
    return out


# ------------------------------------------------------------------------------------- #
# comparisons
# ------------------------------------------------------------------------------------- #
def moe_error(got, ref64) -> float:
    """max over rows of ``max |got - ref| / rms(ref row)``."""
    ref64 = ref64.double()
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    rms = ref64.pow(2).mean(dim=-1).sqrt()
    assert bool((rms > 0).all()), "a reference row without signal cannot normalise an error"
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float(((got - ref64).abs().amax(dim=-1) / rms).max())


def assert_moe_close(got, ref64, bound: float) -> float:
    err = moe_error(got, ref64)
    assert err <= bound, f"max |got - ref64| / rms(ref row) = {err:.3e} > bound {bound:.3e}"
    return err


def zero_pass_share(ref, tol: float) -> float:
    """Share of the reference's elements on which an all-zero output satisfies ``assert_close(rtol = atol = tol)``."""
    r = ref.detach().cpu().double().abs()
    return float((r <= tol + tol * r).double().mean())


def assert_has_signal(ref, tol: float, cap: float = 0.10) -> float:
    share = zero_pass_share(ref, tol)
    assert share <= cap, f"an all-zero output passes {100 * share:.1f} % of this reference at tol {tol} (cap {100 * cap:.0f} %)"
    return share


# ------------------------------------------------------------------------------------- #
# inputs
# ------------------------------------------------------------------------------------- #
def fp8_block_experts(e, n, k, g, block=128):
    """e4m3 codes ~ N(0, 1) and ``block x block`` scales ``(U(0, 1) + 0.5) / sqrt(K)``: dequantised weights ~ N(0, 1 / K)."""
    q = torch.randn(e, n, k, generator=g).to(torch.float8_e4m3fn).view(torch.uint8)
    s = (torch.rand(e, -(-n // block), -(-k // block), generator=g) + 0.5) / k**0.5
    return q, s


def interleave_rows(w):
    """``[E, 2 I, ...]`` stacked gate|up rows (or their per-row scales) as (gate_j, up_j) pairs: row 2j = gate_j, 2j + 1 = up_j."""
    e, two_i = w.shape[0], w.shape[1]
    i = two_i // 2
    return torch.stack((w[:, :i], w[:, i:]), dim=2).reshape(e, two_i, *w.shape[2:]).contiguous()


def moe_case(fmt: str, tokens: int, experts: int, top_k: int, hidden: int, inter: int, seed: int):
    """Seeded inputs of one block: ``(x, w1, w2, wts, ids, kw)`` with ``kw`` the quantisation keywords both
    ``kernels.fused_moe`` and ``oracle.fused_moe`` take.  ``fmt``: f16 | fp8_block | int8_channel | fp8_channel.
    Every token picks ``top_k`` distinct experts."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tokens, hidden, generator=g).half()
    ids = torch.stack([torch.randperm(experts, generator=g)[:top_k] for _ in range(tokens)])
    wts = torch.softmax(torch.randn(tokens, top_k, generator=g), dim=-1).half()
    if fmt == "fp8_block":
        w1, s1 = fp8_block_experts(experts, 2 * inter, hidden, g)
        w2, s2 = fp8_block_experts(experts, hidden, inter, g)
        return x, w1, w2, wts, ids, dict(w1_scale=s1, w2_scale=s2, group_n=128, group_k=128)
    w1 = torch.randn(experts, 2 * inter, hidden, generator=g) / hidden**0.5
    w2 = torch.randn(experts, hidden, inter, generator=g) / inter**0.5
    if fmt == "f16":
        return x, w1.half(), w2.half(), wts, ids, {}
    quant = {"int8_channel": O.quantize_int8_per_channel, "fp8_channel": O.quantize_fp8_per_channel}[fmt]
    (q1, s1), (q2, s2) = quant(w1), quant(w2)
    return x, q1, q2, wts, ids, dict(w1_scale=s1, w2_scale=s2, group_n=1, group_k=hidden)


def groups_of(kw) -> dict:
    """``moe_ref64`` keywords for the ``fused_moe`` keywords ``kw`` (one grid for both matrices unless given per matrix)."""
    if "w1_scale" not in kw:
        return {}
    g = (kw.get("group_n", 0), kw.get("group_k", 0))
    return dict(w1_scale=kw["w1_scale"], w2_scale=kw["w2_scale"], w1_group=kw.get("w1_group") or g,
                w2_group=kw.get("w2_group") or g)
