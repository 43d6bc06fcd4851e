"""TEST INFRASTRUCTURE ONLY -- the pre-packed W4A16 decode engines' own arithmetic in exact form, a float64 reference of the
product, and the largest error a correct engine can make against it.  Plain torch, device-agnostic (the GPU tests run it on the
device, ``tests/test_w4_ref_cpu.py`` checks it on the CPU); nothing here calls a kernel of the project.

What the engines compute (csrc/gemm_w4_common.h::v3_dequant, csrc/gemm_w4_v3.hip::w4a16_pack_scales_kernel):

* load time: per (row, group) the fp16 pair ``hs = fp16(s)`` and ``hz = fp16(fp32(-z * s))`` -- the fp32 product of the fp32 zero and
  the fp32 scale (NOT of the rounded ``hs``), one rounding to fp32, one to fp16, both to nearest even;
* run time: the nibble ``q`` widened exactly to fp16 (1024 + q, minus 1024), then ONE fp16 fma ``w = fma(q, hs, hz)``;
* ``y[m, n] = fp16(sum_k x[m, k] * w[n, k] (+ bias[n]))``: exact fp16 x fp16 products, fp32 accumulation in an order the engine
  chooses, the bias added in fp32, one rounding to fp16 (split-K planes: the fp32 sums themselves, no bias).
"""

from __future__ import annotations

import torch

U_ACC = 2.0 ** -23  # unit roundoff allowed for one fp32 accumulation step: a TRUNCATING add (round to nearest would be 2**-24)


def unpack_int4(qweight: torch.Tensor) -> torch.Tensor:
    """``[N, K/8] int32`` -> ``[N, K] int32`` nibbles, LSB first along K (the oracle's ``unpack_int4``, on any device)."""
    shifts = torch.arange(8, dtype=torch.int32, device=qweight.device) * 4
    return ((qweight.unsqueeze(-1) >> shifts) & 0xF).reshape(qweight.shape[0], -1)


def scale_pair16(scales: torch.Tensor, zeros: torch.Tensor):
    """``ll_w4a16_pack_scales`` restated: ``(fp16(s), fp16(fp32(-z * s)))`` per (row, group), as fp16 tensors ``[N, K/g]``."""
    s32, z32 = scales.float(), zeros.float()
    return s32.half(), (-z32 * s32).half()


def dequant16(qweight: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, group_size: int) -> torch.Tensor:
    """The ``[N, K]`` fp16 weights exactly as the decode engines define them: ``fp16(q * hs + hz)`` with one rounding.  The fma is
    evaluated in float64, where it is exact (a 4-bit by 11-bit product plus an 11-bit addend that is a multiple of the scale's
    last place: at most 17 significant bits), and rounded once to fp16 (the value also fits fp32, so the narrowing through
    fp32 that a float64 -> fp16 conversion may take rounds once)."""
    hs, hz = scale_pair16(scales, zeros)
    q = unpack_int4(qweight).double()
    s = hs.double().repeat_interleave(group_size, dim=1)
    z = hz.double().repeat_interleave(group_size, dim=1)
    return (q * s + z).float().half()


def ref64(x: torch.Tensor, w16: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``x @ w16.T (+ bias)`` in float64."""
    y = x.double() @ w16.double().T
    return y if bias is None else y + bias.double()


def abs_sum64(x: torch.Tensor, w16: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``sum_k |x[m, k] * w16[n, k]| (+ |bias[n]|)`` in float64: the sum of the magnitudes of the terms a kernel adds up."""
    a = x.double().abs() @ w16.double().abs().T
    return a if bias is None else a + bias.double().abs()


def half_ulp16(y64: torch.Tensor) -> torch.Tensor:
    """Half the fp16 unit in the last place at ``|y64|``: ``2**(floor(log2 |y|) - 11)``, never below the subnormal spacing's half
    ``2**-25`` (every ``|y| < 2**-14``, zero included)."""
    _, e = torch.frexp(y64.double().abs())  # |y| = f * 2**e, f in [0.5, 1)  ->  floor(log2 |y|) = e - 1
    e = torch.where(y64 == 0, torch.full_like(e, -100), e)
    return torch.ldexp(torch.ones_like(y64, dtype=torch.float64), (e - 12).clamp(min=-25))


def bound(y64: torch.Tensor, abs64: torch.Tensor, k: int, planes: bool = False) -> torch.Tensor:
    """The largest ``|got - y64|`` a correct engine can produce, elementwise.  A derived number, not a measured one.

    A correct engine holds the ``k`` products ``x * w16`` exactly (11 x 11 significant bits fit fp32's 24), adds them and the bias
    -- ``n = k + 1`` terms ``t_i`` -- in fp32 in SOME order, and rounds the fp32 result ``s`` once to fp16.

    Summation.  Every fp32 addition returns ``(a + b)(1 + d)`` with ``|d| <= u``.  Whatever the order (sequential, pairwise, four
    k-quarters that meet at the end, split-K), a term passes through at most ``n - 1`` additions, so
    ``|s - sum t_i| <= ((1 + u)**(n - 1) - 1) * sum |t_i| <= (n - 1) u / (1 - (n - 1) u) * sum |t_i|`` (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2), and ``k u / (1 - k u) <= (k + 1) u`` as long as ``k (k + 1) u <= 1``, i.e. for every
    ``k <= 2895`` at ``u = 2**-23``.  ``u = 2**-23`` and not ``2**-24``: the matrix cores may align the products of one instruction to
    the largest exponent and truncate instead of rounding to nearest; a truncated add loses less than one unit in the last place of
    its result, ``<= 2**-23`` relative.  Hence the term ``(k + 1) * 2**-23 * abs64`` with ``abs64 = sum |t_i|``.

    Final rounding.  ``|fp16(s) - s|`` is at most half an fp16 ulp -- taken at ``y64``, with the subnormal spacing as the floor;
    dropped for fp32 planes (``planes=True``), which are not rounded.  One caveat, stated rather than paid for: where ``y64``
    lies just below a power of two and ``s`` has crossed it by more than one ulp of ``y64``'s binade, ``fp16(s)`` rounds on the
    coarser grid above and the strict worst case is the summation term plus half an ulp of THAT binade.  Crossing by that much
    takes a summation error near its worst case (every one of the k roundings lost in the same direction); the bound is kept
    in the tighter form, which can only make the tests stricter, never hide a failure."""
    assert 0 < k <= 2895
    b = (k + 1) * U_ACC * abs64.double()
    return b if planes else b + half_ulp16(y64)


def worst_ratio(got: torch.Tensor, y64: torch.Tensor, bnd: torch.Tensor) -> torch.Tensor:
    """``max |got - y64| / bnd`` as a 0-d tensor on the inputs' device (the record for the notebook; <= 1 passes)."""
    return ((got.double() - y64).abs() / bnd).max()


def within_flags(got: torch.Tensor, y64: torch.Tensor, bnd: torch.Tensor) -> torch.Tensor:
    """Device-side verdict, no synchronisation: ``[all finite, worst |err| / bound]`` as a float64 tensor of two."""
    return torch.stack([torch.isfinite(got).all().double(), worst_ratio(torch.nan_to_num(got.double(), nan=1e300, posinf=1e300, neginf=-1e300),
                                                                        y64, bnd)])


def assert_within(got: torch.Tensor, y64: torch.Tensor, bnd: torch.Tensor, what: str = "") -> float:
    """Every element of ``got`` is finite and within ``bnd`` of ``y64``; on failure the worst element with its row and column.
    Returns the worst ``|err| / bound`` (one synchronisation)."""
    assert got.shape == y64.shape == bnd.shape, (got.shape, y64.shape, bnd.shape)
    finite, worst = within_flags(got, y64, bnd).tolist()
    if finite == 1.0 and worst <= 1.0:
        return worst
    g = got.double()
    if finite != 1.0:
        idx = int((~torch.isfinite(g)).flatten().nonzero()[0])
        r, c = divmod(idx, got.shape[1])
        raise AssertionError(f"{what}: non-finite output {g[r, c].item()} at row {r}, column {c}")
    ratio = (g - y64).abs() / bnd
    idx = int(ratio.argmax())
    r, c = divmod(idx, got.shape[1])
    bad = int((ratio > 1).sum())
    raise AssertionError(f"{what}: {bad} of {got.numel()} elements outside the bound; worst at row {r}, column {c}: got {g[r, c].item()!r}, "
                         f"float64 {y64[r, c].item()!r}, |err| {abs(g[r, c].item() - y64[r, c].item()):.3e} > bound {bnd[r, c].item():.3e} "
                         f"(ratio {ratio[r, c].item():.2f})")


def product_rms(x: torch.Tensor, w16: torch.Tensor) -> float:
    """Root mean square of a single product ``x[m, k] * w16[n, k]`` over all (m, n, k)."""
    return float(((x.double() ** 2).mean(0) * (w16.double() ** 2).mean(0)).mean().sqrt())


def assert_bound_bites(x: torch.Tensor, w16: torch.Tensor, bnd: torch.Tensor) -> float:
    """The condition that keeps the bound from hiding a failure: the largest bound is at most half the rms of ONE product, so an
    output that lost, doubled or misplaced a single typical term lands outside it.  The ratio grows like ``K**2 * 2**-23`` (bound
    ~ K * 2**-23 * K * mean|product|): ~0.16 at K = 1280 with ``dense_case``, past 1/2 near K = 2300 -- the bounded tests stay at
    K <= 1280.  Returns the ratio."""
    ratio = float(bnd.max()) / product_rms(x, w16)
    assert ratio <= 0.5, f"largest bound / rms of one product = {ratio:.3f} > 0.5: the bound could hide a dropped term"
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------ #
# generators (CPU tensors; a fixed seed per case)
# ------------------------------------------------------------------------------------------------------------------------------ #
def _words(n: int, k: int, g: torch.Generator) -> torch.Tensor:
    return torch.randint(-(2 ** 31), 2 ** 31 - 1, (n, k // 8), dtype=torch.int64, generator=g).to(torch.int32)


def exact_case(n: int, k: int, group_size: int, seed: int):
    """``(qweight, scales, zeros, bias)`` on which the affine map is exact: random words, per (row, group) a scale from
    {0.25, 0.5, 1, 2, 4} and an integer zero 0..15, an integer-valued fp16 bias in -8..8.  ``-z * s`` and every
    ``(q - z) * s + bias`` are then fp16 values, and ``dequant16`` equals ``(q - z) * s`` in plain integer arithmetic."""
    g = torch.Generator().manual_seed(seed)
    qw = _words(n, k, g)
    groups = k // group_size
    sc = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[torch.randint(0, 5, (n, groups), generator=g)]
    zr = torch.randint(0, 16, (n, groups), generator=g).float()
    bias = torch.randint(-8, 9, (n,), generator=g).half()
    return qw, sc, zr, bias


def dense_case(m: int, n: int, k: int, group_size: int, seed: int):
    """``(x, qweight, scales, zeros, bias)``: the suite's usual draw -- ``x ~ 0.5 N(0, 1)`` fp16, random words, scales uniform in
    [0.005, 0.015], integer zeros 0..15, bias ``~ 0.1 N(0, 1)`` fp16."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(m, k, generator=g) * 0.5).half()
    qw = _words(n, k, g)
    sc = torch.rand(n, k // group_size, generator=g) * 0.01 + 0.005
    zr = torch.randint(0, 16, (n, k // group_size), generator=g).float()
    bias = (torch.randn(n, generator=g) * 0.1).half()
    return x, qw, sc, zr, bias


def one_hot_rows(m: int, k: int, k0: int, device=None) -> torch.Tensor:
    """fp16 ``[m, k]``: row ``i`` is the unit vector of position ``k0 + i``."""
    x = torch.zeros(m, k, dtype=torch.float16, device=device)
    i = torch.arange(m, device=device)
    x[i, k0 + i] = 1.0
    return x


def one_hot_starts(m: int, k: int):
    """The ``k0`` values of a one-hot sweep with ``m`` rows: every k position for m = 64 and m = 32; otherwise at least the first
    and the last k of every 128-chunk (row 0 on the first, row m - 1 on the last)."""
    if m in (32, 64):
        return list(range(0, k, m))
    return sorted({c for c0 in range(0, k, 128) for c in (c0, c0 + 128 - m)})


def sparse_int_rows(m: int, k: int, nnz: int = 16) -> torch.Tensor:
    """fp16 ``[m, k]`` with ``nnz`` non-zeros per row from {+-1, +-2}: non-zero ``j`` of row ``i`` falls into the 16-k block
    ``(i * nnz + j) mod (k / 16)`` -- consecutive blocks, so a row's positions are distinct and ``k / 16`` consecutive non-zeros
    visit every block of every 128-chunk (a block fixes the engines' k-half, lane half and k-step pair)."""
    assert k % 16 == 0 and nnz <= k // 16
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0])
    x = torch.zeros(m, k, dtype=torch.float16)
    for i in range(m):
        for j in range(nnz):
            t = i * nnz + j
            blk, lap = t % (k // 16), t // (k // 16)
            x[i, blk * 16 + (i * 7 + j * 5 + lap) % 16] = vals[(i + 3 * j + lap) % 4]
    return x
