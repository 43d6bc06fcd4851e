"""GPU tests of the W4A16 row-group loop (csrc/gemm_w4_v4.hip), the engine of the fused gate|up projection: all four default
instances ``wgemm4_kernel<4 | 5, 1 | 2>``, workgroups with a full and with a short last row group (both scale-pair load paths),
every k position, bias, both group sizes, ragged batches, a strided activation matrix and K shorter than the rings.

Widths come from the host plan (``ll_w4a16_v4_plan``), not from a literal CU count:
  N4r = 32 (3 cus + 4)   instance 4, tiles of four and of three row groups      N4f = 128 cus   instance 4, every tile full
  N5r = 32 (4 cus + 4)   instance 5, tiles of five and of four row groups       N5f = 160 cus   instance 5, every tile full
K is 128 (one unit, fewer than V4_AHEAD), 384 (more than V4_AHEAD, fewer than any ring) or 1280 (ten units: every ring -- 7 / 8
weight slots, 4 / 5 activation slots -- wraps).  References: ``tests/_w4_ref.py`` -- the engines' dequantisation restated exactly,
the product in float64 on the device, and a derived error bound; comparisons stay on the device.  Every test first asserts that
its launch takes the row-group loop (``w4a16_engine``), so a retuned dispatch cannot silently empty this file.

Not reached by any default launch, and not tested here: the split-K partial body (``LL_GEMM4`` bit 1) and the ``<2, *>``
instances (``LL_GEMM4_SMALL`` / ``LL_GEMM4_RGP``) -- the knobs are read once per process from the environment."""

import ctypes

import pytest
import torch

from oracle import oracle as O
from tests import _w4_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_BOUNDED = 1280
WANT_PLAN = {"N4r": (1, 4, 3, 4), "N4f": (1, 4, 4, 0), "N5r": (1, 5, 4, 4), "N5f": (1, 5, 5, 0)}  # takes, nrgt, rbase, rrem
_CACHE: dict = {}


def Q():
    import lite_llama_amd.kernels.quantization as q

    return q


def _plan(m, n, k, gs, ep=0):
    from lite_llama_amd import _lib

    out = (ctypes.c_int32 * 8)()
    assert _lib.lib().ll_w4a16_v4_plan(m, n, k, gs, ep, ctypes.cast(out, ctypes.c_void_p)) == 0
    return list(out)


@pytest.fixture(scope="module")
def widths():
    """The four widths for this device's CU count, each checked against the plan: instance, rbase and rrem as the file assumes."""
    cus = _plan(64, 37888, 3584, 128)[5]
    w = {"N4r": 32 * (3 * cus + 4), "N4f": 128 * cus, "N5r": 32 * (4 * cus + 4), "N5f": 160 * cus}
    for name, n in w.items():
        for m in (1, 64):
            for k, gs, ep in [(128, 128, 0), (384, 128, 0), (1280, 128, 0), (1280, 256, 1)]:
                takes, grid, nrgt, rbase, rrem = _plan(m, n, k, gs, ep)[:5]
                assert (takes, nrgt, rbase, rrem) == WANT_PLAN[name] and grid == cus, (name, n, m, k, gs, ep)
    yield w
    _CACHE.clear()


def _takes(m, n, k, gs, epilogue=0):
    assert Q().w4a16_engine(m, n, k, gs, epilogue) == "row_groups", (m, n, k, gs, epilogue)


def _exact(widths, name, k, gs):
    """exact_case weights of one width, packed and dequantised once (on the device) for every test that uses them."""
    key = ("exact", name, k, gs)
    if key not in _CACHE:
        n = widths[name]
        qw, sc, zr, bias = (t.to(DEV) for t in R.exact_case(n, k, gs, seed=n + k + gs))
        w16 = R.dequant16(qw, sc, zr, gs)
        plain = (R.unpack_int4(qw).float() - zr.repeat_interleave(gs, 1)) * sc.repeat_interleave(gs, 1)
        assert torch.equal(w16.float(), plain)  # the reference of the exact tests is plain integer arithmetic
        _CACHE[key] = dict(n=n, pw=Q().pack_w4a16_weights(qw), ps=Q().pack_w4a16_scales(sc, zr), w16=w16, bias=bias)
    return _CACHE[key]


def _dense(widths, name, gs):
    """dense_case at K = 1280 with 64 rows (tests take the leading M), packed and dequantised once."""
    key = ("dense", name, gs)
    if key not in _CACHE:
        n = widths[name]
        x, qw, sc, zr, bias = R.dense_case(64, n, K_BOUNDED, gs, seed=3 * n + gs)
        d = dict(n=n, cpu=(x, qw, sc, zr, bias), x=x.to(DEV), bias=bias.to(DEV))
        qd, sd, zd = qw.to(DEV), sc.to(DEV), zr.to(DEV)
        d.update(pw=Q().pack_w4a16_weights(qd), ps=Q().pack_w4a16_scales(sd, zd), w16=R.dequant16(qd, sd, zd, gs))
        _CACHE[key] = d
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------ #
# 1. exact at every k position, with scales and zeros in play
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [64, 32, 1, 17, 33])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("name,k,gs", [("N4r", 1280, 128), ("N5r", 1280, 256), ("N4f", 384, 128), ("N5f", 128, 128)])
def test_one_hot_rows_return_the_dequantised_weights_bit_for_bit(widths, name, k, gs, with_bias, m):
    """x = one-hot rows (row i picks k0 + i) over exact_case weights (power-of-two scale and integer zero per (row, group), integer
    bias): the output IS ``dequant16[:, k0 : k0 + m].T (+ bias)``, bit for bit.  M = 64 and 32 visit every k0; M = 1, 17, 33 at least
    the first and the last k of every 128-chunk.  Pins the nibble order, the k-half / k-quarter split, the four-way LDS reduction,
    the permlane32 output swizzle, every row group's scale and zero in both load paths (one 16-byte request for four groups plus 4-byte
    requests for the fifth; 4-byte requests for three), gshift, the ring wrap, the bias columns and both MT instances."""
    c = _exact(widths, name, k, gs)
    n, wt = c["n"], c["w16"].T
    _takes(m, n, k, gs)
    bias = c["bias"] if with_bias else None
    starts = R.one_hot_starts(m, k)
    bad = torch.zeros(len(starts), dtype=torch.int64, device=DEV)
    for i, k0 in enumerate(starts):
        y = Q().w4a16_matmul_prepacked(R.one_hot_rows(m, k, k0, DEV), c["pw"], c["ps"], group_size=gs, bias=bias)
        want = wt[k0:k0 + m] + bias if with_bias else wt[k0:k0 + m]  # (q - z) * s + bias is an fp16 value: the fp16 add is exact
        bad[i] = (y != want).sum()
    bad = bad.cpu()
    assert not bool(bad.any()), {starts[i]: int(b) for i, b in enumerate(bad) if b}


# ------------------------------------------------------------------------------------------------------------------------------ #
# 2. exact sums
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [64, 17])
@pytest.mark.parametrize("name,gs,with_bias", [("N4r", 128, True), ("N5r", 256, False)])
def test_small_integer_sums_are_exact(widths, name, gs, with_bias, m):
    """exact_case weights, x with 16 non-zeros per row from {+-1, +-2}, placed so that the rows together hit every 16-k block of
    every chunk (hence every chunk and every k-quarter).  Every product is a multiple of 0.25 and the magnitudes of a row's terms add
    up to less than 2048 (asserted), so every partial sum in any order is exact in fp32 and the fp32 result IS the float64 sum.
    The output must be that sum rounded once to fp16, bit for bit -- and equal to it outright wherever it is an fp16 value (a
    multiple of 0.25 is one below 512; asserted to be nearly every output)."""
    k = K_BOUNDED
    c = _exact(widths, name, k, gs)
    n = c["n"]
    _takes(m, n, k, gs)
    bias = c["bias"] if with_bias else None
    x = R.sparse_int_rows(m, k)
    cols = x.nonzero()[:, 1]
    assert {int(v) // 16 for v in cols} == set(range(k // 16))
    blk = (cols % 128) // 16  # the engine's k-quarter of a 16-k block b: (k-half b >> 2, k-step pair b & 1)
    assert {(int(v) // 128, int(b) >> 2, int(b) & 1) for v, b in zip(cols, blk)} == {(ch, kh, jp) for ch in range(k // 128) for kh in (0, 1) for jp in (0, 1)}
    x = x.to(DEV)
    y64, a64 = R.ref64(x, c["w16"], bias), R.abs_sum64(x, c["w16"], bias)
    y = Q().w4a16_matmul_prepacked(x, c["pw"], c["ps"], group_size=gs, bias=bias)
    is16 = y64.half().double() == y64
    in_range = bool(a64.max() < 2048) and bool((y64 * 4 == (y64 * 4).round()).all())
    exact_frac = float(is16.double().mean())
    assert in_range and exact_frac > 0.999, (float(a64.max()), exact_frac)
    assert torch.equal(y, y64.half())
    assert torch.equal(y.double()[is16], y64[is16])


# ------------------------------------------------------------------------------------------------------------------------------ #
# 3. dense data against float64 under the derived bound, over the whole output
# ------------------------------------------------------------------------------------------------------------------------------ #
_NAMES, _MS = ["N4r", "N4f", "N5r", "N5f"], [1, 17, 32, 33, 64]


@pytest.mark.parametrize("m", _MS)
@pytest.mark.parametrize("gs", [128, 256])
@pytest.mark.parametrize("name", _NAMES)
def test_dense_outputs_stay_inside_the_derived_bound(widths, name, gs, m):
    """dense_case at K = 1280: EVERY output within ``bound`` of the float64 product of the engines' own fp16 weights (final rounding
    + any-order fp32 summation at u = 2**-23; derived in tests/_w4_ref.py), after ``assert_bound_bites`` has shown that the bound is
    smaller than half a typical product (0.21 - 0.29 of one here).  Bias on half the cases.  Worst |err| / bound measured on the
    MI355X: 0.27 - 0.36 over the 40 cases, the same as a CPU fp32 product rounded once (DESIGN_NOTEBOOK.md 4.5; a record, not a
    threshold).  One case also keeps the suite's older bar in view: 1e-2 of the CPU oracle on a 256-row sample."""
    with_bias = (_NAMES.index(name) + _MS.index(m) + gs // 128) % 2 == 0
    d = _dense(widths, name, gs)
    n, k = d["n"], K_BOUNDED
    _takes(m, n, k, gs)
    x, bias = d["x"][:m], d["bias"] if with_bias else None
    y = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], group_size=gs, bias=bias)
    y64, a64 = R.ref64(x, d["w16"], bias), R.abs_sum64(x, d["w16"], bias)
    bnd = R.bound(y64, a64, k)
    bites = R.assert_bound_bites(x, d["w16"], bnd)
    print(f"[row_groups dense] {name} N={n} g={gs} M={m} bias={int(with_bias)}: bound/product {bites:.3f}, "
          f"worst |err|/bound {float(R.worst_ratio(y, y64, bnd)):.4f}")
    R.assert_within(y, y64, bnd, f"{name} g{gs} M={m}")
    if (name, gs, m) == ("N5r", 128, 64):
        xc, qw, sc, zr, bc = d["cpu"]
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:256].sort().values
        ref = O.w4a16_matmul(xc, qw[rows], sc[rows], zr[rows], group_size=gs, bias=bc[rows] if with_bias else None)
        torch.testing.assert_close(y[:, rows.to(DEV)].float().cpu(), ref.float(), rtol=1e-2, atol=1e-2)


# ------------------------------------------------------------------------------------------------------------------------------ #
# 4. fused swiglu epilogue
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("name", ["N4r", "N5r"])
def test_fused_swiglu_equals_swiglu_of_the_same_engines_plain_output(widths, name, m):
    """``gate_up_swiglu=True`` == ``swiglu_forward(y[:, 0::2], y[:, 1::2])`` bit for bit, y = the SAME engine's plain output on the same
    packed weights: one engine, one summation order, both GEMM outputs rounded to fp16 first, one definition of silu(g) * u
    (common.h::ll_silu_mul_f32, which pins the fp32 product before the narrowing so that every kernel rounds twice alike).  y itself
    is covered by the bounded test."""
    from lite_llama_amd.kernels import swiglu_forward

    d = _dense(widths, name, 128)
    n, k, x = d["n"], K_BOUNDED, d["x"][:m]
    _takes(m, n, k, 128, 1)
    _takes(m, n, k, 128, 0)
    y = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], group_size=128)
    fused = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], group_size=128, gate_up_swiglu=True)
    two = swiglu_forward(y[:, 0::2].contiguous(), y[:, 1::2].contiguous())
    assert fused.shape == (m, n // 2) and bool(torch.isfinite(fused).all())
    assert torch.equal(fused, two), int((fused != two).sum())


# ------------------------------------------------------------------------------------------------------------------------------ #
# 5. ragged and strided
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [1, 17, 33])
@pytest.mark.parametrize("name", ["N4r", "N5r"])
def test_ragged_batches_leave_later_rows_alone_and_a_row_stride_is_honoured(widths, name, m):
    """M = 1, 17, 33 written into a 64-row buffer pre-filled with a sentinel bit pattern: rows >= M are untouched (``row_ok``; plain
    and swiglu epilogues), rows < M are the ordinary call's.  x as the view ``big[:, :K]`` of an ``(M, K + 8)`` tensor (row stride
    K + 8, garbage behind every row): bit-identical to the contiguous call."""
    sent = 0x5A5A
    d = _dense(widths, name, 128)
    n, k, gs, x, bias = d["n"], K_BOUNDED, 128, d["x"][:m].contiguous(), d["bias"]
    _takes(m, n, k, gs, 0)
    _takes(m, n, k, gs, 1)
    y = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], group_size=gs, bias=bias)
    ys = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], group_size=gs, gate_up_swiglu=True)
    buf = torch.full((64, n), sent, dtype=torch.int16, device=DEV)
    Q()._launch_prepacked(buf.data_ptr(), x, m, n, k, d["pw"], d["ps"], bias, gs, 0, "row-group test")
    bufs = torch.full((64, n // 2), sent, dtype=torch.int16, device=DEV)
    Q()._launch_prepacked(bufs.data_ptr(), x, m, n, k, d["pw"], d["ps"], None, gs, 1, "row-group test")
    big = torch.full((m, k + 8), 777.0, dtype=torch.float16, device=DEV)
    big[:, :k] = x
    view = big[:, :k]
    assert view.stride(0) == k + 8
    y2 = Q().w4a16_matmul_prepacked(view, d["pw"], d["ps"], group_size=gs, bias=bias)
    ok = torch.stack([(buf[:m] == y.view(torch.int16)).all(), (buf[m:] == sent).all(), (bufs[:m] == ys.view(torch.int16)).all(),
                      (bufs[m:] == sent).all(), (y2.view(torch.int16) == y.view(torch.int16)).all(), torch.isfinite(y).all()])
    assert ok.tolist() == [True] * 6, ok.tolist()  # rows < M plain, rows >= M plain, the same for swiglu, strided == contiguous, finite


# ------------------------------------------------------------------------------------------------------------------------------ #
# 6. determinism and neighbours
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("name", ["N4r", "N5r"])
def test_repeated_launches_are_bit_identical_and_the_unit_loop_agrees(widths, name, m):
    """Three more launches reproduce the first bit for bit; the forced unit loop (``_tile_blocks=1``: same dequantiser, another fp32
    summation order) agrees within one fp16 ulp of the largest value, ``2**-9 max|y| + 1e-6`` -- the bar of the neighbouring engines'
    tests (test_short_stream_full_k_outputs_match_oracle_and_unit_loop)."""
    d = _dense(widths, name, 128)
    n, k, gs, x, bias = d["n"], K_BOUNDED, 128, d["x"][:m], d["bias"]
    _takes(m, n, k, gs)
    assert Q().w4a16_engine(m, n, k, gs, 1 << 8) == "unit_loop"
    kw = dict(group_size=gs, bias=bias)
    a = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], **kw)
    same = torch.stack([(Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], **kw) == a).all() for _ in range(3)])
    b = Q().w4a16_matmul_prepacked(x, d["pw"], d["ps"], _tile_blocks=1, **kw)
    scale = b.float().abs().max()
    diff = (a.float() - b.float()).abs().max()
    res = torch.stack([same.all().float(), torch.isfinite(a).all().float(), diff, scale]).tolist()
    assert res[0] == 1.0 and res[1] == 1.0
    assert res[2] <= res[3] * 2.0 ** -9 + 1e-6, res
