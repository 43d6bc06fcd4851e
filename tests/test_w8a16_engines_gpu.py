"""GPU tests of the three engines behind ``w8a16_matmul`` (``ll_w8a16_matmul``, csrc/gemm_wq.hip): the skinny split-K engine
``dense8_kernel<D8_FP8 | D8_I8, 1 | 2>`` + ``dense8_finish`` (csrc/gemm_w8_skinny.hip; M <= 64, N % 4 == 0, K % 128 == 0), the M-tiled
engine ``w8_mtiled_kernel<1 | 2, WH>`` (csrc/gemm_w8_prefill.hip; M > 64, N % 32 == 0, K % 64 == 0) and the generic engine
``wgemm_kernel<FMT_FP8 | FMT_I8, 1 | 2, 1, 2>`` (everything else) -- with scales in play at every k position, at checkpoint
magnitudes (fp16-subnormal weights, fp16-subnormal int8 scales), every split structure of the skinny engine, partial last scale
rows and columns, ragged N / M, row-strided operands and transposed scales.

Shapes (``tests/_w8_ref.py::SHAPES``; chunks of 128 k -> split-K planes from ``d8_splits``):
  S1 132 x 128   skinny   1 -> 1              single chunk (the refetch), ragged second tile of 4 rows
  S2 256 x 640   skinny   5 -> 2 (3 + 2)      short last split; group_k = 256 leaves a partial last scale column
  S3 388 x 1152  skinny   9 -> 3              three full tiles + 4 rows; group_n = 64 / 128 leave a partial last scale row
  S4 128 x 2560  skinny   20 -> 10            second round of dense8_finish with a tail of two planes
  G1 130 x 384   generic  (N % 4 != 0)        G2 256 x 336  generic (K % 128 != 0), partial last k-group at group_k = 128
  T1 160 x 1152  M-tiled at M = 65, 129, 200 (ragged N tile; one row / one tile + one row / partial second M tile)
  T2 130 x 384   generic at M = 100 (more than one M block)
Formats: fp8 with (group_n, group_k) = (128, 128) and (64, 256); int8 per channel (1, K), group-wise (1, 128) and (1, 256).

References: ``tests/_w8_ref.py`` -- the engines' dequantisation restated exactly, the product in float64 on the device, the derived
error bound of ``tests/_w4_ref.py``; comparisons stay on the device, a handful of synchronisations per test.  Every test first asserts
that its launch takes the engine the table names (``w8a16_engine``, built from the launch functions' own predicates) and, on the
skinny engine, leaves the plane count the table names (derived from ``ll_dense8_partial_words``): a retuned dispatch cannot silently empty this file.

Not reached by any default launch, and not tested here: ``LL_DENSE8_OFF``, ``LL_W8_NO_MTILED``, ``LL_P8_WMH`` and
``LL_D8_NT_MIN_MB`` -- the knobs are read once per process from the environment."""

import pytest
import torch

from oracle import oracle as O
from tests import _w8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5A5A
_CACHE: dict = {}


def Q():
    import lite_llama_amd.kernels.quantization as q

    return q


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def _lib():
    from lite_llama_amd import _lib as L

    return L.lib()


def _route(tag, m, fmt, gk, x_stride=None, w_stride=None, want=None):
    """Assert, before any launch, the engine of this call and (skinny) its plane count."""
    n, k = R.SHAPES[tag]
    want = want or R.want_engine(tag, m)
    got = Q().w8a16_engine(m, n, k, fmt, gk, x_stride, w_stride)
    assert got == want, (tag, m, fmt, gk, x_stride, w_stride, got, want)
    if want == "skinny":
        assert R.skinny_planes(_lib().ll_dense8_partial_words(1, n, k), n, k) == R.SKINNY_PLANES[tag], tag
    return want


def _case(kind, tag, fmt, gn, gk):
    """One weight set of a shape on the device, built and dequantised once: ``kind`` = "mild" / "subnormal" (checkpoint_case8; x with
    the shape's largest batch) or "all" / "sum" (exact_case8)."""
    key = (kind, tag, fmt, gn, gk)
    if key not in _CACHE:
        n, k = R.SHAPES[tag]
        seed = R.case_seed(tag, fmt, gn, gk)
        if kind in ("mild", "subnormal"):
            rows = {"T1": 200, "T2": 100}.get(tag, 64)
            x, q, sc, bias = R.checkpoint_case8(fmt, rows, n, k, gn, gk, seed, spread=kind)
            if kind == "subnormal" and fmt == "int8":
                assert not bool(R.supported_scale(fmt, sc).all())  # the draw does hold fp16-subnormal scales
        else:
            q, sc, bias = R.exact_case8(fmt, n, k, gn, gk, seed, codes=kind)
            x = None
        d = dict(n=n, k=k, cpu=(x, q, sc, bias), q=q.to(DEV), sc=sc.to(DEV), bias=bias.to(DEV), x=None if x is None else x.to(DEV))
        d["w16"] = R.dequant16(fmt, d["q"], d["sc"], gn, gk)
        if x is None:
            assert torch.equal(d["w16"].double(), R.true64(fmt, d["q"], d["sc"], gn, gk))  # the exact tests' reference is plain arithmetic
        _CACHE[key] = d
    return _CACHE[key]


def _mm(x, c, gn, gk, bias=None):
    return Q().w8a16_matmul(x, c["q"], c["sc"], group_n=gn, group_k=gk, bias=bias)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _differ(y, want):
    """Elementwise: the fp16 bit patterns differ -- except +0 against -0: a weight of -0 (the fp8 code 0x80, a negative product
    rounded to zero) added to an accumulator that starts at +0 gives +0."""
    return (_bits(y) != _bits(want)) & ~((y == 0) & (want == 0))


def _shape_formats(tags):
    return [(t, f, gn, gk) for t in tags for f, gn, gk in R.formats_for(t)]


# ------------------------------------------------------------------------------------------------------------------------------ #
# 1. one-hot rows: the dequantised weights bit for bit, at every k position, with scales in play
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("kind", ["mild", "subnormal", "all", "all+bias"])
@pytest.mark.parametrize("tag,fmt,gn,gk", _shape_formats(["S1", "S2", "S3", "G1", "G2", "T1"]))
def test_one_hot_rows_return_the_dequantised_weights_bit_for_bit(tag, fmt, gn, gk, kind):
    """x = one-hot rows (row i picks k = (k0 + i) mod K): a single non-zero term makes the fp32 sum exact, so the output IS
    ``dequant16[:, k].T`` bit for bit -- over checkpoint-scale weights (arbitrary scales; fp16-subnormal weights), over the
    wide-spread variant (fp16-subnormal int8 scales: pins ``fp16(s)`` and the kept denormals), and over exact_case8 weights (all 256
    fp8 codes, the full int8 range), there also with a bias: the fp32 sum of one weight and an integer bias is exact, so the output is
    that sum rounded once.  M = 64 and 32 (M-tiled: 65 and 200) visit every k0; M = 1, 17, 33 the first and the last k of every
    chunk.  Pins, per engine: the scale row and column at every k-half, the partial last scale row and column, both scale strides,
    the LDS layout and swizzle, the split boundaries and the finish pass."""
    with_bias = kind.endswith("+bias")
    c = _case(kind.split("+")[0], tag, fmt, gn, gk)
    n, k, wt = c["n"], c["k"], c["w16"].T
    bias = c["bias"] if with_bias else None
    ms = (65, 200) if tag == "T1" else (64, 32, 1, 17, 33)
    for m in ms:
        _route(tag, m, fmt, gk)
    bad, where = [], []
    for m in ms:
        idx = torch.arange(m, device=DEV)
        for k0 in R.one_hot_starts8(m, k):
            y = _mm(R.one_hot_wrapped(m, k, k0, DEV), c, gn, gk, bias)
            want = wt[(k0 + idx) % k]
            if with_bias:
                want = (want.double() + bias.double()).float().half()  # exact in float64 and in fp32: one rounding, like the engines
            bad.append(_differ(y, want).sum())
            where.append((m, k0))
    bad = torch.stack(bad).cpu()
    assert not bool(bad.any()), {where[i]: int(b) for i, b in enumerate(bad) if b}


# ------------------------------------------------------------------------------------------------------------------------------ #
# 2. exact sums
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("tag,fmt,gn,gk", _shape_formats(["S2", "S3", "S4", "G2", "T1"]))
def test_small_integer_sums_are_exact(tag, fmt, gn, gk):
    """exact_case8 weights ("sum" draw: fp8 codes with 1 <= |value| <= 448), x with 16 non-zeros per row from {+-1, +-2} that
    together hit every 16-k block.  Every term is a multiple of the quantum (2**-5 fp8, 2**-2 int8) and the magnitudes of a row's terms
    add up to less than 2**24 quanta (both asserted), so every partial sum in any order is exact in fp32 and the fp32 result IS the
    float64 sum: the output must be that sum rounded once to fp16, bit for bit, and equal to it outright wherever it is an fp16
    value.  S4 is the only check of more than eight planes: a dropped or doubled plane fails.  M = 64 and 17 (T1: 129); bias on
    half the cases."""
    c = _case("sum", tag, fmt, gn, gk)
    n, k = c["n"], c["k"]
    quantum = R.sum_quantum(fmt)
    ms = (129,) if tag == "T1" else (64, 17)
    for m in ms:
        _route(tag, m, fmt, gk)
    res = [((c["w16"].double() / quantum) % 1 == 0).all().double()]  # every weight, hence every term of an integer activation
    for i, m in enumerate(ms):
        bias = c["bias"] if (i + sorted(R.SHAPES).index(tag) + gn + gk // 128) % 2 == 0 else None
        x = R.sparse_int_rows(m, k)
        assert {int(v) // 16 for v in x.nonzero()[:, 1]} == set(range(k // 16))
        assert set(x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        x = x.to(DEV)
        y64, a64 = R.ref64(x, c["w16"], bias), R.abs_sum64(x, c["w16"], bias)
        y = _mm(x, c, gn, gk, bias)
        is16 = y64.float().half().double() == y64
        res += [a64.max() / quantum, (~_differ(y, y64.float().half())).all().double(),
                (torch.where(is16, y.double(), y64) == y64).all().double(), is16.double().mean()]
    res = torch.stack(res).tolist()
    assert res[0] == 1.0
    for i, m in enumerate(ms):
        amax, same, same64, frac16 = res[1 + 4 * i:5 + 4 * i]
        assert amax < 2 ** 24, (m, amax)
        assert same == 1.0 and same64 == 1.0, (tag, fmt, m, same, same64, frac16)


# ------------------------------------------------------------------------------------------------------------------------------ #
# 3. checkpoint-scale data against float64 under the derived bound, over the whole output
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("tag,fmt,gn,gk,ms", R.bounded_cases())
def test_checkpoint_scale_outputs_stay_inside_the_derived_bound(tag, fmt, gn, gk, ms):
    """checkpoint_case8 (block scales ~1e-4, weights ~0.02, mild row spread): EVERY output within ``bound`` of the float64 product of
    the engines' own fp16 weights (final rounding + any-order fp32 summation at u = 2**-23; derived in tests/_w4_ref.py), after
    ``assert_bound_bites`` has shown the bound to be at most half the rms of one product (K <= 1152).  Bias on every other batch.
    Worst |err| / bound measured on the MI355X: DESIGN_NOTEBOOK.md 8.19 (records, not thresholds).  One case per format also keeps the
    suite's older bar in view: 1e-2 of the CPU oracle."""
    c = _case("mild", tag, fmt, gn, gk)
    n, k = c["n"], c["k"]
    for m in ms:
        _route(tag, m, fmt, gk)
    for i, m in enumerate(ms):
        bias = c["bias"] if i % 2 == 0 else None
        x = c["x"][:m]
        y = _mm(x, c, gn, gk, bias)
        y64, a64 = R.ref64(x, c["w16"], bias), R.abs_sum64(x, c["w16"], bias)
        bnd = R.bound(y64, a64, k)
        bites = R.assert_bound_bites(x, c["w16"], bnd)
        print(f"[w8a16 bounded] {tag} {R.want_engine(tag, m)} {fmt} g=({gn},{gk}) M={m} bias={int(bias is not None)}: bound/product {bites:.3f}, "
              f"worst |err|/bound {float(R.worst_ratio(torch.nan_to_num(y.double(), nan=1e300), y64, bnd)):.4f}")
        R.assert_within(y, y64, bnd, f"{tag} {fmt} g=({gn},{gk}) M={m}")
    if (tag, fmt, gn, gk) in {("S3", "fp8", 128, 128), ("S3", "int8", 1, 1152), ("G1", "fp8", 128, 128), ("G1", "int8", 1, 384),
                              ("T1", "fp8", 128, 128), ("T1", "int8", 1, 1152)}:  # the older bar, once per format and engine
        xc, q, sc, bc = c["cpu"]
        m_bar = max(ms)  # the largest batch of the shape, with bias
        got = _mm(c["x"][:m_bar], c, gn, gk, c["bias"])
        ref = O.w8a16_matmul(xc[:m_bar], q, sc, group_n=gn, group_k=gk, bias=bc)
        torch.testing.assert_close(got.float().cpu(), ref.float(), rtol=1e-2, atol=1e-2)


# ------------------------------------------------------------------------------------------------------------------------------ #
# 4. partial mode
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("tag,fmt,gn,gk", R.PARTIAL_CASES)
def test_partial_planes_sum_to_the_product(tag, fmt, gn, gk, m):
    """``dense_matmul_partials(..., max_splits=12)``: the fp32 planes, summed in float64, within the bound without its rounding term
    (``planes=True``; a term passes through no more additions than in the finished form) of the float64 product; at most 12 planes.
    group_k = 64 and 192 (partial mode only) give the two k-halves of a chunk different scales."""
    c = _case("mild", tag, fmt, gn, gk)
    n, k = c["n"], c["k"]
    x = c["x"][:m]
    wf = 1 if fmt == "fp8" else 2
    count, form = _lib().ll_dense_partials_count(m, n, k, wf, 12), _lib().ll_dense_partials_form(m, n, k, wf, 12)
    assert 1 <= count <= 12 and form in (1, 2)
    if form == 2:
        assert count == R.streaming_planes(n, k, 12)
    ps = Q().dense_matmul_partials(x, c["q"], c["sc"], group_n=gn, group_k=gk, max_splits=12)
    assert ps is not None and ps.parts.shape == (count, m, n) and ps.parts.dtype == torch.float32
    y64, a64 = R.ref64(x, c["w16"]), R.abs_sum64(x, c["w16"])
    bnd = R.bound(y64, a64, k, planes=True)
    worst = R.assert_within(ps.parts.double().sum(0), y64, bnd, f"planes {tag} {fmt} M={m}")
    print(f"[w8a16 planes] {tag} {fmt} g=({gn},{gk}) M={m}: {count} planes from the {'short-stream form' if form == 1 else 'streaming kernel'}, "
          f"worst |err|/bound {worst:.4f}")


@pytest.mark.parametrize("tag,fmt,gn,gk", [c for c in R.PARTIAL_CASES if c[3] in (64, 192)])
def test_partial_planes_of_one_hot_rows_are_the_weights_with_a_scale_per_k_half(tag, fmt, gn, gk):
    """One-hot rows through partial mode, M = 64 at every k0: one plane holds the weight, the others zero, so the float64 sum of the
    planes IS ``dequant16[:, k].T`` -- with scale groups of 64 and 192 k, where the group index of the chunk's second k-half
    (``kbase / group_k``) differs from that of its first.  The only place a wrong k-half scale index of ``dense8_kernel`` can show:
    the finished entry takes group_k % 128 == 0 or K only."""
    c = _case("mild", tag, fmt, gn, gk)
    n, k, wt = c["n"], c["k"], c["w16"].T
    wf = 1 if fmt == "fp8" else 2
    # this test is about dense8_kernel: the call must be the streaming kernel's (not the short-stream form's), with its plane count
    assert _lib().ll_dense_partials_form(64, n, k, wf, 12) == 2
    assert _lib().ll_dense_partials_count(64, n, k, wf, 12) == R.streaming_planes(n, k, 12)
    idx = torch.arange(64, device=DEV)
    starts = R.one_hot_starts8(64, k)
    bad = []
    for k0 in starts:
        ps = Q().dense_matmul_partials(R.one_hot_wrapped(64, k, k0, DEV), c["q"], c["sc"], group_n=gn, group_k=gk, max_splits=12)
        assert ps is not None
        bad.append((ps.parts.double().sum(0) != wt[(k0 + idx) % k].double()).sum())
    bad = torch.stack(bad).cpu()
    assert not bool(bad.any()), {starts[i]: int(b) for i, b in enumerate(bad) if b}


# ------------------------------------------------------------------------------------------------------------------------------ #
# 5. ragged batches and strides, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------ #
def _abi_call(out_ptr, x, q, sc, bias, m, n, k, gn, gk, fmt):
    from lite_llama_amd import _lib as L

    ws, cnt = L.gemm_workspace(x.device, m, n, k)
    L.check(L.lib().ll_w8a16_matmul(out_ptr, x.data_ptr(), q.data_ptr(), sc.data_ptr(), L.ptr(bias), m, n, k, gn, min(gk, k),
                                    L.LL_W_FP8E4M3 if fmt == "fp8" else L.LL_W_INT8, x.stride(0), q.stride(0), sc.stride(0), sc.stride(1),
                                    ws.data_ptr(), cnt.data_ptr(), L.stream_ptr()), "ll_w8a16_matmul (test)")


@pytest.mark.parametrize("m", [1, 17, 33])
@pytest.mark.parametrize("tag,fmt,gn,gk", [("S3", "fp8", 128, 128), ("S3", "int8", 1, 128), ("G1", "fp8", 128, 128), ("G1", "int8", 1, 384)])
def test_ragged_batches_leave_later_rows_alone(tag, fmt, gn, gk, m):
    """M = 1, 17, 33 written through the C ABI into a 64-row buffer pre-filled with a sentinel bit pattern: rows < M are the
    wrapper's output bit for bit, rows >= M still hold the sentinel (33: the MT = 2 instances below a full second tile)."""
    c = _case("mild", tag, fmt, gn, gk)
    n, k = c["n"], c["k"]
    _route(tag, m, fmt, gk)
    x = c["x"][:m].contiguous()
    y = _mm(x, c, gn, gk, c["bias"])
    buf = torch.full((64, n), SENT, dtype=torch.int16, device=DEV)
    _abi_call(buf.data_ptr(), x, c["q"], c["sc"], c["bias"], m, n, k, gn, gk, fmt)
    ok = torch.stack([(buf[:m] == _bits(y)).all(), (buf[m:] == SENT).all(), torch.isfinite(y).all()])
    assert ok.tolist() == [True] * 3, ok.tolist()


@pytest.mark.parametrize("tag,m,fmt,gn,gk", [(t, m, f, gn, gk) for t, m in (("S3", 33), ("G1", 17), ("T1", 129))
                                              for f, gn, gk in (("fp8", 128, 128), ("fp8", 64, 256), ("int8", 1, 128))])
def test_row_strided_operands_and_transposed_scales_change_nothing(tag, m, fmt, gn, gk):
    """Each bit-identical to the contiguous call, on the same engine (route asserted with the strides): x as ``big[:, :K]`` of an
    ``(M, K + 8)`` tensor filled with 777; qweight as ``wide[:, :K]`` of an ``(N, K + 16)`` tensor filled with garbage; scales as
    the transpose of a contiguous ``[kb, nb]`` tensor -- and all three at once."""
    c = _case("mild", tag, fmt, gn, gk)
    n, k = c["n"], c["k"]
    eng = _route(tag, m, fmt, gk)
    _route(tag, m, fmt, gk, x_stride=k + 8, want=eng)
    _route(tag, m, fmt, gk, w_stride=k + 16, want=eng)
    _route(tag, m, fmt, gk, x_stride=k + 8, w_stride=k + 16, want=eng)
    x, bias = c["x"][:m].contiguous(), c["bias"]
    y = _mm(x, c, gn, gk, bias)
    big = torch.full((m, k + 8), 777.0, dtype=torch.float16, device=DEV)
    big[:, :k] = x
    xv = big[:, :k]
    wide = torch.full((n, k + 16), 0x7B, dtype=torch.uint8, device=DEV).view(c["q"].dtype)
    wide[:, :k] = c["q"]
    qv = wide[:, :k]
    st = c["sc"].T.contiguous().T
    assert xv.stride(0) == k + 8 and qv.stride(0) == k + 16 and st.stride() == (1, c["sc"].shape[0]) and torch.equal(st, c["sc"])
    kw = dict(group_n=gn, group_k=gk, bias=bias)
    got = [Q().w8a16_matmul(xv, c["q"], c["sc"], **kw), Q().w8a16_matmul(x, qv, c["sc"], **kw), Q().w8a16_matmul(x, c["q"], st, **kw),
           Q().w8a16_matmul(xv, qv, st, **kw)]
    ok = torch.stack([(_bits(g) == _bits(y)).all() for g in got] + [torch.isfinite(y).all()])
    assert ok.tolist() == [True] * 5, ok.tolist()  # strided x, strided qweight, transposed scales, all three, finite


# ------------------------------------------------------------------------------------------------------------------------------ #
# 6. determinism and neighbours
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("tag,m,fmt,gn,gk", [("S3", 64, "fp8", 128, 128), ("S3", 17, "int8", 1, 128), ("S4", 64, "fp8", 64, 256), ("S4", 33, "int8", 1, 2560),
                                              ("G1", 64, "fp8", 128, 128), ("G1", 17, "int8", 1, 384), ("T1", 129, "fp8", 128, 128), ("T1", 200, "int8", 1, 256)])
def test_repeated_launches_are_bit_identical(tag, m, fmt, gn, gk):
    """Three more launches reproduce the first bit for bit (workspace planes and stream-K counters are reused between them)."""
    c = _case("mild" if tag != "S4" else "sum", tag, fmt, gn, gk)
    _route(tag, m, fmt, gk)
    x = c["x"][:m] if c["x"] is not None else R.sparse_int_rows(m, c["k"]).to(DEV)
    a = _mm(x, c, gn, gk, c["bias"])
    same = torch.stack([(_bits(_mm(x, c, gn, gk, c["bias"])) == _bits(a)).all() for _ in range(3)] + [torch.isfinite(a).all()])
    assert same.tolist() == [True] * 4, same.tolist()


@pytest.mark.parametrize("fmt,gn,gk", R.formats_for("T1"))
def test_mtiled_rows_agree_with_the_skinny_engine(fmt, gn, gk):
    """Rows 0..63 of an M-tiled call at M = 129 against the 64-row skinny call on the same weights (same dequantiser, another fp32
    summation order): within one fp16 ulp of the largest value, ``2**-9 max|y| + 1e-6`` -- the bar of the neighbouring engines' tests."""
    c = _case("mild", "T1", fmt, gn, gk)
    assert _route("T1", 129, fmt, gk) == "mtiled" and _route("T1", 64, fmt, gk) == "skinny"
    a = _mm(c["x"][:129], c, gn, gk, c["bias"])[:64]
    b = _mm(c["x"][:64], c, gn, gk, c["bias"])
    res = torch.stack([torch.isfinite(a).all().float(), (a.float() - b.float()).abs().max(), b.float().abs().max()]).tolist()
    assert res[0] == 1.0 and res[1] <= res[2] * 2.0 ** -9 + 1e-6, res
