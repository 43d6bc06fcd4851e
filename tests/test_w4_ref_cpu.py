"""CPU tests of ``tests/_w4_ref.py``: the exact restatement of the W4A16 decode engines' dequantisation, the float64 reference and
the derived error bound that ``tests/test_w4a16_row_groups_gpu.py`` holds the row-group loop to.  The checker is checked here: a
correct fp32 product passes the bound, and each of five wrong results fails it."""

import pytest
import torch

from oracle import oracle as O
from tests import _w4_ref as R

CUS = 256  # the compute units of the shapes below (what the host plan assumes without a device)
N4R, N4F, N5R, N5F = 32 * (3 * CUS + 4), 128 * CUS, 32 * (4 * CUS + 4), 160 * CUS
K_BOUNDED = 1280


def _ulp16(v: torch.Tensor) -> torch.Tensor:
    return 2 * R.half_ulp16(v.double())


@pytest.mark.parametrize("gs", [128, 256])
def test_dequant16_is_plain_integer_arithmetic_on_the_exact_case(gs):
    """Power-of-two scales, integer zeros: fp16(s), fp16(-z * s) and the fma are exact, so dequant16 == (q - z) * s bit for bit."""
    n, k = 384, 1280
    qw, sc, zr, bias = R.exact_case(n, k, gs, seed=1)
    want = (O.unpack_int4(qw).float() - zr.repeat_interleave(gs, 1)) * sc.repeat_interleave(gs, 1)
    got = R.dequant16(qw, sc, zr, gs)
    assert got.dtype == torch.float16 and got.shape == (n, k)
    assert torch.equal(got.float(), want)
    assert torch.equal((want + bias.float()[:, None]).half().float(), want + bias.float()[:, None])  # (q - z) * s + bias: an fp16 value
    assert torch.equal(R.unpack_int4(qw), O.unpack_int4(qw))
    assert set(sc.unique().tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0} and set(zr.unique().tolist()) == set(map(float, range(16)))
    assert bias.float().abs().max() <= 8 and torch.equal(bias.float(), bias.float().round())


@pytest.mark.parametrize("gs", [128, 256])
def test_dequant16_stays_within_three_ulps_of_the_oracle_weight(gs):
    """The claim of csrc/gemm_w4_common.h: against fp16(fp32((q - z) * s)) the engines' weight is off by at most 3 fp16 ulps (the
    roundings of s, of z * s and of the fma).  The ulp is that of the LARGER of the two terms q * s and z * s: the roundings
    happen at the terms' magnitude, so where q is close to z the small difference carries their absolute error (q == z: the
    oracle's weight is 0, the engines' up to 1.2e-4 on this draw -- 1920 ulps of the weight itself, 2 of the term).  Measured: 2."""
    n, k = 512, 1280
    _, qw, sc, zr, _ = R.dense_case(1, n, k, gs, seed=2)
    want = O.dequant_int4(qw, sc, zr, gs).half()
    got = R.dequant16(qw, sc, zr, gs)
    # ulp of the larger of the two terms q * s, z * s: where q ~ z the weight cancels and its own ulp says nothing about the roundings
    term = torch.maximum(O.unpack_int4(qw).float(), zr.repeat_interleave(gs, 1)) * sc.repeat_interleave(gs, 1)
    err = (got.double() - want.double()).abs()
    assert bool((err <= 3 * _ulp16(torch.maximum(want.float().abs(), term))).all())
    assert bool((err > 0).any())  # ... and the two definitions do differ: the kernels' bound must not be built on the oracle's weight


def _dense(m, n, k, gs, seed, bias=True):
    x, qw, sc, zr, b = R.dense_case(m, n, k, gs, seed)
    b = b if bias else None
    w16 = R.dequant16(qw, sc, zr, gs)
    y64, a64 = R.ref64(x, w16, b), R.abs_sum64(x, w16, b)
    return x, qw, sc, zr, b, w16, y64, a64, R.bound(y64, a64, k)


def test_a_correct_fp32_product_passes_and_the_oracle_is_measured_against_the_bound(capsys):
    """An fp32 matmul of the engines' own weights, bias added in fp32, rounded once to fp16 -- a correct kernel in the sense of
    ``bound`` -- passes ``assert_within``.  ``oracle.w4a16_matmul`` rounds the weight differently (fp32((q - z) * s), never to
    fp16).  Found on the dense draw at K = 1280 (seeds 3..7, up to 64 x 2048 outputs): the oracle stays INSIDE the bound, worst
    |err| / bound 0.58 - 0.68, against 0.30 - 0.35 for the correct product (whose error is almost all final rounding) -- the weight
    roundings are unbiased and average out over 1280 terms.  That is an observation about this draw, not a property: the
    kernels are bounded against ``ref64`` of ``dequant16``, and nothing in their bound depends on the oracle."""
    m, n, k, gs = 33, 768, K_BOUNDED, 128
    x, qw, sc, zr, b, w16, y64, a64, bnd = _dense(m, n, k, gs, seed=3)
    good = (x.float() @ w16.float().T + b.float()).half()
    worst = R.assert_within(good, y64, bnd, "fp32 product")
    orc = O.w4a16_matmul(x, qw, sc, zr, group_size=gs, bias=b)
    ratio = float(R.worst_ratio(orc, y64, bnd))
    frac = float((((orc.double() - y64).abs() / bnd) > 1).double().mean())
    with capsys.disabled():
        print(f"\n[w4_ref] worst |err| / bound at K={k}: correct fp32 product {worst:.3f}, oracle.w4a16_matmul {ratio:.3f} "
              f"({100 * frac:.2f} % of elements outside)")
    assert worst < 1.0
    assert torch.isfinite(orc).all() and ratio < 50  # recorded, not required: the same product, so near the bound and not orders away
    # planes: no rounding term
    assert torch.equal(R.bound(y64, a64, k, planes=True), (k + 1) * 2.0 ** -23 * a64)
    R.assert_within(x.float() @ w16.float().T, R.ref64(x, w16), R.bound(R.ref64(x, w16), R.abs_sum64(x, w16), k, planes=True), "fp32 planes")


def test_each_wrong_result_fails_assert_within():
    m, n, k, gs = 17, 512, K_BOUNDED, 128
    x, qw, sc, zr, b, w16, y64, a64, bnd = _dense(m, n, k, gs, seed=4)
    R.assert_bound_bites(x, w16, bnd)
    xf, bf = x.float(), b.float()

    def product(w):
        return xf @ w.float().T + bf

    wrong = {}
    wrong["all zeros"] = torch.zeros(m, n, dtype=torch.float16)
    # one product dropped from one output: the largest-magnitude term of the element (5, 77)
    t = xf[5] * w16[77].float()
    j = int(t.abs().argmax())
    d = product(w16)
    d[5, 77] -= t[j]
    wrong["one product dropped"] = d.half()
    # one group of 128 takes its neighbour's scale (every row's group 3 reads group 4's scale)
    sc2 = sc.clone()
    sc2[:, 3] = sc[:, 4]
    wrong["neighbour group's scale"] = product(R.dequant16(qw, sc2, zr, gs)).half()
    # one row takes the next row's zero (all its groups) -- a row whose zeros really differ
    zr2 = zr.clone()
    zr2[100] = zr[101]
    assert not torch.equal(zr[100], zr[101])
    wrong["next row's zero"] = product(R.dequant16(qw, sc, zr2, gs)).half()
    wrong["bias added twice"] = (product(w16) + bf).half()
    for what, got in wrong.items():
        with pytest.raises(AssertionError, match="outside the bound"):
            R.assert_within(got, y64, bnd, what)
    # the report names the element
    with pytest.raises(AssertionError, match="row 5, column 77"):
        R.assert_within(wrong["one product dropped"], y64, bnd, "dropped")
    bad = product(w16).half()
    bad[3, 9] = float("nan")
    with pytest.raises(AssertionError, match="non-finite output nan at row 3, column 9"):
        R.assert_within(bad, y64, bnd, "nan")


@pytest.mark.parametrize("n,gs", [(N4R, 128), (N4F, 256), (N5R, 256), (N5F, 128)])
def test_bound_bites_at_the_bounded_shapes(n, gs):
    """The four widths of the row-group tests at K = 1280 (a 2048-row sample of the N weight rows: the condition is about K and
    the draw, the sample keeps the maximum over ~130 000 outputs), the whole batch and a single row."""
    x, qw, sc, zr, b = R.dense_case(64, n, K_BOUNDED, gs, seed=n + gs)
    rows = torch.arange(0, n, n // 2048)[:2048]
    w16 = R.dequant16(qw[rows], sc[rows], zr[rows], gs)
    for m in (64, 1):
        y64, a64 = R.ref64(x[:m], w16, b[rows]), R.abs_sum64(x[:m], w16, b[rows])
        ratio = R.assert_bound_bites(x[:m], w16, R.bound(y64, a64, K_BOUNDED))
        assert 0.05 < ratio < 0.5


def test_bound_does_not_bite_at_the_headline_k():
    """K = 3584: the summation allowance has outgrown half a product -- the bounded tests must not be run there."""
    k = 3584
    x, qw, sc, zr, b = R.dense_case(64, 512, k, 128, seed=6)
    w16 = R.dequant16(qw, sc, zr, 128)
    with pytest.raises(AssertionError, match="could hide a dropped term"):
        R.assert_bound_bites(x, w16, (k + 1) * 2.0 ** -23 * R.abs_sum64(x, w16, b) + R.half_ulp16(R.ref64(x, w16, b)))
    with pytest.raises(AssertionError):
        R.bound(R.ref64(x, w16, b), R.abs_sum64(x, w16, b), k)  # ... and k (k + 1) u <= 1 no longer holds: the derivation stops at 2895


def test_half_ulp16_and_the_input_builders():
    v = torch.tensor([0.0, 2.0 ** -30, 2.0 ** -14, 1.0, 1.5, 2.0, 1023.9, 1024.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -2, 2.0 ** -1, 2.0 ** -10], dtype=torch.float64)
    assert torch.equal(R.half_ulp16(v), want)
    for m in (1, 17, 32, 33, 64):
        starts = R.one_hot_starts(m, 1280)
        hit = set()
        for k0 in starts:
            x = R.one_hot_rows(m, 1280, k0)
            assert x.sum() == m and bool((x.sum(1) == 1).all())
            hit |= set(x.nonzero()[:, 1].tolist())
        assert {c * 128 for c in range(10)} | {c * 128 + 127 for c in range(10)} <= hit
        if m in (32, 64):
            assert hit == set(range(1280))
    for m in (17, 64):
        x = R.sparse_int_rows(m, 1280)
        assert bool(((x != 0).sum(1) == 16).all()) and set(x.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert {int(c) // 16 for c in x.nonzero()[:, 1]} == set(range(80))  # every 16-k block of every chunk
