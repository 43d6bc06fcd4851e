"""CPU tests of ``tests/_w8_ref.py``: the exact restatement of the 8-bit engines' dequantisation, the reference's meaning of the same
weights, the distance allowed between the two, and the inputs ``tests/test_w8a16_engines_gpu.py`` feeds the three engines of
``w8a16_matmul``.  The checker is checked here: on every bounded case a correct fp32 product passes the derived bound and the
bound is small enough to notice one lost product; the route table of the GPU file is held against the host-side route query."""

import pytest
import torch

from oracle import oracle as O
from tests import _w8_ref as R


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def test_unit_scales_widen_every_code_exactly():
    """fp8: ``dequant16`` with unit scales is the reference's bit surgery times 256 on all 256 byte values, compared as bit patterns
    (so a NaN would have to be the same NaN; under the bit surgery the encodings 0x7F / 0xFF are +-480 and nothing is one).  int8:
    the codes themselves."""
    codes = torch.arange(256, dtype=torch.uint8).reshape(2, 128)
    ones = torch.ones(1, 1)
    got = R.dequant16_fp8(codes, ones, 128, 128)
    want = (O.fp8e4m3_bits_to_fp16(codes).float() * 256.0).half()
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(R.widen_fp8(codes)), _bits(O.fp8e4m3_bits_to_fp16(codes)))
    assert bool(torch.isfinite(got).all()) and got[0, 0x7F] == 480.0 and got[1, 0x7F] == -480.0
    finite = [c for c in range(256) if c & 0x7F != 0x7F]
    e4m3 = codes.view(torch.float8_e4m3fn).float().reshape(-1)[finite]
    assert torch.equal(got.float().reshape(-1)[finite], e4m3)  # every finite e4m3 value, subnormals included
    assert torch.equal(R.code_values64("fp8", codes).reshape(-1)[finite], e4m3.double())
    q = codes.view(torch.int8)
    assert torch.equal(R.dequant16_int8(q, ones, 128, 128).float(), q.float())


def test_expand_scales_covers_partial_groups_in_both_directions():
    s = torch.arange(1, 10, dtype=torch.float32).reshape(3, 3)
    e = R.expand_scales(s, 5, 7, 2, 3)
    assert e.shape == (5, 7)
    assert e[:, 0].tolist() == [1, 1, 4, 4, 7] and e[0].tolist() == [1, 1, 1, 2, 2, 2, 3]
    assert e[4, 6] == 9
    assert torch.equal(R.expand_scales(torch.tensor([2.0, 3.0]), 2, 4, 1, 99), torch.tensor([[2.0] * 4, [3.0] * 4]))  # group_k clamps to K
    with pytest.raises(AssertionError):
        R.expand_scales(s, 5, 7, 2, 2)


@pytest.mark.parametrize("fmt,gn,gk", [("fp8", 128, 128), ("fp8", 64, 256), ("int8", 1, 1152), ("int8", 1, 128), ("int8", 1, 256)])
@pytest.mark.parametrize("codes", ["all", "sum"])
def test_dequant16_is_plain_arithmetic_on_the_exact_case(fmt, gn, gk, codes):
    """Power-of-two scales: the multiplier and the product are exact, so ``dequant16 == true64`` outright -- the reference of the
    exact GPU tests is plain arithmetic.  The "sum" draw holds what the exact-sum test assumes: every weight a multiple of the
    quantum, ``1 <= |value| <= 448`` for fp8."""
    n, k = 388, 1152
    q, sc, bias = R.exact_case8(fmt, n, k, gn, gk, seed=1, codes=codes)
    w16, t64 = R.dequant16(fmt, q, sc, gn, gk), R.true64(fmt, q, sc, gn, gk)
    assert w16.dtype == torch.float16 and w16.shape == (n, k)
    assert torch.equal(w16.double(), t64)
    assert set(sc.unique().tolist()) == set(R.SCALE_CHOICES) and sc.shape == (-(-n // gn), -(-k // gk))
    assert bias.float().abs().max() <= 8 and torch.equal(bias.float(), bias.float().round())
    vals = R.code_values64(fmt, q)
    if fmt == "int8":
        assert int(q.min()) == -128 and int(q.max()) == 127
    elif codes == "all":
        assert len(q.unique()) == 256
    else:
        assert float(vals.abs().min()) == 1.0 and float(vals.abs().max()) == 448.0 and bool((vals < 0).any()) and bool((vals > 0).any())
    if codes == "sum" or fmt == "int8":
        scaled = t64 / R.sum_quantum(fmt)
        assert torch.equal(scaled, scaled.round())
    # + bias: the fp32 sum of one weight and the bias is exact (at most 15 bits apart), so an engine's output is it rounded once
    yb = w16.double() + bias.double()[:, None]
    assert torch.equal(yb.float().double(), yb)


@pytest.mark.parametrize("tag,fmt,gn,gk,ms", R.bounded_cases())
def test_bounded_cases_bite_pass_a_correct_product_and_tie_to_the_oracle(tag, fmt, gn, gk, ms, capsys):
    """Every checkpoint-scale case of the GPU file's bounded test, on the CPU: all scales inside the supported range and
    ``|dequant16 - true64| <= semantic_bound`` everywhere; the bound of the sum at most half the rms of one product
    (``assert_bound_bites``); an fp32 product rounded once passes ``assert_within`` -- a test the reference alone could not pass
    would be meaningless; and ``oracle.w8a16_matmul`` (the scale applied in fp32) lies within the semantic bound, propagated
    through the sum, of ``ref64(x, dequant16)`` -- plus the oracle's own fp32 summation and its rounding to fp16."""
    n, k = R.SHAPES[tag]
    x, q, sc, bias = R.checkpoint_case8(fmt, max(ms), n, k, gn, gk, R.case_seed(tag, fmt, gn, gk))
    assert bool(R.supported_scale(fmt, sc).all())
    w16, t64 = R.dequant16(fmt, q, sc, gn, gk), R.true64(fmt, q, sc, gn, gk)
    sb = R.semantic_bound(t64)
    assert bool(((w16.double() - t64).abs() <= sb).all())
    assert bool((w16.double() != t64).any())  # ... and the two definitions do differ
    if fmt == "fp8":
        assert bool((q & 0x7F != 0x7F).all()) and float(R.code_values64(fmt, q).abs().max()) == 448.0
    else:
        assert int(q.abs().max()) == 127
    rows = []
    for i, m in enumerate(ms):
        b = bias if i % 2 == 0 else None
        xm = x[:m]
        y64, a64 = R.ref64(xm, w16, b), R.abs_sum64(xm, w16, b)
        bnd = R.bound(y64, a64, k)
        bites = R.assert_bound_bites(xm, w16, bnd)
        good = xm.float() @ w16.float().T
        good = (good + b.float() if b is not None else good).half()
        worst = R.assert_within(good, y64, bnd, f"fp32 product {tag} {fmt} M={m}")
        rows.append((m, bites, worst))
        orc = O.w8a16_matmul(xm, q, sc, group_n=gn, group_k=gk, bias=b)
        allowed = xm.double().abs() @ sb.T + R.bound(y64, a64, k)  # semantic distance + the oracle's own summation and rounding
        assert bool(((orc.double() - y64).abs() <= allowed).all()), (tag, fmt, m)
    with capsys.disabled():
        print(f"\n[w8_ref] {tag} {fmt} g=({gn},{gk}): " + ", ".join(f"M={m} bound/product {b:.3f} fp32 |err|/bound {w:.3f}" for m, b, w in rows))


@pytest.mark.parametrize("tag,fmt,gn,gk", R.PARTIAL_CASES)
def test_partial_mode_cases_bite_and_pass_a_correct_product(tag, fmt, gn, gk):
    """The cases of the GPU file's partial-mode test, held to the bound without its rounding term: it bites, and fp32 planes of a
    correct product (two k-halves, added in float64 like the test does) pass."""
    n, k = R.SHAPES[tag]
    x, q, sc, _ = R.checkpoint_case8(fmt, 64, n, k, gn, gk, R.case_seed(tag, fmt, gn, gk))
    assert bool(R.supported_scale(fmt, sc).all())
    w16 = R.dequant16(fmt, q, sc, gn, gk)
    for m in (17, 64):
        xm = x[:m]
        y64, a64 = R.ref64(xm, w16), R.abs_sum64(xm, w16)
        bnd = R.bound(y64, a64, k, planes=True)
        assert R.assert_bound_bites(xm, w16, bnd) <= 0.5
        h = k // 256 * 128
        planes = torch.stack([xm[:, :h].float() @ w16[:, :h].float().T, xm[:, h:].float() @ w16[:, h:].float().T])
        assert R.assert_within(planes.double().sum(0), y64, bnd, f"fp32 planes {tag} {fmt}") <= 1.0


@pytest.mark.parametrize("fmt,gn,gk", [("int8", 1, 1152), ("int8", 1, 128), ("fp8", 128, 128)])
def test_subnormal_scale_variant_and_the_documented_loss_below_the_range(fmt, gn, gk, capsys):
    """The wide-spread draw: for int8 a share of the scales are fp16 subnormals and the weights of their blocks leave
    ``semantic_bound``; the documented limit is checked instead -- per block ``|fp16(s) - s| <= 2**-25``, so the weight's relative
    error is at most ``2**-25 / s + 2**-11`` (the multiplier's) plus ``2**-11`` (the product's, relative, or ``2**-25`` absolute).  fp8
    multiplies by ``s * 256`` and stays inside the range on this draw; both formats must show fp16-subnormal weights, which a
    flushing build would return as zero."""
    n, k = 388, 1152
    _, q, sc, _ = R.checkpoint_case8(fmt, 1, n, k, gn, gk, seed=7, spread="subnormal")
    ok = R.supported_scale(fmt, sc)
    w16, t64 = R.dequant16(fmt, q, sc, gn, gk), R.true64(fmt, q, sc, gn, gk)
    ok_w = R.expand_scales(ok.float(), n, k, gn, gk) > 0
    err = (w16.double() - t64).abs()
    assert bool((err[ok_w] <= R.semantic_bound(t64)[ok_w]).all())
    sub_w = float(((w16 != 0) & (w16.abs().double() < R.MIN_NORMAL16)).double().mean())
    assert sub_w > 0.002, sub_w
    mult = R.expand_scales(R.multiplier64(fmt, sc).float(), n, k, gn, gk).double()
    e_mult = 2.0 ** -25 / mult + 2.0 ** -11  # the multiplier's relative error: half the subnormal spacing, or half an ulp
    limit = t64.abs() * (e_mult + 2.0 ** -11 * (1 + e_mult)) + 2.0 ** -25
    assert bool((err <= limit).all())
    rel = torch.where(t64 != 0, err / t64.abs(), torch.zeros_like(err))
    if fmt == "int8":
        assert 0.05 < float((~ok).double().mean()) < 0.95
        big = t64.abs() >= 2.0 ** -13  # away from the product's own subnormal rounding: the multiplier's loss alone
        worst_in = float(rel[ok_w & big].max())
        worst_out = float(rel[~ok_w & big].max()) if bool((~ok_w & big).any()) else float(rel[~ok_w].max())
        smallest = float(sc[~ok].min())
        assert worst_in <= 2.0 ** -10 + 2.0 ** -22
        assert worst_out <= 2.0 ** -25 / smallest * (1 + 2.0 ** -11) + 2.0 ** -10 + 2.0 ** -22
        with capsys.disabled():
            print(f"\n[w8_ref] int8 g=({gn},{gk}) subnormal draw: {100 * float((~ok).double().mean()):.1f} % of scales below 2**-14 (smallest "
                  f"{smallest:.3e}); worst relative |dequant16 - true64| inside the range {worst_in:.2e}, below it {worst_out:.2e} "
                  f"(2**-25 / s = {2.0 ** -25 / smallest:.2e}); {100 * sub_w:.2f} % of weights fp16 subnormals")
    else:
        assert bool(ok.all())
        with capsys.disabled():
            print(f"\n[w8_ref] fp8 subnormal draw: every multiplier normal; {100 * sub_w:.2f} % of weights fp16 subnormals")


def test_which_draws_hold_fp16_subnormal_weights():
    """Where the bit-exact one-hot tests exercise kept denormals.  fp8 at checkpoint scales: the smallest codes times ``amax / 448``
    fall below 2**-14 already on the mild draw.  int8 on the mild draw: none -- the smallest non-zero weight is the scale itself,
    ``amax / 127`` ~ 5e-4 -- so for int8 it is the wide-spread variant that holds them (and the subnormal scales)."""
    def frac(fmt, gn, gk, spread):
        _, q, sc, _ = R.checkpoint_case8(fmt, 1, 388, 1152, gn, gk, seed=8, spread=spread)
        w16 = R.dequant16(fmt, q, sc, gn, gk)
        return float(((w16 != 0) & (w16.abs().double() < R.MIN_NORMAL16)).double().mean())

    assert 0.001 < frac("fp8", 128, 128, "mild") < 0.05
    assert frac("int8", 1, 1152, "mild") == 0.0
    assert 0.005 < frac("int8", 1, 1152, "subnormal") < 0.05 and 0.005 < frac("fp8", 128, 128, "subnormal") < 0.05


def test_input_builders_reach_every_k_position():
    for k in (128, 336, 640, 1152):
        for m in (1, 17, 32, 33, 64, 65, 200):
            hit = set()
            for k0 in R.one_hot_starts8(m, k):
                x = R.one_hot_wrapped(m, k, k0)
                assert bool((x.sum(1) == 1).all()) and x.sum() == m
                if m <= k:
                    assert bool((x.sum(0) <= 1).all())
                hit |= set(x.nonzero()[:, 1].tolist())
            edges = {c for c0 in range(0, k, 128) for c in (c0, min(c0 + 128, k) - 1)}
            assert edges <= hit, (k, m)
            if m >= 32 and m != 33:
                assert hit == set(range(k)), (k, m)


def test_route_table_matches_the_host_side_query():
    """``kernels.quantization.w8a16_engine`` (``ll_w8a16_engine``; host only, built from the launch functions' own predicates) names
    the engine the table of ``_w8_ref`` expects for every shape, batch and format of the GPU file, the skinny engine's plane counts
    are the table's, and strides the engines cannot take move the route."""
    from lite_llama_amd import _lib
    from lite_llama_amd.kernels.quantization import w8a16_engine

    def planes(n, k):
        return R.skinny_planes(_lib.lib().ll_dense8_partial_words(1, n, k), n, k)

    for tag, (n, k) in R.SHAPES.items():
        fmts = R.formats_for(tag)
        assert {f for f, _, _ in fmts} == {"fp8", "int8"} and ("fp8", 128, 128) in fmts and ("int8", 1, k) in fmts, (tag, fmts)
        assert len(set(fmts)) == len(fmts) and all(gk <= k for _, _, gk in fmts)
        for fmt, gn, gk in fmts:
            for m in R.DECODE_MS + (65, 100, 129, 200):
                assert w8a16_engine(m, n, k, fmt, gk) == R.want_engine(tag, m), (tag, fmt, gk, m)
    for tag, want in R.SKINNY_PLANES.items():
        assert planes(*R.SHAPES[tag]) == want, tag
    assert planes(130, 384) == 0 and planes(256, 336) == 0
    for tag, fmt, _, _ in R.PARTIAL_CASES:  # partial mode: where the streaming kernel serves, its split rule under the cap gives the count
        n, k = R.SHAPES[tag]
        assert R.streaming_planes(n, k, 12) == R.SKINNY_PLANES[tag]
        for m in (17, 64):
            wf = 1 if fmt == "fp8" else 2
            form, count = _lib.lib().ll_dense_partials_form(m, n, k, wf, 12), _lib.lib().ll_dense_partials_count(m, n, k, wf, 12)
            assert form in (1, 2) and 1 <= count <= 12 and (form == 1 or count == R.streaming_planes(n, k, 12))
    n, k = R.SHAPES["S3"]
    assert w8a16_engine(17, n, k, "fp8", 128, x_stride_m=k + 8, qw_stride_n=k + 16) == "skinny"
    assert w8a16_engine(129, 160, 1152, "int8", 128, x_stride_m=1152 + 8, qw_stride_n=1152 + 16) == "mtiled"
    assert w8a16_engine(17, n, k, "fp8", 128, x_stride_m=k + 4) == "none" and w8a16_engine(17, n, k, "fp8", 128, qw_stride_n=k + 8) == "none"
    assert w8a16_engine(17, n, k, "int8", 192) == "none" and w8a16_engine(0, n, k, "int8") == "none"
    assert w8a16_engine(17, n, k + 8, "int8") == "none" and w8a16_engine(17, n, k + 16, "int8") == "generic"
