"""CPU tests of ``tests/_rowops_ref.py``: the checker of ``tests/test_rowops_gpu.py`` is checked here.  For the cases the GPU file
runs: (1) the project's fp32 oracle, or a plain fp32 restatement of the kernel, lies inside every bracket; (2) the smallest realistic
faults, restated on the CPU, leave it; (3) the share of brackets pinned to one value stays high on the random norm rows; (4) the
dispatch table the cases were chosen from quotes csrc/norm_act.hip line for line and the cases reach every instance and the second
trip of every grid-stride loop.  There is no host-side dispatch query: the launchers decide inside ``extern "C"`` entry points that
launch at once, and a query sharing their predicates would mean restructuring the launch code, so the table lives in the reference
module and ``test_dispatch_table_quotes_the_source`` fails when a quoted line changes."""

import pytest
import torch

from oracle import oracle as O
from tests import _rowops_ref as R

F16, BF16 = R.F16, R.BF16
IDS = {"ids": R.dname}


def _rejects(got, lo, hi):
    return not R.in_bracket(got, lo, hi)


# ------------------------------------------------------------------------------------------------------------------------------ #
# rounding and the checker itself
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_to_storage_rounds_once_where_a_detour_through_fp32_rounds_twice():
    for dtype, ulp in ((F16, 2.0 ** -10), (BF16, 2.0 ** -7)):
        tie = 1.0 + ulp / 2
        x = torch.tensor([tie + 2.0 ** -40, tie - 2.0 ** -40, tie, -(tie + 2.0 ** -40), 3 * ulp / 2 + 1.0 + 2.0 ** -40], dtype=torch.float64)
        want = torch.tensor([1.0 + ulp, 1.0, 1.0, -(1.0 + ulp), 1.0 + 2 * ulp], dtype=torch.float64)
        assert torch.equal(R.to_storage(x, dtype).double(), want), dtype
        assert float(x.float().to(dtype)[0]) == 1.0  # the detour: fp32 swallows the 2**-40, the tie then goes to even
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    for dtype in R.DTYPES:
        v = every.view(dtype)
        keep = ~torch.isnan(v)
        assert torch.equal(R.bits(R.to_storage(v.double(), dtype))[keep], every[keep])  # exact values stay, -0 and infinities too
    big = torch.tensor([65519.9, 65520.0, 1e300, -1e300, 2.0 ** -25, 2.0 ** -25 + 1e-20, float("nan")], dtype=torch.float64)
    got = R.to_storage(big, F16).double()
    assert got[:6].tolist() == [65504.0, float("inf"), float("inf"), float("-inf"), 0.0, 2.0 ** -24] and bool(torch.isnan(got[6]))


def test_assert_in_bracket_compares_values_and_skips_nothing():
    t = lambda *v: torch.tensor(v, dtype=F16)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    assert R.assert_in_bracket(t(1.0, -0.0, inf, nan), t(1.0, 0.0, inf, nan), t(1.0, 0.0, inf, nan)) == 1.0
    assert R.assert_in_bracket(t(1.0, 2.0), t(1.0, 1.0), t(1.0, 3.0)) == 0.5
    for got, lo, hi in ((t(nan), t(1.0), t(1.0)), (t(1.0), t(nan), t(nan)), (t(65504.0), t(inf), t(inf)), (t(inf), t(1.0), t(65504.0)),
                        (t(1.0), t(nan), t(2.0)), (t(1.001), t(1.0), t(1.0)), (t(-1.0), t(1.0), t(1.0))):
        assert _rejects(got, lo, hi), (got, lo, hi)
    with pytest.raises(AssertionError, match=r"1 of 2 elements outside .*50.00 % of the brackets are pinned.*first at \(1,\)"):
        R.assert_in_bracket(t(1.0, 4.0), t(1.0, 1.0), t(1.0, 3.0), "x")
    with pytest.raises(AssertionError):
        R.assert_in_bracket(t(1.0).to(BF16), t(1.0), t(1.0))
    lo, hi = R.candidates(t(2.0, 1.0, -1.0), t(1.0, 2.0, -1.0))
    assert lo.tolist() == [1.0, 1.0, -1.0] and hi.tolist() == [2.0, 2.0, -1.0]


# ------------------------------------------------------------------------------------------------------------------------------ #
# dispatch
# ------------------------------------------------------------------------------------------------------------------------------ #
def test_dispatch_table_quotes_the_source():
    assert R.dispatch_text_missing() == []


def test_the_cases_reach_every_instance_and_the_second_loop_trip():
    want = {("cached", t, v) for _, t, v in R.NORM_CACHED} | {("twopass", 8), ("twopass", 1)}
    assert {R.norm_instance(n) for n in R.NORM_NS} == want
    for (nv_max, tpr, vpt), (_, tpr2, vpt2) in zip(R.NORM_CACHED, R.NORM_CACHED[1:] + ((0, None, None),)):
        assert nv_max * 8 in R.NORM_NS and nv_max * 8 + 8 in R.NORM_NS  # both sides of every switch
        assert R.norm_instance(nv_max * 8) == ("cached", tpr, vpt)
        assert R.norm_instance(nv_max * 8 + 8) == (("cached", tpr2, vpt2) if tpr2 else ("twopass", 8))
    assert R.norm_instance(2048, aligned=False) == ("twopass", 1) and R.norm_instance(65536) == ("twopass", 8)
    assert [R.norm_rows(n) for n in (128, 256, 512, 2048)] == [[1, 15, 16, 17], [1, 7, 8, 9], [1, 3, 4, 5], [1, 2]]
    assert {R.partials_instance(n, s) for n in R.PART_NS for s in R.PART_S} == {(v, m) for v in (1, 2, 4) for m in (4, 6, 8, 12)}
    assert {R.slots_instance(n, k) for n in R.PART_NS for k in R.SLOT_K} == {(v, m) for v in (1, 2, 4) for m in (2, 4, 8)}
    for inst, counts in ((R.partials_instance, R.PART_S), (R.slots_instance, R.SLOT_K)):  # the count at the load count and one below
        loads = sorted({inst(8, c)[1] for c in counts})
        assert all(m in counts and m - 1 in counts for m in loads), loads
    rows, k, n = R.MOE_SUM_BIG
    assert R.grid_trips(rows, n, 4096) == (8, 4096, 2) and k == 2
    assert R.grid_trips(*R.SWIGLU_BIG_VEC, 4096) == (8, 4096, 2) and R.grid_trips(*R.SWIGLU_BIG_SCALAR, 4096) == (1, 4096, 2)
    assert R.grid_trips(1, R.ACT_BIG_VEC, 8192) == (8, 8192, 2) and R.grid_trips(1, R.ACT_BIG_SCALAR, 8192) == (1, 8192, 2)
    assert R.grid_trips(3, 300, 4096)[0] == 1 and R.grid_trips(3, 2048, 4096, aligned=False)[0] == 1
    assert R.rope_work(32, 8, 128, True, False) == (320, 2) and R.rope_work(28, 4, 24, False, False) == (384, 2)
    assert R.rope_work(64, 8, 256, True, True) == (1280, 2) and R.rope_work(80, 4, 24, False, True) == (1056, 2)
    assert R.rope_work(4, 2, 64, True, True) == (32, 1)
    assert set(R.rope_heads(128)) >= {(32, 8)} and set(R.rope_heads(24)) >= {(28, 4)}


def test_onehot_columns_cover_the_ends_every_vector_index_and_the_wave_boundaries():
    assert R.onehot_cols(8) == [0, 7] and R.onehot_cols(136) == [0, 135]
    assert R.onehot_cols(2048) == [0, 511, 512, 1023, 1024, 1535, 1536, 2047]
    assert R.onehot_cols(4096) == [0, 511, 512, 1023, 1024, 1535, 1536, 2047, 2048, 2559, 2560, 3071, 3072, 3583, 3584, 4095]
    c = R.onehot_cols(2056)  # (256, 2): v = 1 holds one vector
    assert {0, 2047, 2048, 2055, 511, 512, 1535, 1536} <= set(c) and max(c) == 2055
    c = R.onehot_cols(8192)
    assert {2047, 4095, 6143, 8191} <= set(c) and {4096 + 512 - 1, 4096 + 512} <= set(c)
    c = R.onehot_cols(65536)  # two-pass, 32 trips of 256 vectors
    assert {0, 511, 512, 2047, 2048, 65535, 31 * 2048 + 511, 31 * 2048 + 512, 31 * 2048 - 1} <= set(c)
    assert R.onehot_cols(300) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 299]
    for n in R.NORM_NS:
        assert all(0 <= v < n for v in R.onehot_cols(n)) and len(R.onehot_cols(n)) <= 40


# ------------------------------------------------------------------------------------------------------------------------------ #
# skip_rmsnorm
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.NORM_NS)
def test_norm_brackets_hold_the_oracle_pin_most_elements_and_reject_the_faults(n, dtype):
    """Per row width of the GPU file (17 rows; 64 below n = 1024, where 17 rows are too few elements to measure a share): the oracle
    and the fp32 restatement pass with and without a residual at both eps; the pinned share is at least 90 % (fp16) / 98 % (bf16);
    a vector of 8 columns lost from the sum of squares, the weight multiplied before the first rounding and -- on the 2**-12 rows,
    where eps carries the variance -- eps added outside the square root all leave the bracket."""
    rows = 64 if n < 1024 else 17
    floor = 0.90 if dtype == F16 else 0.98
    for with_res in (True, False):
        for kind in ("randn", "tiny", "big"):
            x, r, w = R.norm_inputs(kind, rows, n, dtype, with_res=with_res)
            for eps in R.NORM_EPS:
                (ylo, yhi), rb = R.norm_brackets(x, r, w, eps)
                y32, r32 = R.kernel_norm32(x, r, w, eps)
                share = R.assert_in_bracket(y32, ylo, yhi, f"fp32 restatement {kind} n={n} eps={eps}")
                yo, ro = O.skip_rmsnorm(x.clone(), None if r is None else r.clone(), w, eps)
                R.assert_in_bracket(yo, ylo, yhi, f"oracle {kind} n={n} eps={eps}")
                if with_res:
                    R.assert_in_bracket(r32, *rb, "residual")
                    R.assert_in_bracket(ro, *rb, "oracle residual")
                    assert R.pinned_share(*rb) > 0.99
                    assert _rejects((x.float() + r.float() + 2.0 ** -8).to(dtype), *rb)
                if kind == "randn":
                    print(f"norm n={n} {R.dname(dtype)} res={with_res} eps={eps}: pinned {100 * share:.2f} %")
                    assert share >= floor, (n, dtype, eps, share)
                    assert _rejects(R.kernel_norm32(x, r, w, eps, "drop8")[0], ylo, yhi), ("drop8", n, eps)
                    assert _rejects(R.kernel_norm32(x, r, w, eps, "w_first")[0], ylo, yhi), ("w_first", n, eps)
                if kind == "tiny":
                    assert _rejects(R.kernel_norm32(x, r, w, eps, "eps_outside")[0], ylo, yhi), ("eps_outside", n, eps)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.NORM_NS)
def test_onehot_rows_reject_the_loss_of_their_column(n, dtype):
    """One-hot energy rows: the restatement passes; losing the vector that holds the hot column moves ``y`` there from ``sqrt(n) w`` to
    ``w / sqrt(eps)`` and leaves the bracket on every row, at every n (the random rows notice a lost vector on fewer and fewer
    elements as n grows)."""
    for with_res in (True, False):
        x, r, w = R.onehot_inputs(n, dtype, with_res)
        cols = R.onehot_cols(n)
        assert x.shape[0] == len(cols)
        for eps in R.NORM_EPS:
            (ylo, yhi), rb = R.norm_brackets(x, r, w, eps)
            y32, r32 = R.kernel_norm32(x, r, w, eps)
            R.assert_in_bracket(y32, ylo, yhi, f"one-hot n={n}")
            if with_res:
                R.assert_in_bracket(r32, *rb)
                assert R.pinned_share(*rb) == 1.0
            for i, c in enumerate(cols):
                xi, ri = x[i:i + 1], None if r is None else r[i:i + 1]
                bad = R.kernel_norm32(xi, ri, w, eps, "drop8", drop_at=c)[0]
                assert _rejects(bad, ylo[i:i + 1], yhi[i:i + 1]), (n, c, eps)


# ------------------------------------------------------------------------------------------------------------------------------ #
# sums of planes and slots, moe_sum
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("form,counts", [("planes", R.PART_S), ("slots", R.SLOT_K)])
def test_plane_and_slot_sums_pass_restated_and_reject_a_dropped_or_doubled_plane(form, counts, dtype):
    eps = 1e-6
    for n in R.PART_NS + (300,):
        for cnt in counts:
            if form == "planes":
                if n == 300:
                    continue
                parts, r, w = R.plane_inputs(cnt, 3, n, dtype)
                dim = 0
            else:
                parts, r, w = R.slot_inputs(cnt, 3, n, dtype)
                dim = 1
            slo, shi = R.sum_bracket(parts, dim, dtype)
            assert R.pinned_share(slo, shi) == 1.0
            R.assert_in_bracket(R.kernel_sum32(parts, dim).to(dtype), slo, shi, "sum")
            (ylo, yhi), rb = R.partials_brackets(parts, dim, r, w, eps)
            x = R.kernel_sum32(parts, dim).to(dtype)
            y32, r32 = R.kernel_norm32(x, r, w, eps)
            R.assert_in_bracket(y32, ylo, yhi, f"{form} y n={n} count={cnt}")
            R.assert_in_bracket(r32, *rb, f"{form} r n={n} count={cnt}")
            if form == "slots":  # moe_sum in the oracle's words: the fp32 sum over the slots, rounded once
                R.assert_in_bracket(parts.float().sum(1).to(dtype), *R.candidates(slo, R.to_storage(parts.double().sum(1), dtype)))
            for fault in R.SUM_FAULTS:
                xb = R.kernel_sum32(parts, dim, fault).to(dtype)
                assert _rejects(xb, slo, shi), (fault, n, cnt)
                yb, rbad = R.kernel_norm32(xb, r, w, eps)
                assert _rejects(rbad, *rb) and _rejects(yb, ylo, yhi), (fault, n, cnt)


# ------------------------------------------------------------------------------------------------------------------------------ #
# swiglu, activations
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
def test_swiglu_bracket_holds_the_oracle_saturates_exactly_and_rejects_a_swapped_pair(dtype):
    for n in R.SWIGLU_NS:
        for kind, rows in (("randn", 37), ("edges", R.swiglu_edge_rows(n, dtype))):
            g, u = R.swiglu_inputs(kind, rows, n, dtype)
            lo, hi = R.swiglu_bracket(g, u)
            share = R.assert_in_bracket(O.swiglu_forward(g, u), lo, hi, f"oracle {kind} n={n}")
            R.assert_in_bracket(R.kernel_swiglu32(g, u), lo, hi, f"restatement {kind} n={n}")
            if kind == "randn":
                assert share > 0.95
                assert _rejects(R.kernel_swiglu32(u, g), lo, hi)
    g, u = R.swiglu_edges(dtype)
    lo, hi = R.swiglu_bracket(g, u)
    inf = float("inf")
    at = lambda gv, uv: ((g.double() == gv) & (u.double() == uv)).nonzero()[0, 0]  # noqa: E731
    top = float(torch.tensor(65504.0).to(dtype))
    sq = inf if dtype == F16 else top * top  # 65504**2 overflows fp16; bf16 holds 2**32
    for gv, uv, want in ((top, top, sq), (top, -top, -sq), (-top, top, 0.0), (0.0, top, 0.0), (-0.0, -1.0, 0.0)):
        i = at(gv, uv)
        assert float(lo[i]) == want and float(hi[i]) == want, (gv, uv, float(lo[i]), float(hi[i]))
    i = at(-88.0, top)  # sigmoid(-88) = 6e-39 is an fp32 subnormal: the bracket reaches from twice the true value to zero
    assert float(hi[i]) == 0.0 and (float(lo[i]) == 0.0 if dtype == F16 else -1e-31 < float(lo[i]) < -1e-32)
    i = at(-30.0, top)
    assert float(lo[i]) == float(hi[i]) < 0.0  # and nowhere else: sigmoid(-30) is a normal number
    if dtype == F16:
        i = at(30.0, 65504.0)
        assert float(lo[i]) == inf and float(hi[i]) == inf  # 30 * 65504 overflows fp16: the kernel must saturate
        i = at(2.0 ** -14, 1.0)
        assert float(lo[i]) == float(hi[i]) == 2.0 ** -15  # an fp16 subnormal result, pinned
    assert bool(torch.isfinite(lo.double()).logical_or(torch.isinf(lo.double())).all())


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_activation_brackets_hold_the_oracle(kind, dtype):
    for numel in R.ACT_NS + (8192,):
        x = R.act_inputs(numel, dtype)
        lo, hi = R.act_bracket(x, kind)
        R.assert_in_bracket(O.activation(x, kind), lo, hi, f"oracle {kind} {numel}")
        R.assert_in_bracket(R.kernel_act32(x, kind), lo, hi, f"restatement {kind} {numel}")
        if kind in ("relu", "leaky_relu"):
            assert R.pinned_share(lo, hi) == 1.0
        else:
            other = R.kernel_act32(x, "gelu" if kind == "tanh" else "tanh")
            assert _rejects(other, lo, hi)
    x = torch.tensor([float("nan"), -0.0, 0.0, -1.0, 2.0], dtype=dtype)
    lo, hi = R.act_bracket(x, "relu")
    assert bool(torch.isnan(lo[0])) and lo[1:].tolist() == [0.0, 0.0, 0.0, 2.0]
    assert _rejects(torch.zeros(5, dtype=dtype), lo, hi)  # a relu that drops the NaN


# ------------------------------------------------------------------------------------------------------------------------------ #
# RoPE
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("table", R.ROPE_TABLES, **IDS)
@pytest.mark.parametrize("hd", R.ROPE_HDS)
def test_rope_brackets_pass_the_restatement_and_reject_a_flipped_sine_and_a_wrong_row(hd, table, dtype):
    """Both table widths, the batched and the position-indexed form.  With an fp32 table the project's oracle computes in fp32 and
    must pass; with a 16-bit table it rounds every elementary operation in that type, which is exactly what the two candidates
    exclude -- the plain fp32 restatement stands in."""
    bs, sl = 3, 5
    for hq, hk in R.rope_heads(hd):
        for width in (hd, hd // 2):
            q, k, cos, sin = R.rope_inputs(bs, sl, hq, hk, hd, dtype, table, width)
            for x in (q, k):
                lo, hi = R.rope_bracket(x, cos, sin)
                share = R.assert_in_bracket(R.kernel_rope32(x, cos, sin), lo, hi, f"hd={hd} width={width}")
                assert share > (0.9 if table == torch.float32 else 0.99)
                assert _rejects(R.kernel_rope32(x, cos, sin, fault="sin_sign"), lo, hi)
                assert _rejects(R.kernel_rope32(x, cos, sin, fault="wrong_row"), lo, hi)
            if table == torch.float32:
                qo, ko = O.rope_emb_forward(q.clone(), k.clone(), cos, sin, bs, sl)
                R.assert_in_bracket(qo, *R.rope_bracket(q, cos, sin), "oracle q")
                R.assert_in_bracket(ko, *R.rope_bracket(k, cos, sin), "oracle k")
    q, k, cos, sin = R.rope_inputs(bs, sl, 4, 2, hd, dtype, table, hd, rows=40)
    pos = torch.randperm(40)[: bs * sl]
    lo, hi = R.rope_bracket(q, cos, sin, pos)
    R.assert_in_bracket(R.kernel_rope32(q, cos, sin, pos), lo, hi, "positions")
    assert _rejects(R.kernel_rope32(q, cos, sin, torch.arange(bs * sl)), lo, hi)
    assert _rejects(R.kernel_rope32(q, cos, sin, pos, fault="sin_sign"), lo, hi)
