"""CPU tier of the top-k / min-p sampler tests: the references of tests/_sampler_filters_ref.py against ``nucleus_exact`` and
against a plain torch composition, the proof that the exact cases are exact in fp32 and hold what the GPU test relies on,
and the proof that both acceptance rules have teeth: a list of defective samplers is rejected by them."""

from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _sampler_filters_ref as F
from tests import _sampler_ref as R

DEFECTS = {
    "drop-ties": "top-k drops the tokens tied with the k-th (keeps logit > v only, and the k-th itself by index)",
    "k-by-index": "top-k keeps exactly k tokens, the lowest indices among the tied",
    "row-mass": "the nucleus mass is top_p of the whole row, not of the survivors",
    "min-p-first": "min-p is applied before the nucleus is chosen",
    "min-p-of-sum": "min-p is relative to the sum, not to the maximum",
    "min-p-strict": "min-p keeps p > min_p * p_max, not >=",
}


# ----------------------------------------------------------------------------------------------------------------- #
# a second, independent statement of the rule -- a plain torch composition -- with the defects
# ----------------------------------------------------------------------------------------------------------------- #
LOG2E = 1.4426950408889634


def _compose(logits, scale, k, top_p, min_p, defect=None):
    """``(mass [vocab] fp64 with zeros outside the kept set, near [vocab] bool)``: mask below the k-th value, softmax, sort,
    cumsum, mask below ``min_p * max``.  The softmax is left unnormalised -- ``exp2(logit * scale - max)``, ``scale`` =
    log2(e) / T -- so that on an exact case (``scale`` 2, 1 or 0.5, integral products) every number here is exact in fp64.
    ``near``: tokens within 1e-6 of one of the two thresholds."""
    x = logits.double()
    vocab = x.numel()
    alive = torch.ones(vocab, dtype=torch.bool)
    if 0 < k < vocab:
        order = torch.sort(-x, stable=True).indices
        v = x[order[k - 1]]
        if defect == "drop-ties":
            alive = x > v
            alive[order[0]] = True
        elif defect == "k-by-index":
            alive = torch.zeros(vocab, dtype=torch.bool)
            alive[order[:k]] = True
        else:
            alive = x >= v
    z = x * scale
    p_row = torch.exp2(z - z.max())
    p = torch.where(alive, p_row, torch.zeros_like(p_row))
    floor = float(np.float32(min_p)) * (float(p.sum()) if defect == "min-p-of-sum" else float(p.max()))
    passes = (p > floor) if defect == "min-p-strict" and min_p > 0 else (p >= floor)
    if defect == "min-p-first":
        p = torch.where(passes, p, torch.zeros_like(p))
    total = float(p_row.sum()) if defect == "row-mass" else float(p.sum())
    sp, si = torch.sort(-p, stable=True)
    before = torch.empty_like(p).scatter_(0, si, torch.cumsum(-sp, 0) + sp)
    thr = float(np.float32(top_p)) * total
    keep = (before <= thr) & passes & (p > 0)
    near = ((before - thr).abs() < 1e-6 * total) | ((p - floor).abs() < 1e-6 * float(p.max()))
    return torch.where(keep, p, torch.zeros_like(p)), near & (p > 0)


def _draw64(mass, u):
    """Inverse CDF in token order, fp64: the first token whose cumulative mass exceeds ``u * Z``."""
    if not bool((mass > 0).any()):
        return torch.full((len(u),), -1, dtype=torch.int64)  # a defect left nothing to draw from
    cdf = torch.cumsum(mass, 0)
    pos = torch.searchsorted(cdf, u.double() * cdf[-1], right=True)
    last = int(mass.nonzero()[-1])
    return torch.where(pos < mass.numel(), pos, torch.full_like(pos, last))


def _exact_mutant(case, r, defect):
    """The kept set of row ``r`` of an exact case under ``defect``, through ``_compose`` on the stored fp32 logits."""
    l = case.logits(torch.float32)[r, 1]
    mass, _ = _compose(l, float(case.k[r]), case.top_k[r], case.top_p[r][0] / case.top_p[r][1], case.min_p[r], defect)
    return sorted(mass.nonzero().reshape(-1).tolist())


# ----------------------------------------------------------------------------------------------------------------- #
# the references
# ----------------------------------------------------------------------------------------------------------------- #
def test_filters_off_is_nucleus_exact_on_every_exact_case():
    for case in R.exact_cases().values():
        for r in range(case.exps.shape[0]):
            want = R.nucleus_exact(case.exps[r], *case.top_p[r])
            for k in (0, -3, case.vocab, case.vocab + 5):
                assert F.filtered_exact(case.exps[r], k, *case.top_p[r], 0.0) == want, (case.name, r, k)


def test_integer_reference_agrees_with_the_torch_composition():
    for case in F.filter_cases().values():
        for r, n in enumerate(case.nuclei()):
            assert _exact_mutant(case, r, None) == n.kept, (case.name, r)


def test_fp64_reference_agrees_with_the_torch_composition():
    """On seeded rows the kept set of ``windows_filtered`` at delta = 0 is the composition's, tokens within 1e-6 of a
    threshold aside, and top-k -- exact in both -- leaves the same survivors."""
    for vocab, dtype in ((4097, torch.float32), (1025, torch.float16), (2000, torch.bfloat16)):
        g = torch.Generator().manual_seed(vocab)
        logits = (torch.randn(12, vocab, generator=g) * 2).to(dtype)
        logits[3, ::5] = float("-inf")
        t = torch.tensor([0.3, 1.0, 1.3, 0.7] * 3)
        ks = torch.tensor([1, 50, 1000, 0, vocab, 7, 50, 300, 2, 1000, 50, 20])
        tps = [0.9, 1.0, 0.5, 0.9, 1.0, 0.2, 1.0, 0.9, 1.0, 0.95, 0.9, 1.0]
        mps = [0.0, 0.01, 0.1, 0.1, 0.0, 0.0, 0.3, 0.01, 0.5, 0.0, 0.1, 1.0]
        p, before, ratio = F.filtered64(logits, t, ks)
        for r in range(12):
            inner, outer, _, _ = F.windows_filtered((p[r], before[r], ratio[r], tps[r], mps[r]), 0.0)
            assert torch.equal(inner, outer)
            mass, near = _compose(logits[r], LOG2E / float(t[r]), int(ks[r]), tps[r], mps[r])
            assert torch.equal((inner & (p[r] > 0)) | near, (mass > 0) | near), (vocab, r)
            k = int(ks[r])
            if 0 < k < vocab:
                kth = torch.sort(logits[r].double(), descending=True).values[k - 1]
                assert torch.equal(p[r] > 0, (logits[r].double() >= kth) & (logits[r].double() > float("-inf")))
                assert int((logits[r].double() >= kth).sum()) >= k


# ----------------------------------------------------------------------------------------------------------------- #
# the exact cases
# ----------------------------------------------------------------------------------------------------------------- #
def test_filter_cases_are_exact_in_fp32():
    """Masses are powers of two within 2^-20 of the maximum; the survivors' fp32 sum and ``top_p * S`` are representable;
    every min-p comparison is one of representable numbers; and the fp32 product ``u * Z`` -- rounded, on the
    ``(j + 0.37) / 257`` grid -- lies on the same side of every cumulative mass as the exact product, so the draw through
    it is the integer reference's."""
    for case in F.filter_cases().values():
        want, nuc = case.expected()
        u = case.u_grid().numpy()
        for r, n in enumerate(nuc):
            x = case.exps[r]
            alive = np.asarray(F.top_k_survivors(x, case.top_k[r]))
            live = x[alive][x[alive] != R.ZERO]
            top = int(live.max())
            assert top == int(x[x != R.ZERO].max()) and top - int(live.min()) <= 20, case.name
            unit = Fraction(1, 1 << (top - int(live.min())))
            assert n.total < 1 << 24
            e = np.ldexp(np.float32(1), (live - top).astype(np.int32)).astype(np.float32)
            assert Fraction(float(e.sum(dtype=np.float32))) == Fraction(float(e[::-1].sum(dtype=np.float32))) == n.total * unit
            tp = np.float32(case.top_p[r][0] / case.top_p[r][1])
            assert Fraction(float(tp)) == Fraction(*case.top_p[r])
            s32, z32 = np.float32(float(n.total * unit)), np.float32(float(n.z * unit))
            assert Fraction(float(np.float32(tp * s32))) == Fraction(*case.top_p[r]) * n.total * unit, (case.name, r)
            assert 0.0 <= case.min_p[r] <= 1.0 and float(np.float32(case.min_p[r])) == case.min_p[r]
            cum = np.cumsum(np.asarray(n.mass, dtype=np.float64)) * float(unit)     # small integers times a power of two
            target = (u * z32).astype(np.float32)
            got = [n.kept[int(np.argmax(cum > t))] for t in target]
            assert got == want[:, r].tolist(), (case.name, r)
            l = case.logits(torch.float32)[r, 1].numpy()
            z = (l * np.float32(case.k[r])).astype(np.float32)
            fin = x != R.ZERO
            assert np.array_equal(z[fin] - z[fin].max(), (x[fin] - top).astype(np.float32))
            assert (z[~fin] < z[fin].max() - 1000).all()
        assert (np.float32(1.4426950408889634) / case.temperature().numpy()).tolist() == [float(k) for k in case.k]
        for dtype in (torch.float16, torch.bfloat16):
            case.logits(dtype)  # representable in every dtype (asserted inside)


def test_filter_cases_are_what_the_issue_lists():
    cases = F.filter_cases()
    assert [cases[f"filters-vocab{v}"].vocab for v in F.FILTER_VOCABS] == [1, 2, 63, 64, 65, 1025, 4097, 152064]
    for v in F.FILTER_VOCABS:
        c = cases[f"filters-vocab{v}"]
        seg = R.segment(v)
        assert {1, 2, v - 1, v} <= set(c.top_k) and set(c.k) == {2, 1, 0.5}
        nuc = c.nuclei()
        tied_across, kth_is_ninf = 0, 0
        for r in range(c.exps.shape[0]):
            k, x = c.top_k[r], c.exps[r]
            if not 0 < k < v:
                continue
            kth = np.sort(x)[v - k]
            tied = np.nonzero(x == kth)[0]
            if kth == R.ZERO:
                assert len(F.top_k_survivors(x, k)) == v            # everything survives
                kth_is_ninf += bool(c.ninf[r])
            elif len(tied) > 1 and len(F.top_k_survivors(x, k)) > k:
                tied_across += len({int(i) // seg for i in tied}) > 1
        if v >= 1025:
            assert tied_across >= 2 and kth_is_ninf >= 1, (v, tied_across, kth_is_ninf)
        if v >= 63:
            # rows 3 and 9: min_p = 1/4 keeps the tokens at a quarter of the maximum, one ulp above drops exactly them
            assert c.min_p[3] == 0.25 and c.min_p[9] == F.next_up(0.25) and c.min_p[9] > 0.25
            m9 = nuc[9]
            assert max(m9.mass) // min(m9.mass) == 2                # 1 and 1/2 stay
            quarter = [i for i in np.nonzero(c.exps[9] != R.ZERO)[0] if c.exps[9][i] == c.exps[9][c.exps[9] != R.ZERO].max() - 2]
            assert quarter and not set(quarter) & set(m9.kept)
            assert F.filtered_exact(c.exps[9], 0, 1, 1, 0.25).kept == sorted(set(m9.kept) | set(quarter))
            assert len(nuc[11].kept) >= 1 and len(set(nuc[11].mass)) == 1    # min_p = 1, top_p = 0: a maximum
    c = cases["filters-rationed"]
    want, nuc = c.expected()
    seg = R.segment(c.vocab)
    ties = c.notes["ties"]
    assert min(ties) // seg != max(ties) // seg                      # the tie group straddles two wave segments
    assert [n.ties_kept for n in nuc] == c.notes["nucleus_ties"] and [len(n.kept) for n in nuc] == c.notes["kept"]
    for r in (0, 1, 2, 4):
        drawn = set(want[:, r].tolist())
        assert set(ties[:nuc[r].ties_kept]) <= drawn and not set(ties[nuc[r].ties_kept:]) & drawn  # reachable / unreachable
    c = cases["filters-order"]
    assert [n.kept for n in c.nuclei()[:2]] == [[3, 5, 70], [0, 150, 299]]


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_every_defect_is_rejected_by_an_exact_case(defect):
    """The kept set under the defect differs from the reference's on some row, and draws of the grid land in the
    difference: a kernel with the defect fails the GPU test's equality."""
    caught = []
    for case in F.filter_cases().values():
        if case.vocab > R.SMALL_EXACT:
            continue
        want, nuc = case.expected()
        u = case.u_grid()
        for r, n in enumerate(nuc):
            assert _exact_mutant(case, r, None) == n.kept
            kept = _exact_mutant(case, r, defect)
            if kept == n.kept:
                continue
            mass = torch.zeros(case.vocab, dtype=torch.float64)
            x = case.exps[r]
            mass[kept] = torch.from_numpy(np.ldexp(1.0, (x[kept] - x[x != R.ZERO].max()).astype(np.int32)))
            if not torch.equal(_draw64(mass, u), want[:, r]):
                caught.append((case.name, r))
    assert caught, DEFECTS[defect]
    if defect in ("min-p-first", "min-p-of-sum", "min-p-strict"):
        assert ("filters-order", 0) in caught
    if defect == "row-mass":
        assert ("filters-rationed", 0) in caught


# ----------------------------------------------------------------------------------------------------------------- #
# the windowed rule
# ----------------------------------------------------------------------------------------------------------------- #
def _windowed_rows():
    """A few rows of the GPU test's own cases (the 4097 fp32 case whole would do; these keep the test short) and a bf16 row
    with ties at the k-th value."""
    key = (4097, torch.float32)
    case, ref = F.windowed_filter_case(*key), F.windowed_filter_reference(*key)
    out = [(case.logits[r], float(case.temperature[r]), int(case.top_k[r]), float(case.top_p[r]), float(case.min_p[r]),
            F.windowed_row(case, ref, r), case.what[r]) for r in range(len(case.what))]
    g = torch.Generator().manual_seed(9)
    l = (torch.randn(1, 4097, generator=g) * 1.5).to(torch.bfloat16)
    for k, tp, mp in ((300, 1.0, 0.0), (300, 0.9, 0.1)):
        p, before, ratio = F.filtered64(l, 1.0, k)
        assert int((p[0] > 0).sum()) > k, "the bf16 row has ties at the k-th value"
        out.append((l[0], 1.0, k, tp, mp, (p[0], before[0], ratio[0], tp, mp), f"bf16-k{k}-p{tp}-minp{mp}"))
    return out


def test_windowed_rule_accepts_the_contract_and_rejects_the_defects():
    u = F.u_grid()
    rejected = {d: 0 for d in DEFECTS}
    for l, t, k, tp, mp, row, what in _windowed_rows():
        mass, _ = _compose(l, LOG2E / float(np.float32(t)), k, tp, mp)
        assert not F.check_windowed_filtered(_draw64(mass, u), u, row, what)
        assert F.smallest_delta_filtered(_draw64(mass, u), u, row) == R.DELTA_LADDER[-1]
        for d in DEFECTS:
            bad_mass, _ = _compose(l, LOG2E / float(np.float32(t)), k, tp, mp, d)
            if (bad_mass > 0).sum() != (mass > 0).sum() or not torch.equal(bad_mass > 0, mass > 0):
                rejected[d] += bool(F.check_windowed_filtered(_draw64(bad_mass, u), u, row, what))
    # ">" instead of ">=" differs only when a ratio EQUALS min_p: an exact case's business
    assert all(n > 0 for d, n in rejected.items() if d != "min-p-strict"), rejected
