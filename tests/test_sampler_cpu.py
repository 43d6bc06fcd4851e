"""CPU tier of the sampler tests: the references of tests/_sampler_ref.py against the golden and the oracle, the proof that
the "exact" cases are exact in fp32, and the proof that the acceptance rules of tests/test_sampler_gpu.py have teeth: a
small fp32 emulation of the contract passes them everywhere, and the same emulation with each of a list of defects is
rejected by them, on an exact case and on a windowed one."""

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import _golden as G
from tests import _sampler_ref as R


def _golden():
    return np.load(G.GOLDEN_DIR + "/sampler_reference.npz")


# ----------------------------------------------------------------------------------------------------------------- #
# the references
# ----------------------------------------------------------------------------------------------------------------- #
def _dist64(logits, t, tp):
    p, before = R.nucleus64(logits, t, tp)
    d = torch.where(R.kept64(before, tp), p, torch.zeros_like(p))
    return d / d.sum(dim=-1, keepdim=True)


def test_nucleus64_reproduces_the_golden_and_the_oracle():
    d = _golden()
    logits = torch.from_numpy(d["topp.logits"])
    t, tp = torch.from_numpy(d["topp.temperature"]), torch.from_numpy(d["topp.top_p"])
    got = _dist64(logits, t, tp)
    want = torch.from_numpy(d["topp.dist"]).double()
    assert torch.equal(got > 0, want > 0)  # the same nucleus
    assert float((got - want).abs().max()) < 1e-6  # the golden is fp32
    g = torch.Generator().manual_seed(3)
    for dtype, vocab in ((torch.float16, 4097), (torch.bfloat16, 1025), (torch.float32, 63)):
        logits = (torch.randn(5, vocab, generator=g) * 2).to(dtype)
        logits[1, ::3] = float("-inf")
        t = torch.tensor([0.3, 1.0, 1.3, 5.0, 0.7])
        tp = torch.tensor([0.9, 1.0, 0.2, 0.95, 0.5])
        got, want = _dist64(logits, t, tp), O.top_p_distribution(logits, t, tp).double()
        # fp32 against fp64: a token whose mass before it is within 1e-6 of top_p may fall on either side
        p, before = R.nucleus64(logits, t, tp)
        near = (before - tp.double().view(-1, 1)).abs() < 1e-6
        assert torch.equal((got > 0) | near, (want > 0) | near)
        assert float(((got - want).abs() * ~near).max()) < 1e-5
        assert bool((got[1, ::3] == 0).all())  # -inf: no mass, never kept


def test_nucleus_exact_agrees_with_nucleus64_on_every_exact_case():
    for case in R.exact_cases().values():
        want, nuc = case.expected()
        logits = case.logits(torch.float32)[:, 1, :]
        p, before = R.nucleus64(logits, case.temperature(), case.top_p_f32())
        keep = R.kept64(before, case.top_p_f32()) & (p > 0)
        for r, n in enumerate(nuc):
            # T0 is log2(e) rounded to fp32, so the fp64 masses are powers of two only to ~1e-8: a token ON the threshold
            # may fall on either side here (that nucleus_exact places it right is checked by hand in the next test)
            edge = (before[r] - case.top_p_f32()[r].double()).abs() < 1e-6
            got = set(keep[r].nonzero().reshape(-1).tolist())
            assert got - set(edge.nonzero().reshape(-1).tolist()) <= set(n.kept) <= got | set(
                (edge & (p[r] > 0)).nonzero().reshape(-1).tolist()), (case.name, r)
            mass = torch.zeros(case.vocab, dtype=torch.float64)
            mass[n.kept] = torch.tensor(n.mass, dtype=torch.float64)  # small integers: the fp64 CDF below is exact
            cdf = torch.cumsum(mass, 0)
            u = case.u_grid().double()
            assert torch.equal((cdf.view(1, -1) > u.view(-1, 1) * n.z).float().argmax(dim=-1), want[:, r]), (case.name, r)
            assert torch.equal(O.sample_from_distribution(mass.view(1, -1).expand(len(u), -1), u), want[:, r])


def test_exact_cases_are_what_the_issue_lists():
    cases = R.exact_cases()
    for v in R.EXACT_VOCABS:
        c = cases[f"vocab{v}"]
        seg = R.segment(v)
        for w in range(1, 16):
            if w * seg < v:
                assert (c.exps[:6, [w * seg - 1, w * seg]] != R.ZERO).all()
        assert (c.exps[:6, [0, v - 1]] != R.ZERO).all()
        assert [(c.exps[r] != R.ZERO).sum() for r in (6, 7)] == [1, 1]
        assert len(set(c.k)) == 3 and c.k[0] != c.k[1]
    for name in ("ties_stripes", "ties_segments"):
        c = cases[name]
        want, nuc = c.expected()
        seg = R.segment(c.vocab)
        for r, n in enumerate(nuc):
            ties = c.notes["ties"][r]
            assert n.ties == 40 and n.ties_kept == c.notes["kept"][r]
            kept_ties = ties[:n.ties_kept]
            drawn = set(want[:, r].tolist())
            assert set(kept_ties) <= drawn and not set(ties[n.ties_kept:]) & drawn, (name, r)  # reachable / unreachable
        spans = [(min(t) // 64 == max(t) // 64, min(t) // seg == max(t) // seg) for t in
                 (cases["ties_stripes"].notes["ties"][0], cases["ties_stripes"].notes["ties"][3],
                  cases["ties_segments"].notes["ties"][0], cases["ties_segments"].notes["ties"][3])]
        assert spans[:3] == [(True, True), (False, True), (False, False)]
        last = cases["ties_segments"].notes["ties"][3]
        assert min(last) >= (c.vocab - 1) // seg * seg and c.vocab % seg != 0  # all in the last, short segment
    c = cases["halves"]
    want, nuc = c.expected()
    assert [len(n.kept) for n in nuc] == [4, 2, 3, 4, 1, 4, 3, 2]
    assert want[0].tolist() == [5, 5, 5, 5, 700, 5, 5, 5]  # u = 0: the first kept token in token order
    c = cases["top_p_zero"]
    assert c.expected()[0][3].tolist() == [64, 1087, 0, 63]


def _sums(e):
    fwd = np.float32(0)
    for x in e:
        fwd = np.float32(fwd + x)
    bwd = np.float32(0)
    for x in e[::-1]:
        bwd = np.float32(bwd + x)
    pair = e.copy()
    while len(pair) > 1:
        if len(pair) % 2:
            pair = np.append(pair, np.float32(0))
        pair = (pair[0::2] + pair[1::2]).astype(np.float32)
    return fwd, bwd, pair[0]


def test_exact_cases_are_exact_in_fp32():
    """The guard of the word "exact": every mass is a power of two within 2^-20 of the maximum, fp32 sums of a row taken
    forwards, backwards and pairwise all equal the integer sum, and ``top_p * S`` and every ``u * Z`` are representable."""
    from fractions import Fraction
    for case in R.exact_cases().values():
        want, nuc = case.expected()
        for r, n in enumerate(nuc):
            x = case.exps[r]
            live = x[x != R.ZERO]
            top = int(live.max())
            assert top - int(live.min()) <= 20, case.name
            unit = Fraction(1, 1 << (top - int(live.min())))        # the smallest mass when the maximum is 1.0
            e = np.ldexp(np.float32(1), (live - top).astype(np.int32)).astype(np.float32)
            assert n.total < 1 << 24
            for s in _sums(e):
                assert Fraction(float(s)) == n.total * unit, (case.name, r)
            tp = np.float32(case.top_p[r][0] / case.top_p[r][1])
            assert Fraction(float(tp)) == Fraction(*case.top_p[r])
            s32, z32 = np.float32(float(n.total * unit)), np.float32(float(n.z * unit))
            assert Fraction(float(np.float32(tp * s32))) == Fraction(*case.top_p[r]) * n.total * unit, (case.name, r)
            for u in case.u_grid().numpy():
                assert Fraction(float(np.float32(u * z32))) == Fraction(float(u)) * n.z * unit, (case.name, r, u)
            # the stored logits give these exponents: l * k is an integer
            l = case.logits(torch.float32)[r, 1].numpy()
            z = (l * np.float32(case.k[r])).astype(np.float32)
            fin = x != R.ZERO
            assert np.array_equal(z[fin] - z[fin].max(), (x[fin] - top).astype(np.float32))
            assert (z[~fin] < z[fin].max() - 1000).all()
        k32 = (np.float32(1.4426950408889634) / case.temperature().numpy()).tolist()
        assert k32 == [float(k) for k in case.k]


# ----------------------------------------------------------------------------------------------------------------- #
# an fp32 emulation of the contract, and its defects
# ----------------------------------------------------------------------------------------------------------------- #
MUTANTS = {
    "a": "keep iff before < top_p, not <=",
    "b-": "one tied token too few",
    "b+": "one tied token too many",
    "c": "ties kept from the highest index down",
    "d": "inverse CDF in sorted order, not token order",
    "e": "a draw on an edge gives the earlier token",
    "f": "the last segment's tail tokens are ignored (vocabulary rounded down to 64)",
    "g": "the temperature of row 0 is used for every row",
    "h": "the row stride is taken as the vocabulary",
    "i": "a zero-mass token is returned when u is near 1",
}


def _cumsum32(x):
    """fp32 prefix sums in three levels of 64, the way a kernel would: short chains, so the rounding stays near one ulp."""
    n = x.numel()
    pad = (-n) % 4096
    c0 = torch.cumsum(torch.cat([x, x.new_zeros(pad)]).view(-1, 64, 64), dim=2)
    t0 = c0[:, :, -1]
    c1 = torch.cumsum(t0, dim=1)
    t1 = c1[:, -1]
    off1 = torch.cumsum(t1, dim=0) - t1
    return ((off1.view(-1, 1) + (c1 - t0)).unsqueeze(2) + c0).reshape(-1)[:n]


def _emulate_row(l, temperature, top_p, u, mutant):
    f32 = np.float32
    if l.numel() == 0 or not bool(torch.isfinite(l.float()).any()):
        return torch.full((len(u),), -1, dtype=torch.int64)  # a defect left nothing to draw from
    k = torch.tensor(f32(1.4426950408889634) / f32(temperature))
    z = l.float() * k
    e = torch.exp2(z - z.max())
    s = e.sum()
    p_thr = torch.tensor(f32(top_p)) * s
    fits = (lambda a: bool(a < p_thr)) if mutant == "a" else (lambda a: bool(a <= p_thr))
    blo, bhi, g = 0, 0x3F800000, torch.tensor(0.0)
    while blo < bhi:  # the smallest t with (mass of e > t) fitting: positive floats order like their bit patterns
        mid = blo + ((bhi - blo) >> 1)
        a = torch.where(e > float(np.array(mid, dtype=np.uint32).view(f32)), e, torch.zeros_like(e)).sum()
        if fits(a):
            bhi, g = mid, a
        else:
            blo = mid + 1
    tau = float(np.array(bhi, dtype=np.uint32).view(f32))
    tie = e == tau
    c = int(tie.sum())
    n_tie = c
    if tau > 0 and c > 0:
        q = float((p_thr - g) / tau)
        if mutant == "a":
            n_tie = int(np.ceil(q))  # ties j with g + j * tau < P
        else:
            n_tie = int(np.floor(q)) + 1 + {"b-": -1, "b+": 1}.get(mutant, 0)
        n_tie = max(0 if mutant == "a" else 1, min(c, n_tie))
    rank = torch.cumsum(tie.to(torch.int64), 0) - 1
    keep_tie = tie & ((rank >= c - n_tie) if mutant == "c" else (rank < n_tie))
    keep = (e > tau) | keep_tie
    if mutant == "a" and float(p_thr) == 0.0:
        keep = torch.zeros_like(keep)  # before < 0 holds for no token
    order = torch.sort(-e, stable=True).indices if mutant == "d" else torch.arange(e.numel())
    idx = order[keep[order]]          # kept tokens in the order the CDF walks them
    if idx.numel() == 0:
        return torch.full((len(u),), -1, dtype=torch.int64)
    ke = e[idx]
    live = ke > 0
    if not bool(live.any()):
        return torch.full((len(u),), -1, dtype=torch.int64)
    # the running sum moves only at tokens that carry mass: a kept zero-mass token repeats the value before it
    cdf_live = torch.cummax(_cumsum32(ke[live]), 0).values
    seen = torch.cumsum(live.to(torch.int64), 0)
    cdf = torch.where(seen > 0, cdf_live[(seen - 1).clamp(min=0)], torch.zeros_like(ke))
    target = u.float() * cdf[-1]
    pos = torch.searchsorted(cdf, target, right=mutant != "e")  # first kept token with cdf > target (e: >=)
    last_live = idx[live.nonzero()[-1, 0]]
    tok = torch.where(pos < idx.numel(), idx[pos.clamp(max=idx.numel() - 1)], last_live)
    if mutant == "i":
        tok = torch.where(u > 0.9, idx.max(), tok)  # the last KEPT token, mass or not (tau = 0 keeps the zero-mass ones)
    return tok


def emulate(logits, temperature, top_p, u, mutant=None):
    """``[len(u), rows]`` tokens: the contract in fp32 (``exp2`` of ``l * k - max``, the keep rule by bisection, the token-order
    CDF), with the defect ``mutant`` of ``MUTANTS``.  ``logits`` may be a strided view of a larger tensor."""
    rows, vocab = logits.shape
    out = torch.empty(len(u), rows, dtype=torch.int64)
    for r in range(rows):
        l = logits[r]
        if mutant == "h":
            base = logits._base if logits._base is not None else logits
            start = logits.storage_offset() + r * vocab
            l = base.reshape(-1)[start:start + vocab]
        if mutant == "f":
            l = l[:vocab // 64 * 64]
        out[:, r] = _emulate_row(l, float(temperature[0 if mutant == "g" else r]), float(top_p[r]), u, mutant)
    return out


def _exact_failures(case, dtype, mutant):
    want, _ = case.expected()
    got = emulate(case.logits(dtype)[:, 1, :], case.temperature(), case.top_p_f32(), case.u_grid(), mutant)
    return int((got != want).sum())


def _windowed_failures(key, mutant, rows=None):
    case, (p, before) = R.windowed_case(*key), R.windowed_reference(*key)
    u = case.u_grid()
    got = emulate(case.logits, case.temperature, case.top_p, u, mutant)
    bad = []
    for r in (range(len(case.what)) if rows is None else rows):
        bad += R.check_windowed(got[:, r], u, (p[r], before[r], float(case.top_p[r])), f"{case.name} row {r} {case.what[r]}")
    return bad, got


def test_the_correct_emulation_passes_every_exact_case():
    for case in R.exact_cases().values():
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            if case.vocab > R.SMALL_EXACT and dtype != torch.float16:
                continue
            assert _exact_failures(case, dtype, None) == 0, (case.name, dtype)


@pytest.mark.parametrize("key", R.WINDOWED, ids=[R.windowed_name(*k) for k in R.WINDOWED])
def test_windowed_rows_are_tight_and_the_correct_emulation_passes(key):
    """Per seeded row: the window leaves few tokens optional -- ``|O| - |I|`` (tokens that carry mass) is at most 1 % of
    ``|O|`` or 32 -- and the correct emulation is accepted on every draw at DELTA.  Where ``top_p + DELTA >= 1`` the outer
    nucleus is the whole vocabulary by definition and the count says nothing (on a peaked row the last 1e-5 of mass is
    nearly every token); there the optional tokens must hold at most DELTA of mass together.  Also prints the smallest
    delta at which the emulation would still pass, next to which the GPU test prints the kernel's."""
    case, (p, before) = R.windowed_case(*key), R.windowed_reference(*key)
    widths = []
    for r in range(len(case.what)):
        inner, outer, _, _ = R.windows(p[r], before[r], float(case.top_p[r]), R.DELTA)
        live = p[r] > 0
        n_i, n_o = int((inner & live).sum()), int((outer & live).sum())
        widths.append(n_o)
        if float(case.top_p[r]) + R.DELTA < 1.0:
            assert n_o - n_i <= max(0.01 * n_o, 32), (case.name, r, case.what[r], n_i, n_o)
        else:
            assert float(p[r][outer & ~inner].sum()) <= R.DELTA * (1 + 1e-9), (case.name, r, case.what[r])
    if key[0] >= 100000:
        assert max(widths) > 50000 and min(widths) < 10, widths
    assert len(set(case.temperature.tolist())) > 3 and len(set(case.top_p.tolist())) > 3
    bad, got = _windowed_failures(key, None)
    assert not bad, bad
    u = case.u_grid()
    deltas = [R.smallest_delta(got[:, r], u, (p[r], before[r], float(case.top_p[r]))) for r in range(len(case.what))]
    print(f"{case.name}: nucleus widths {min(widths)} .. {max(widths)}; smallest passing delta of the fp32 emulation: "
          f"{max(deltas):.0e} (worst row {case.what[deltas.index(max(deltas))]})")


SMALL_WINDOWED = (4097, torch.float32, "cross")
WIDE_WINDOWED = (152064, torch.float16, "cross")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_defect_is_rejected_on_an_exact_and_on_a_windowed_case(mutant):
    exact = {}
    for case in R.exact_cases().values():
        if case.vocab <= R.SMALL_EXACT:
            n = sum(_exact_failures(case, dt, mutant) for dt in (torch.float32, torch.bfloat16))
            if n:
                exact[case.name] = n
    windowed = {}
    bad, _ = _windowed_failures(SMALL_WINDOWED, mutant)
    if bad:
        windowed[R.windowed_name(*SMALL_WINDOWED)] = bad
    if mutant in ("c", "d", "g", "h", "i"):  # also on vocabulary-sized rows, the last six (edge) rows for speed
        n_rows = len(R.windowed_case(*WIDE_WINDOWED).what)
        bad, _ = _windowed_failures(WIDE_WINDOWED, mutant, rows=range(n_rows - 6, n_rows))
        if bad:
            windowed[R.windowed_name(*WIDE_WINDOWED)] = bad
    print(f"mutant ({mutant}) {MUTANTS[mutant]}: wrong draws per exact case {exact}; windowed cases that reject it: "
          f"{ {k: len(v) for k, v in windowed.items()} }")
    assert exact, f"mutant ({mutant}) {MUTANTS[mutant]} passes every exact case {[c for c in R.exact_cases()]}"
    assert windowed, f"mutant ({mutant}) {MUTANTS[mutant]} passes the windowed case {R.windowed_name(*SMALL_WINDOWED)}"


# ----------------------------------------------------------------------------------------------------------------- #
# argmax and penalty references
# ----------------------------------------------------------------------------------------------------------------- #
def test_first_argmax_agrees_with_torch():
    g = torch.Generator().manual_seed(1)
    for n in (1, 63, 64, 65, 1023, 1025, 16385):
        for dtype in (torch.float16, torch.bfloat16, torch.float32):
            x = torch.randint(-3, 4, (4, n), generator=g).to(dtype)
            x[1] = float("-inf")
            x[2] = 2.0
            if n > 1:
                x[3, 0], x[3, -1] = -0.0, 0.0
                x[3, 1:-1] = -1.0
            want = torch.argmax(x.float(), dim=-1)
            assert torch.equal(R.first_argmax(x), want) and torch.equal(O.greedy_argmax(x.float()), want)
            assert want[1] == 0 and want[2] == 0 and want[3] == 0


def test_penalty_ref_agrees_with_the_oracle_and_the_golden():
    d = _golden()
    for dt, dtype in (("f32", torch.float32), ("f16", torch.float16)):
        logits = torch.from_numpy(d[f"rp_{dt}.logits"]).to(dtype)
        ids, mask = torch.from_numpy(d[f"rp_{dt}.ids"]), torch.from_numpy(d[f"rp_{dt}.mask"])
        assert torch.equal(R.penalty_ref(logits, ids, mask, 1.3).float(), torch.from_numpy(d[f"rp_{dt}.scalar_1p3"]))
        pen = torch.from_numpy(d[f"rp_{dt}.row_penalty"])
        got = R.penalty_ref(logits, ids, mask, pen)
        assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(d[f"rp_{dt}.per_row"]))
    g = torch.Generator().manual_seed(2)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        logits = (torch.randn(4, 300, generator=g) * 4).to(dtype)
        logits[:, :4] = torch.tensor([0.0, -0.0, -60000.0 if dtype == torch.float16 else -3e38, float("-inf")]).to(dtype)
        ids = torch.randint(0, 300, (4, 40), generator=g)
        ids[:, :4] = torch.arange(4)
        mask = torch.rand(4, 40, generator=g) > 0.3
        mask[:, :4] = True
        for pen in (1.3, 0.8, 1.0, torch.tensor([1.0, 1.1, 0.8, 2.0])):
            got, want = R.penalty_ref(logits, ids, mask, pen), O.apply_repetition_penalty(logits, ids, mask, pen)
            assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (dtype, pen)
    assert R.penalty_chunks(1) == (1, 1) and R.penalty_chunks(8193) == (2, 4097) and R.penalty_chunks(600000) == (64, 9375)
    assert R.argmax_chunks(1, 152064) == (37, 4110) and R.argmax_chunks(64, 152064) == (32, 4752)
    assert R.argmax_chunks(600, 152064) == (3, 50688) and R.argmax_chunks(1024, 152064) is None
