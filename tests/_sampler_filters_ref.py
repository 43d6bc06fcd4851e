"""References for ``ll_sample_filtered`` (csrc/sampler_filters.hip), written from its contract -- the header comment of the
entry point -- not from the kernel, and the cases the CPU and the GPU tests share.  Extends tests/_sampler_ref.py.

The contract, per row, with p = softmax(stored logit / T):
  1. top-k: v = the k-th largest stored logit; survivors = all tokens with logit >= v (ties of the k-th survive); k <= 0 or
     k >= vocab is off; -inf sorts last, and v = -inf keeps everything;
  2. top-p over the survivors: ordered by (probability descending, index ascending), ``before_i`` = the survivors' mass
     strictly before i; kept iff ``before_i <= top_p * (mass of the survivors)``;
  3. min-p: a kept token is dropped if ``p_i < min_p * p_max`` -- after the nucleus has been chosen;
  4. the draw at ``u``: the first token, in TOKEN order, whose cumulative kept mass strictly exceeds ``u * Z``.

Two ways to hold a kernel to it, as in _sampler_ref.py: exact cases (power-of-two masses, small integer sums: every draw
EQUALS ``filtered_exact``) and windowed cases (seeded rows against ``filtered64`` under ``accept_filtered`` at DELTA = 1e-5,
no draw exempt).  Top-k is defined on stored values, so it is exact in both."""

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

from tests._sampler_ref import (DELTA, DELTA_LADDER, N_U, T0, U_LAST, ZERO, ExactCase, ExactNucleus, _cdf, segment)


# ----------------------------------------------------------------------------------------------------------------- #
# the rule in Python integers
# ----------------------------------------------------------------------------------------------------------------- #
def top_k_survivors(exponents, k):
    """Token ids that survive top-k, ascending.  The stored logit rises with the exponent and a zero-mass token (``ZERO``,
    the smallest int64) is stored below every other, so the order of the exponents is the order of the stored values."""
    exponents = np.asarray(exponents, dtype=np.int64)
    vocab = len(exponents)
    if k <= 0 or k >= vocab:
        return list(range(vocab))
    v = np.sort(exponents)[vocab - k]
    return np.nonzero(exponents >= v)[0].tolist()


def filtered_exact(exponents, k, top_p_num, top_p_den, min_p):
    """``nucleus_exact`` with the two filters.  ``min_p``: the fp32 value the kernel is handed, compared as an exact
    rational against ``mass / largest mass``."""
    exponents = np.asarray(exponents, dtype=np.int64)
    survivors = np.asarray(top_k_survivors(exponents, k), dtype=np.int64)
    alive = survivors[exponents[survivors] != ZERO].tolist()
    lo = min(int(exponents[i]) for i in alive)
    m = {i: 1 << (int(exponents[i]) - lo) for i in alive}
    total = sum(m.values())
    top = max(m.values())
    nucleus, before = [], 0
    for i in sorted(alive, key=lambda i: (-m[i], i)):
        if before * top_p_den <= top_p_num * total:
            nucleus.append(i)
        before += m[i]
    tie_mass = min(m[i] for i in nucleus)
    ties = sum(1 for i in alive if m[i] == tie_mass)
    ties_kept = sum(1 for i in nucleus if m[i] == tie_mass)
    floor = Fraction(float(np.float32(min_p)))
    kept = sorted(i for i in nucleus if Fraction(m[i], top) >= floor)
    return ExactNucleus(kept, [m[i] for i in kept], total, sum(m[i] for i in kept), tie_mass, ties, ties_kept)


# ----------------------------------------------------------------------------------------------------------------- #
# fp64 reference and the windowed rule
# ----------------------------------------------------------------------------------------------------------------- #
def filtered64(logits, temperature, top_k):
    """``(p, before, ratio)``, each ``[rows, vocab]`` fp64 in token order: ``p`` the probability among the top-k survivors
    (0 for a token that top-k removed), ``before`` the survivors' mass strictly before the token in the order (probability
    descending, index ascending), ``ratio = p / p_max``.  Top-k is taken on the stored values, exactly."""
    x = logits.detach().cpu().double()
    rows, vocab = x.shape
    t = torch.as_tensor(temperature, dtype=torch.float32).reshape(-1).expand(rows).double().view(-1, 1)
    ks = torch.as_tensor(top_k, dtype=torch.int64).reshape(-1).expand(rows)
    alive = torch.ones_like(x, dtype=torch.bool)
    for r in range(rows):
        k = int(ks[r])
        if 0 < k < vocab:
            alive[r] = x[r] >= torch.sort(x[r], descending=True).values[k - 1]
    p = torch.softmax(torch.where(alive, x, torch.full_like(x, float("-inf"))) / t, dim=-1)
    sp, si = torch.sort(-p, dim=-1, stable=True)
    cum = torch.cumsum(-sp, dim=-1)
    before_sorted = torch.cat([torch.zeros(rows, 1, dtype=torch.float64), cum[:, :-1]], dim=1)
    before = torch.empty_like(p).scatter_(1, si, before_sorted)
    before = torch.where(alive, before, torch.full_like(before, float("inf")))  # a removed token is in no nucleus
    return p, before, p / p.max(dim=-1, keepdim=True).values


def windows_filtered(row, delta):
    """Inner and outer kept set of one row ``(p, before, ratio, top_p, min_p)`` and their renormalised token-order CDFs.
    Inner: ``before <= top_p - delta`` and ``ratio >= min_p + delta``; outer: ``before <= top_p + delta`` and
    ``ratio >= min_p - delta``.  The thresholds are clamped so that the maximum (before = 0, ratio = 1) is in both."""
    p, before, ratio, top_p, min_p = row
    top_p, min_p = float(np.float32(top_p)), float(np.float32(min_p))
    inner = (before <= max(top_p - delta, 0.0)) & (ratio >= min(min_p + delta, 1.0))
    outer = (before <= top_p + delta) & (ratio >= min_p - delta)
    return inner, outer, _cdf(p, inner), _cdf(p, outer)


def accept_filtered(tok, u, row, delta=DELTA):
    """The hull rule of ``_sampler_ref.accept`` over the two sets of ``windows_filtered``; bool per draw, none exempt."""
    p = row[0]
    tok = torch.as_tensor(tok, dtype=torch.int64).reshape(-1)
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
    inner, outer, (bi, ti, _), (bo, to, _) = windows_filtered(row, delta)
    inside = (tok >= 0) & (tok < p.shape[0])
    t = torch.where(inside, tok, torch.zeros_like(tok))
    lo = torch.minimum(bi[t], bo[t]) - delta
    hi = torch.maximum(ti[t], to[t]) + delta
    return inside & outer[t] & (p[t] > 0) & (lo <= u) & (u < hi)


def smallest_delta_filtered(tok, u, row):
    best = None
    for d in DELTA_LADDER:
        if not bool(accept_filtered(tok, u, row, d).all()):
            break
        best = d
    return best


def check_windowed_filtered(tok, u, row, what):
    """Every rule of a windowed row: the list of what failed (empty: the row passes)."""
    tok = torch.as_tensor(tok, dtype=torch.int64).reshape(-1)
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
    bad = []
    ok = accept_filtered(tok, u, row)
    if not bool(ok.all()):
        j = int((~ok).nonzero()[0])
        bad.append(f"{what}: {int((~ok).sum())} of {len(u)} draws outside their window, first u={float(u[j])!r} -> {int(tok[j])}")
    order = torch.argsort(u, stable=True)
    if bool((tok[order][1:] < tok[order][:-1]).any()):
        bad.append(f"{what}: tokens drawn at increasing u do not have non-decreasing indices")
    grid = (u > 0) & (u < U_LAST)
    n_u = int(grid.sum())
    inner, _, _, (_, _, mo) = windows_filtered(row, DELTA)
    need = (inner & (mo > 2.0 / n_u + 2.0 * DELTA)).nonzero().reshape(-1)
    missing = sorted(set(need.tolist()) - set(tok[grid].tolist()))
    if missing:
        bad.append(f"{what}: the grid never drew tokens {missing[:8]} although each holds more than two grid steps of mass")
    return bad


def u_grid():
    """``(j + 0.37) / 257`` plus the two ends, 0 and the largest fp32 below 1, as fp32."""
    u = (torch.arange(N_U, dtype=torch.float64) + 0.37) / N_U
    return torch.cat([torch.zeros(1, dtype=torch.float64), u, torch.tensor([U_LAST], dtype=torch.float64)]).float()


# ----------------------------------------------------------------------------------------------------------------- #
# exact cases
# ----------------------------------------------------------------------------------------------------------------- #
def next_up(x):
    """The fp32 one ulp above ``x``."""
    return float(np.nextafter(np.float32(x), np.float32(2.0)))


@dataclass
class FilterCase(ExactCase):
    """An ``ExactCase`` with ``top_k`` (int) and ``min_p`` (an fp32 value) per row; the draws are at ``u_grid()`` and at
    ``j / u_den``, the edges."""
    top_k: list = field(default_factory=list)
    min_p: list = field(default_factory=list)

    def u_grid(self):
        return torch.cat([u_grid(), torch.arange(self.u_den, dtype=torch.float32) / self.u_den])

    def nuclei(self):
        return [filtered_exact(self.exps[r], self.top_k[r], *self.top_p[r], self.min_p[r]) for r in range(self.exps.shape[0])]

    def expected(self):
        nuc = self.nuclei()
        want = torch.tensor([[n.draw(float(x)) for n in nuc] for x in self.u_grid()], dtype=torch.int64)
        return want, nuc


def _case(name, rows, vocab, offset=2, notes=None):
    """``rows``: dicts with ``at`` {index: exponent}, ``k`` (the kernel's 2, 1 or 0.5), ``top_p`` (num, den), ``top_k``,
    ``min_p`` and ``ninf``."""
    exps = np.full((len(rows), vocab), ZERO, dtype=np.int64)
    for r, row in enumerate(rows):
        for i, e in row["at"].items():
            exps[r, i] = e
    return FilterCase(name, exps, [r["k"] for r in rows], [r["top_p"] for r in rows], 64, [r.get("ninf", False) for r in rows],
                      offset=offset, notes=notes or {}, top_k=[r["top_k"] for r in rows], min_p=[r.get("min_p", 0.0) for r in rows])


def spread_positions(vocab):
    """Index 0, 1, the middle, ``vocab - 2``, ``vocab - 1`` and both sides of every wave segment boundary."""
    seg = segment(vocab)
    pos = {0, 1, vocab // 2, vocab - 2, vocab - 1} | {i for w in range(1, 16) for i in (w * seg - 1, w * seg) if 0 < w * seg < vocab}
    return sorted(i for i in pos if 0 <= i < vocab)


def _case_vocab(vocab):
    """Mass on ``spread_positions`` only, at four levels (1, 1/2, 1/4, 1/8 of the maximum) that rotate from row to row, so
    every level is shared by tokens of different segments.  Rows: ``k`` in {1, 2, vocab - 1, vocab}, half the positions (the
    k-th value in the middle of a level) and one more than the positions (the k-th value is a zero-mass token's: -inf on the
    rows with ``ninf``, else a finite value that underflows -- everything survives); ``min_p`` exactly a level's ratio (the
    level is kept) and one ulp above (it is dropped); top_p on and off; the kernel's k = 2, 1, 0.5."""
    pos = spread_positions(vocab)
    n = len(pos)
    plan = [(1, (1, 1), 0.0, 1), (2, (1, 1), 0.0, 0.5), (vocab - 1, (3, 4), 0.0, 2), (vocab, (1, 2), 0.25, 1),
            (n // 2, (1, 1), 0.0, 2), (n // 2, (7, 8), 0.25, 0.5), (n + 1, (1, 1), 0.5, 1), (n + 1, (3, 4), next_up(0.125), 2),
            (0, (1, 1), 0.125, 0.5), (0, (1, 1), next_up(0.25), 1), (2, (1, 2), next_up(0.5), 2), (1, (0, 1), 1.0, 1)]
    rows = []
    for r, (top_k, tp, mp, k) in enumerate(plan):
        step = 2 if k == 2 else 1
        rows.append(dict(at={i: -((j + r) % 4) * step for j, i in enumerate(pos)}, k=k, top_p=tp, top_k=top_k, min_p=mp,
                         ninf=r % 2 == 0))
    return _case(f"filters-vocab{vocab}", rows, vocab, notes={"positions": pos})


def _case_rationed():
    """Top-k, then a nucleus whose threshold tie is rationed inside the survivors.  A head of mass 64 (units of the smallest
    mass), 40 tokens of mass 4 that straddle a segment boundary, 16 of mass 2 and 32 of mass 1.  top_k = 41 leaves the head
    and the 40 (mass 224): tie j has 64 + 4 j before it, so top_p = 1/2 (112) keeps exactly ties 0 .. 12, the last ON the
    edge.  Over the whole row (288) the threshold would be 144 and keep 21; top_k = 45 lands inside the 16 and keeps them
    all.  Row 2 squares the masses (the kernel's k = 2: head 256, ties 1) and takes top_p = 7/8 of 296 = 259: ties 0 .. 3, with
    top_k = 30 landing inside the ties.  Then the first rows with a min-p floor at the ties' ratio (1/16: kept) and one ulp above (the ties go)."""
    vocab, seg = 4097, segment(4097)
    ties = list(range(2 * seg - 20, 2 * seg + 20))
    tails = [7, 8, 700, 701, 1500, 1501, 1502, 1503, 1504, 1505, 2500, 2501, 2502, 2503, 3000, 3001]
    dust = list(range(3500, 3532))
    at = {2000: 0, **{i: -4 for i in ties}, **{i: -5 for i in tails}, **{i: -6 for i in dust}}
    at2 = {i: 2 * e for i, e in at.items()}
    rows = [dict(at=at, k=1, top_p=(1, 2), top_k=41), dict(at=at, k=0.5, top_p=(1, 2), top_k=41, ninf=True),
            dict(at=at2, k=2, top_p=(7, 8), top_k=30), dict(at=at, k=1, top_p=(1, 2), top_k=45),
            dict(at=at, k=1, top_p=(1, 2), top_k=41, min_p=0.0625), dict(at=at, k=0.5, top_p=(1, 2), top_k=41, min_p=next_up(0.0625)),
            dict(at=at, k=1, top_p=(1, 2), top_k=0), dict(at=at, k=1, top_p=(1, 1), top_k=41, min_p=next_up(0.0625))]
    return _case("filters-rationed", rows, vocab, notes={"ties": ties, "nucleus_ties": [13, 13, 4, 17, 13, 13, 21, 40], "kept": [14, 14, 5, 18, 14, 1, 22, 1]})


def _case_order():
    """The one case that tells min-p AFTER the nucleus from min-p before it.  Masses 8, 4, 2, 1, 1 (sum 16), top_p = 3/4: the
    mass before the third token is 12 = 3/4 of 16, so the nucleus is the first three; min_p = 1/4 is the third token's ratio
    (2 / 8), so it stays: {8, 4, 2}.  Dropping the two 1s first would leave 14, of which 3/4 is 10.5 < 12: {8, 4}.  The same
    row tells the maximum from the sum as min-p's yardstick (2 / 16 < 1/4 would drop the third) and >= from >."""
    rows = []
    for vocab_pos, k in (([5, 70, 3, 200, 64], 1), ([299, 0, 150, 63, 298], 0.5)):
        rows.append(dict(at=dict(zip(vocab_pos, [0, -1, -2, -3, -3])), k=k, top_p=(3, 4), top_k=0, min_p=0.25))
    rows.append(dict(at=dict(zip([5, 70, 3, 200, 64], [0, -2, -4, -6, -6])), k=2, top_p=(3, 4), top_k=0, min_p=0.25, ninf=True))
    return _case("filters-order", rows, 300)


FILTER_VOCABS = [1, 2, 63, 64, 65, 1025, 4097, 152064]


@functools.lru_cache(maxsize=None)
def filter_cases():
    cases = [_case_vocab(v) for v in FILTER_VOCABS] + [_case_rationed(), _case_order()]
    return {c.name: c for c in cases}


# ----------------------------------------------------------------------------------------------------------------- #
# windowed cases
# ----------------------------------------------------------------------------------------------------------------- #
W_TOP_KS = [1, 50, 1000]
W_MIN_PS = [0.0, 0.01, 0.1]
W_TOP_PS = [0.9, 1.0]
W_TEMPS = [0.3, 1.0]
W_SHAPES = [(152064, torch.float16), (152064, torch.bfloat16), (4097, torch.float32)]
W_SPREADS = [1.0, 1.5, 3.0]


@dataclass
class WindowedFilterCase:
    name: str
    store: torch.Tensor        # [rows, 2, vocab]; the rows are [:, 1, :]
    temperature: torch.Tensor  # [rows] fp32
    top_p: torch.Tensor        # [rows] fp32
    top_k: torch.Tensor        # [rows] int32
    min_p: torch.Tensor        # [rows] fp32
    what: list

    @property
    def logits(self):
        return self.store[:, 1, :]


@functools.lru_cache(maxsize=None)
def windowed_filter_case(vocab, dtype):
    """Seeded normal rows, one per combination of ``W_TOP_KS x W_MIN_PS x W_TOP_PS x W_TEMPS`` (36), the spread cycling.
    fp16 and bf16 rows carry many equal stored logits, hence ties at the k-th value."""
    g = torch.Generator().manual_seed(vocab * 11 + {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}[dtype])
    combos = [(k, mp, tp, t) for k in W_TOP_KS for mp in W_MIN_PS for tp in W_TOP_PS for t in W_TEMPS]
    rows = [torch.randn(vocab, generator=g) * W_SPREADS[i % 3] for i in range(len(combos))]
    store = torch.randn(len(rows), 2, vocab, generator=g) * 2.0
    store[:, 1, :] = torch.stack(rows)
    col = lambda j, dt: torch.tensor([c[j] for c in combos], dtype=dt)
    return WindowedFilterCase(f"{vocab}-{str(dtype)[6:]}", store.to(dtype), col(3, torch.float32), col(2, torch.float32),
                              col(0, torch.int32), col(1, torch.float32),
                              [f"k{k}-minp{mp}-p{tp}-T{t}-spread{W_SPREADS[i % 3]}" for i, (k, mp, tp, t) in enumerate(combos)])


@functools.lru_cache(maxsize=None)
def windowed_filter_reference(vocab, dtype):
    """``(p, before, ratio)`` of the case's stored rows: computed once, shared, never modified."""
    case = windowed_filter_case(vocab, dtype)
    return filtered64(case.logits, case.temperature, case.top_k)


def windowed_row(case, ref, r):
    p, before, ratio = ref
    return p[r], before[r], ratio[r], float(case.top_p[r]), float(case.min_p[r])
