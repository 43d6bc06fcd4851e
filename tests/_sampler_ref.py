"""References for the sampler kernels (csrc/sampler.hip, the argmax kernels of csrc/norm_act.hip), written from the
contract -- the header of sampler.hip and ``oracle.top_p_distribution`` -- not from the kernels, and the cases the CPU and
the GPU tests share.

The contract of the nucleus draw: p = softmax(stored logit / T); tokens ordered by (probability descending, token index
ascending); ``before_i`` = the mass strictly before token i in that order; token i is kept iff ``before_i <= top_p``; the
draw at ``u`` is the first kept token, in TOKEN order, whose cumulative kept mass exceeds ``u * Z`` (strictly: a ``u`` on an
edge belongs to the next token).  A token of zero mass is never drawn.

Two ways to hold a kernel to it:
  * exact cases (``exact_cases``): rows whose masses are powers of two and whose sums are small integers, so every fp32
    quantity of the kernel is exact in any summation order and every draw must EQUAL ``nucleus_exact`` -- no tolerance;
  * windowed cases (``windowed_cases``): seeded rows against ``nucleus64`` under ``accept`` with ``DELTA`` = 1e-5, the one
    margin the first sampler test already used.  No draw is exempt."""

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

DELTA = 1e-5
T0 = float(np.float32(1.4426950408889634))  # the kernel's k = 1.4426950408889634f / T is exactly 2, 1, 0.5 at T0/2, T0, 2*T0
ZERO = np.iinfo(np.int64).min               # exponent sentinel of a zero-mass token in ``nucleus_exact``
N_U = 257
U_LAST = 1.0 - 2.0 ** -24                   # the largest fp32 below 1


# ----------------------------------------------------------------------------------------------------------------- #
# fp64 reference and the windowed rule
# ----------------------------------------------------------------------------------------------------------------- #
def nucleus64(logits, temperature, top_p):
    """``(p, before)``, both ``[rows, vocab]`` fp64 in token order.  ``logits``: the stored values in any float dtype;
    ``temperature`` / ``top_p``: per-row fp32 values (taken as they are stored).  A ``-inf`` logit has p = 0 and sorts after
    every finite one, so it is never kept while ``top_p < 1`` and never carries mass."""
    rows = logits.shape[0]
    t = torch.as_tensor(temperature, dtype=torch.float32).reshape(-1).expand(rows).double().view(-1, 1)
    p = torch.softmax(logits.detach().cpu().double() / t, dim=-1)
    sp, si = torch.sort(-p, dim=-1, stable=True)  # probability descending, token index ascending
    sp = -sp
    cum = torch.cumsum(sp, dim=-1)
    before_sorted = torch.cat([torch.zeros(rows, 1, dtype=torch.float64), cum[:, :-1]], dim=1)
    before = torch.empty_like(p).scatter_(1, si, before_sorted)
    return p, before


def kept64(before, top_p):
    tp = torch.as_tensor(top_p, dtype=torch.float32).reshape(-1).expand(before.shape[0]).double().view(-1, 1)
    return before <= tp


def _cdf(p, keep):
    m = torch.where(keep, p, torch.zeros_like(p))
    through = torch.cumsum(m, dim=-1)
    z = through[-1]
    return (through - m) / z, through / z, m / z


def windows(p, before, top_p, delta):
    """Inner and outer nucleus of one row and their renormalised token-order CDFs.  The inner threshold is clamped at 0:
    the first token of the order has ``before = 0`` and is kept for every ``top_p >= 0``."""
    top_p = float(np.float32(top_p))
    inner = before <= max(top_p - delta, 0.0)
    outer = before <= top_p + delta
    return inner, outer, _cdf(p, inner), _cdf(p, outer)


def accept(tok, u, row, delta=DELTA):
    """bool per draw.  ``row = (p, before, top_p)`` of one row; ``tok`` int64 ``[n]`` drawn at ``u`` ``[n]``.  A token is
    accepted iff it is in the outer nucleus, carries mass, and ``u`` lies within ``delta`` of the hull of the token's
    interval under the inner and under the outer renormalisation.  (For a token outside the inner nucleus the inner
    interval is the empty one at the mass of the inner tokens before it.)"""
    p, before, top_p = row
    tok = torch.as_tensor(tok, dtype=torch.int64).reshape(-1)
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
    inner, outer, (bi, ti, _), (bo, to, _) = windows(p, before, top_p, delta)
    inside = (tok >= 0) & (tok < p.shape[0])
    t = torch.where(inside, tok, torch.zeros_like(tok))
    lo = torch.minimum(bi[t], bo[t]) - delta
    hi = torch.maximum(ti[t], to[t]) + delta
    return inside & outer[t] & (p[t] > 0) & (lo <= u) & (u < hi)


DELTA_LADDER = [1e-5, 3e-6, 1e-6, 3e-7, 1e-7, 3e-8, 1e-8, 3e-9, 1e-9]


def smallest_delta(tok, u, row):
    """The smallest rung of ``DELTA_LADDER`` down to which every draw is accepted at every rung (``None``: not at 1e-5)."""
    best = None
    for d in DELTA_LADDER:
        if not bool(accept(tok, u, row, d).all()):
            break
        best = d
    return best


def must_draw(row, n_u, delta=DELTA):
    """Tokens a grid of spacing ``1 / n_u`` cannot miss: inner tokens whose mass -- under the outer renormalisation, the
    smallest the window allows -- exceeds ``2 / n_u + 2 * delta`` (an interval that wide, moved by at most ``delta`` at each
    end, still holds a grid point)."""
    p, before, top_p = row
    inner, _, _, (_, _, mo) = windows(p, before, top_p, delta)
    return (inner & (mo > 2.0 / n_u + 2.0 * delta)).nonzero().reshape(-1)


# ----------------------------------------------------------------------------------------------------------------- #
# the same rule in Python integers
# ----------------------------------------------------------------------------------------------------------------- #
@dataclass
class ExactNucleus:
    kept: list          # token ids that are kept and carry mass, ascending
    mass: list          # their masses in units of the smallest mass of the row (Python ints)
    total: int          # S, the mass of the whole row in those units
    z: int              # the kept mass
    tie_mass: int       # the smallest kept mass (the threshold value)
    ties: int           # tokens of the row at that mass
    ties_kept: int      # how many of them are kept: the lowest indices

    def draw(self, u):
        target = Fraction(float(u)) * self.z
        cum = 0
        for tok, m in zip(self.kept, self.mass):
            cum += m
            if cum > target:
                return tok
        raise AssertionError("u must lie in [0, 1)")


def nucleus_exact(exponents, top_p_num, top_p_den):
    """``exponents``: int64 array, token i has mass ``2^exponents[i]`` (``ZERO``: no mass).  Keep rule and inverse CDF in
    integers."""
    exponents = np.asarray(exponents, dtype=np.int64)
    pos = np.nonzero(exponents != ZERO)[0].tolist()
    lo = min(int(exponents[i]) for i in pos)
    m = {i: 1 << (int(exponents[i]) - lo) for i in pos}
    total = sum(m.values())
    kept, before = [], 0
    for i in sorted(pos, key=lambda i: (-m[i], i)):
        if before * top_p_den <= top_p_num * total:
            kept.append(i)
        before += m[i]
    tie_mass = min(m[i] for i in kept)
    kept.sort()
    return ExactNucleus(kept, [m[i] for i in kept], total, sum(m[i] for i in kept), tie_mass,
                        sum(1 for i in pos if m[i] == tie_mass), sum(1 for i in kept if m[i] == tie_mass))


# ----------------------------------------------------------------------------------------------------------------- #
# argmax and repetition penalty
# ----------------------------------------------------------------------------------------------------------------- #
def first_argmax(logits):
    """First index of the maximum of the stored values, ``+0 == -0``.  NaN is out of scope."""
    x = logits.detach().cpu().double()
    top = x.max(dim=-1, keepdim=True).values
    idx = torch.arange(x.shape[-1]).expand(x.shape)
    return torch.where(x == top, idx, torch.full_like(idx, x.shape[-1])).min(dim=-1).values


def penalty_ref(logits, token_ids, mask, penalty):
    """``x < 0 ? x * pen : x / pen`` in fp32 on the ORIGINAL logit, once per distinct token at a masked-in position,
    rounded once to the result dtype: the logits dtype for a Python scalar, the promoted dtype for a tensor penalty."""
    logits, token_ids, mask = logits.detach().cpu(), token_ids.detach().cpu().long(), mask.detach().cpu().bool()
    batch = logits.shape[0]
    if torch.is_tensor(penalty):
        out_dtype = torch.promote_types(logits.dtype, penalty.dtype)
        pen = penalty.detach().cpu().reshape(-1).to(torch.float32)
    else:
        out_dtype = logits.dtype
        pen = torch.full((batch,), float(penalty), dtype=torch.float32)
    out = logits.to(out_dtype).clone()
    for b in range(batch):
        toks = torch.unique(token_ids[b][mask[b]])
        x = logits[b, toks].to(torch.float32)
        out[b, toks] = torch.where(x < 0, x * pen[b], x / pen[b]).to(out_dtype)
    return out


def penalty_chunks(vocab):
    """The launch's chunk rule: ``(chunks, per)`` with workgroup c owning ``[c * per, min((c + 1) * per, vocab))``."""
    chunks = min(64, (vocab + 8191) // 8192)
    return chunks, (vocab + chunks - 1) // chunks


def argmax_chunks(rows, vocab):
    """``(chunks, per)`` of the split argmax as the wrapper routes it, ``None`` on the single-kernel path."""
    if vocab >= 16384 and rows < 1024:
        chunks = max(1, min(64, 2048 // max(rows, 1), vocab // 4096))
        return chunks, (vocab + chunks - 1) // chunks
    return None


def segment(vocab):
    """Tokens per wave segment of the nucleus kernel: ``ceil(vocab / 16)`` rounded up to 64."""
    return ((vocab + 15) // 16 + 63) // 64 * 64


# ----------------------------------------------------------------------------------------------------------------- #
# exact cases
# ----------------------------------------------------------------------------------------------------------------- #
@dataclass
class ExactCase:
    """Rows of one vocabulary.  ``exps [rows, vocab]``: the exponent ``l * k - max`` of every token (``ZERO``: no mass);
    ``k [rows]``: 2, 1 or 0.5, i.e. temperature ``T0 / k``; ``top_p``: (numerator, denominator) per row; the draws are at
    ``u = j / u_den``; ``ninf [rows]``: whether a zero-mass token is stored as ``-inf`` or as the integer -2048."""
    name: str
    exps: np.ndarray
    k: list
    top_p: list
    u_den: int
    ninf: list
    offset: int = 0
    notes: dict = field(default_factory=dict)

    @property
    def vocab(self):
        return self.exps.shape[1]

    def temperature(self):
        return torch.tensor([float(np.float32(T0) / np.float32(k)) for k in self.k], dtype=torch.float32)

    def top_p_f32(self):
        return torch.tensor([n / d for n, d in self.top_p], dtype=torch.float32)

    def u_grid(self):
        return torch.arange(self.u_den, dtype=torch.float32) / self.u_den

    def logits(self, dtype, seed=0):
        """``[rows, 2, vocab]`` storage: the rows are ``[:, 1, :]`` (what ``Sampler.sample`` slices out of ``[B, L, V]``);
        ``[:, 0, :]`` is filler that a kernel must not read."""
        rows, vocab = self.exps.shape
        g = torch.Generator().manual_seed(seed)
        store = torch.randint(-8, 9, (rows, 2, vocab), generator=g).to(torch.float32)
        for r in range(rows):
            x = torch.from_numpy(self.exps[r])
            live = x != ZERO
            l = torch.where(live, x, torch.zeros_like(x)).double() / self.k[r] + self.offset
            assert bool((l == l.round()).all())
            zero = float("-inf") if self.ninf[r] else -2048.0
            store[r, 1] = torch.where(live, l, torch.full_like(l, zero)).to(torch.float32)
        out = store.to(dtype)
        assert torch.equal(out.float(), store), "logits of an exact case are representable in every dtype"
        return out

    def expected(self):
        """``[u_den, rows]`` token ids and the per-row ``ExactNucleus``."""
        nuc = [nucleus_exact(self.exps[r], *self.top_p[r]) for r in range(self.exps.shape[0])]
        u = self.u_grid()
        want = torch.tensor([[n.draw(float(x)) for n in nuc] for x in u], dtype=torch.int64)
        return want, nuc


def _blank(rows, vocab):
    return np.full((rows, vocab), ZERO, dtype=np.int64)


def _case_halves():
    """Masses 1/2, 1/4, 1/8, 1/8 at scattered indices (one in the last, short segment), the rest zero mass.  top_p 1/2, 3/4
    and 7/8 put the mass before a token exactly ON top_p: that token is kept, the next is not.  top_p = 0: the maximum."""
    vocab = 1089
    combos = [((1, 1), 1, True), ((1, 2), 0.5, False), ((3, 4), 1, False), ((7, 8), 0.5, True), ((0, 1), 1, False),
              ((1, 1), 0.5, False), ((3, 4), 0.5, True), ((1, 2), 1, True)]
    exps = _blank(len(combos), vocab)
    for r in range(len(combos)):
        exps[r, [700, 5, 129, 1088]] = [0, -1, -2, -2]
    return ExactCase("halves", exps, [c[1] for c in combos], [c[0] for c in combos], 32, [c[2] for c in combos], offset=6)


def _case_top_p_zero():
    """top_p = 0 on dense rows: the first maximum, with the maximum duplicated at several indices."""
    vocab = 1089
    exps = np.tile(-1 - (np.arange(vocab, dtype=np.int64) % 8), (4, 1))
    for r, dup in enumerate([[900, 64, 65, 1088], [1088, 1087], [0, 1, 2], [1024, 1023, 63]]):
        exps[r, dup] = 0
    exps[2] *= 2  # k = 2 reaches even exponents only
    return ExactCase("top_p_zero", exps, [1, 0.5, 2, 1], [(0, 1)] * 4, 16, [False] * 4, offset=-4)


def _ties_rows(vocab, placements):
    """A head of mass 1/4, 40 tokens of mass 2^-6 and 16 of mass 2^-7 (the rest zero mass): tie j of the 40 has exactly
    1/4 + j/64 before it, so top_p = 16/64, 22/64 and 55/64 keep exactly 1, 7 and all 40 -- each ON the edge -- and no tail."""
    tails = [7, 8, 700, 701, 1500, 1501, 1502, 1503, 1504, 1505, 2500, 2501, 2502, 2503, 3000, 3001]
    rows, ks, tps, ninf, ties_at = [], [], [], [], []
    for pi, (head, ties) in enumerate(placements):
        assert len(ties) == 40 and not (set(ties) | {head}) & set(tails)
        for ti, tp in enumerate([(16, 64), (22, 64), (55, 64)]):
            x = np.full(vocab, ZERO, dtype=np.int64)
            x[tails] = -5
            x[ties] = -4
            x[head] = 0
            rows.append(x)
            ks.append(1 if (pi + ti) % 2 == 0 else 0.5)
            tps.append(tp)
            ninf.append((pi + ti) % 3 == 0)
            ties_at.append(list(ties))
    return np.stack(rows), ks, tps, ninf, ties_at


def _case_ties(name, placements):
    exps, ks, tps, ninf, ties_at = _ties_rows(4097, placements)
    return ExactCase(name, exps, ks, tps, 256, ninf, notes={"ties": ties_at, "kept": [1, 7, 40] * len(placements)})


def _case_vocab(vocab):
    """Mass at index 0, at ``vocab - 1`` and on both sides of every segment boundary ``w * seg``; everything else zero mass.
    Rows differ in temperature (k = 2, 1, 0.5 -- so a broadcast of row 0's fails), in top_p and in which position holds the
    maximum.  The last two rows hold ONE finite logit: it is drawn at every u."""
    seg = segment(vocab)
    pos = sorted({0, vocab - 1} | {i for w in range(1, 16) for i in (w * seg - 1, w * seg) if 0 < w * seg < vocab})
    combos = [((1, 1), 2), ((3, 4), 1), ((1, 2), 0.5), ((1, 1), 1), ((7, 8), 2), ((0, 1), 0.5)]
    exps = _blank(len(combos) + 2, vocab)
    for r, (_, k) in enumerate(combos):
        step = 2 if k == 2 else 1
        for n, i in enumerate(pos):
            exps[r, i] = -((n + r) % 4) * step
    exps[6, vocab - 1] = 0
    exps[7, pos[len(pos) // 2]] = 0
    ks = [c[1] for c in combos] + [1, 2]
    tps = [c[0] for c in combos] + [(1, 1), (1, 2)]
    return ExactCase(f"vocab{vocab}", exps, ks, tps, 64, [r % 2 == 0 for r in range(len(ks))], offset=2,
                     notes={"positions": pos})


EXACT_VOCABS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 1089, 4097, 128256, 151936, 152064]
SMALL_EXACT = 4097  # exact cases up to this vocabulary are cheap enough to run every mutant on


@functools.lru_cache(maxsize=None)
def exact_cases():
    seg = segment(4097)  # 320: segments [320 w, 320 (w + 1)), the last one [3840, 4097)
    one_stripe = (2000, list(range(seg + 10, seg + 50)))
    two_stripes = (2000, list(range(seg + 64 - 20, seg + 64 + 20)))
    two_segments = (10, list(range(2 * seg - 20, 2 * seg + 20)))
    last_segment = (10, list(range(4097 - 40, 4097)))
    cases = [_case_halves(), _case_top_p_zero(), _case_ties("ties_stripes", [one_stripe, two_stripes]),
             _case_ties("ties_segments", [two_segments, last_segment])]
    cases += [_case_vocab(v) for v in EXACT_VOCABS]
    return {c.name: c for c in cases}


# ----------------------------------------------------------------------------------------------------------------- #
# windowed cases
# ----------------------------------------------------------------------------------------------------------------- #
SPREADS = [1.0, 1.5, 3.0]
TEMPS = [0.05, 0.3, 1.0, 1.3, 5.0]
TOP_PS = [1e-6, 0.2, 0.9, 0.95, 1.0]
WINDOWED = [(152064, torch.float16, "cross"), (4097, torch.float32, "cross"), (152064, torch.bfloat16, "diag"),
            (128256, torch.float16, "diag"), (128256, torch.bfloat16, "diag")]
GROUP = 8  # distinct rows per launch


@dataclass
class WindowedCase:
    name: str
    store: torch.Tensor        # [rows, 2, vocab]; the rows are [:, 1, :]
    temperature: torch.Tensor  # [rows] fp32, rows differ
    top_p: torch.Tensor        # [rows] fp32, rows differ
    what: list                 # one word per row

    @property
    def logits(self):
        return self.store[:, 1, :]

    def u_grid(self):
        """``(j + 0.37) / 257`` plus the two ends: 0 and the largest fp32 below 1."""
        u = (torch.arange(N_U, dtype=torch.float64) + 0.37) / N_U
        return torch.cat([torch.zeros(1, dtype=torch.float64), u, torch.tensor([U_LAST], dtype=torch.float64)]).float()


def windowed_name(vocab, dtype, kind):
    return f"{vocab}-{str(dtype)[6:]}-{kind}"


@functools.lru_cache(maxsize=None)
def windowed_case(vocab, dtype, kind):
    """Seeded normal rows.  ``cross``: every temperature with every top_p, the spread cycling so that every temperature and
    every top_p meets all three; ``diag``: 8 of those.  Then the edge rows: 30 % of the logits at -inf (index 0 among them,
    top_p = 1: the draw at u = 0 must skip it); a -inf tail after the last positive token at top_p = 1; the last token of
    the vocabulary carrying most of the mass; eight equal logits at the top with the threshold in the middle of them (the
    ties' masses are far above DELTA, so how many are kept and which is pinned even here); top_p = 0."""
    g = torch.Generator().manual_seed(vocab * 7 + {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}[dtype])
    combos = [(SPREADS[(i + j) % 3], t, p) for i, t in enumerate(TEMPS) for j, p in enumerate(TOP_PS)]
    if kind == "diag":
        combos = [combos[i] for i in (4, 2, 8, 11, 5, 19, 20, 13)]
    what = [f"spread{s}-T{t}-p{p}" for s, t, p in combos]
    rows = [torch.randn(vocab, generator=g) * s for s, _, _ in combos]
    temps = [t for _, t, _ in combos]
    tps = [p for _, _, p in combos]

    def add(name, row, t, p):
        what.append(name), rows.append(row), temps.append(t), tps.append(p)

    row = torch.randn(vocab, generator=g) * 3.0
    row[torch.rand(vocab, generator=g) < 0.3] = float("-inf")
    row[0] = float("-inf")
    add("ninf30-p1", row, 1.0, 1.0)
    add("ninf30-p0.95", row.clone(), 0.7, 0.95)
    row = torch.randn(vocab, generator=g) * 1.0
    row[vocab - 1000:] = float("-inf")
    add("ninf-tail", row, 1.3, 1.0)
    row = torch.randn(vocab, generator=g) * 1.5
    row[vocab - 1] = 12.0
    add("heavy-last", row, 1.0, 0.9)
    row = torch.randn(vocab, generator=g) * 1.0
    row[torch.randperm(vocab, generator=g)[:8]] = 14.0
    add("planted-ties", row, 1.0, 0.45)
    add("top_p-zero", torch.randn(vocab, generator=g) * 1.5, 1.0, 0.0)
    store = torch.randn(len(rows), 2, vocab, generator=g) * 2.0
    store[:, 1, :] = torch.stack(rows)
    return WindowedCase(windowed_name(vocab, dtype, kind), store.to(dtype), torch.tensor(temps, dtype=torch.float32),
                        torch.tensor(tps, dtype=torch.float32), what)


@functools.lru_cache(maxsize=None)
def windowed_reference(vocab, dtype, kind):
    """``(p, before)`` of the case's stored rows: computed once, shared, never modified."""
    case = windowed_case(vocab, dtype, kind)
    return nucleus64(case.logits, case.temperature, case.top_p)


def check_windowed(tok, u, row, what):
    """Every rule of a windowed row in one place: ``tok [n]`` drawn at ``u [n]``.  Returns the list of what failed (empty:
    the row passes) -- the GPU test asserts it is empty, the CPU test also checks that wrong samplers fill it."""
    tok = torch.as_tensor(tok, dtype=torch.int64).reshape(-1)
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
    bad = []
    ok = accept(tok, u, row)
    if not bool(ok.all()):
        j = int((~ok).nonzero()[0])
        bad.append(f"{what}: {int((~ok).sum())} of {len(u)} draws outside their window, first u={float(u[j])!r} -> {int(tok[j])}")
    order = torch.argsort(u, stable=True)
    if bool((tok[order][1:] < tok[order][:-1]).any()):
        bad.append(f"{what}: tokens drawn at increasing u do not have non-decreasing indices")
    grid = (u > 0) & (u < U_LAST)  # the evenly spaced part
    need = must_draw(row, int(grid.sum()))
    missing = sorted(set(need.tolist()) - set(tok[grid].tolist()))
    if missing:
        bad.append(f"{what}: the grid never drew tokens {missing[:8]} although each holds more than two grid steps of mass")
    return bad
