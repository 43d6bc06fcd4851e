"""TEST INFRASTRUCTURE ONLY -- the row kernels of csrc/norm_act.hip (skip_rmsnorm in its four forms, moe_sum, swiglu in its
three forms, the element-wise activations, rope_emb_forward and rope_and_cache) restated in float64, the ROUNDING BRACKET every
correct result must fall into, the inputs and the dispatch table of ``tests/test_rowops_gpu.py``, and fp32 restatements of the
kernels (correct, and with one realistic fault each) that ``tests/test_rowops_ref_cpu.py`` runs through the same checker.  Plain
torch, device-agnostic; nothing here calls a kernel of the project.

The checker is ``assert_in_bracket(got, lo, hi)``: ``lo`` and ``hi`` are the float64 reference pushed down and up by the slack the
operation's own fp32 arithmetic can produce and then rounded ONCE to the storage type (``to_storage``; rounding is monotone, so a
value inside the float64 interval rounds inside ``[lo, hi]``).  Where ``lo == hi`` the element is pinned bit for bit.  The library
is built with ``-ffp-contract=off`` and IEEE division / square root, so every fp32 operation below rounds once, to nearest even.

Slacks, each derived from the code it checks:

* residual and plain sums (``r_out``; ``moe_sum``; the inner ``x = storage(sum of planes or slots)``).  The kernels add in fp32 in a
  fixed order, plane or slot 0 first, starting from 0.f (0 + p is exact), so sequential fp32 adds on any IEEE machine reproduce the
  fp32 sum exactly (``seq_sum32``).  The narrowing that follows has two candidates: the fp32 sum rounded to storage, and -- for a
  sum of TWO 16-bit values only -- the exact sum rounded once (the compiler may fuse ``fptrunc(fadd)`` into one mixed-precision
  instruction, see the note at ``ll_silu_mul_f32`` in csrc/common.h).  Two candidates are adjacent or equal storage values, so
  "``got`` is one of them" is the bracket ``[min, max]`` (``candidates``).  With more than one plane or slot the operand of the
  narrowing is an fp32 register that earlier adds already rounded: one candidate.
* RMSNorm output ``y = storage(storage(s * rrms) * w)`` with ``s`` the fp32 ``x + r``: ``var`` in float64 from ``s``, and the bracket
  from ``rrms (1 -+ NORM_DELTA)``, ``NORM_DELTA = 2**-16``, carried through both roundings (``storage(a) * w`` is exact in fp32: at
  most 22 significant bits).  Derivation: a term ``s*s/n`` carries two roundings (2 * 2**-24 relative); a thread adds at most 256
  positive terms serially (two-pass kernel at n = 65536: 32 trips of 8), then a tree of 8 to 10 adds: under 270 * 2**-24 relative on
  ``var``, half of it on ``rrms``, plus the roundings of ``var + eps``, sqrt, the division and ``s * rrms`` (2**-24 each):
  under 140 * 2**-24 < 2**-16 in all.
* swiglu ``storage(fp32(g * sigmoid(g)) * u)``: ``rel = 2**-20`` of the float64 value (hardware exp2 and reciprocal at 1 ulp each,
  three fp32 multiplies, the fp32 rounding of ``g * -log2 e`` amplified by ``|g| 2**-24`` on the exponential).  One correction to
  the issue's ``abs = 0``: where ``sigmoid(g) < 2**-126`` (g below about -87.3) the reciprocal's result is an fp32 SUBNORMAL -- it
  is rounded to a multiple of 2**-149 at best, and the hardware reciprocal may flush it to zero: there ``abs = |ref|``, a bracket
  that reaches from zero to twice the value (all of it below 1e-32 for 16-bit inputs); derived from the fp32 format, not from a
  result.  ``abs = 0`` everywhere else.
* tanh ``2 / (1 + exp(-2x)) - 1``: ``rel = abs = 2**-21`` (cancellation in the final subtraction).  gelu
  ``x/2 (1 + erf(x / sqrt 2))``: ``rel = 2**-21``, ``abs = 2**-21 |x|`` (cancellation in ``1 + erf``).  relu and leaky_relu
  (``x >= 0 ? x : storage(storage(0.01) * x)``) are exact.
* RoPE ``o1 = a c - b s``, ``o2 = b c + a s``.  16-bit tables: both products are exact in fp32, so the result is one fp32 rounding
  of the exact sum, then the narrowing -- or one rounding outright if fused: two candidates.  fp32 tables: the products round;
  ``rel = 2**-21`` and ``abs = 2**-22 (|a c| + |b s|)``.  V heads and every pool row are bit copies.
"""

from __future__ import annotations

import math
import os
import re

import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
NORM_DELTA = 2.0 ** -16
SWIGLU_REL, FP32_MIN_NORMAL = 2.0 ** -20, 2.0 ** -126
TANH_REL = TANH_ABS = GELU_REL = GELU_ABS = 2.0 ** -21
ROPE_REL, ROPE_ABS = 2.0 ** -21, 2.0 ** -22
SENT = 0x5A5A  # bit pattern of the sentinel the GPU tests pre-fill (fp16 211.25, bf16 about 1.5e16: a value no case produces)
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lite_llama_amd", "csrc", "norm_act.hip")


def dname(dtype) -> str:
    return {F16: "f16", BF16: "bf16", torch.float32: "f32"}[dtype]


# ------------------------------------------------------------------------------------------------------------------------------ #
# rounding and the checker
# ------------------------------------------------------------------------------------------------------------------------------ #
def round_odd32(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> fp32 rounded to ODD: exact values stay; an inexact one takes, of its two fp32 neighbours, the one whose last
    mantissa bit is set.  A later rounding to a format at least two bits narrower (fp16, bf16) then equals ONE rounding of the
    float64 value to nearest even (torch's own float64 -> half conversion goes through a nearest-even fp32 and rounds twice)."""
    f = x64.float()
    inexact = f.double() != x64
    even = (f.view(torch.int32) & 1) == 0
    inf = torch.full_like(f, float("inf"))
    other = torch.nextafter(f, torch.where(x64 > f.double(), inf, -inf))
    return torch.where(inexact & even & ~torch.isnan(x64), other, f)


def to_storage(x64: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding of a float64 value to ``dtype`` (nearest even, subnormals kept, overflow to infinity)."""
    return round_odd32(x64).to(dtype)


def candidates(a: torch.Tensor, b: torch.Tensor):
    """``(lo, hi)`` of two candidate results in the storage type: the bracket "``got`` is one of the two" when they are adjacent."""
    le = a.double() <= b.double()
    return torch.where(le, a, b), torch.where(le, b, a)


def bracket(ref64: torch.Tensor, slack64: torch.Tensor, dtype):
    """``(lo, hi)``: ``ref -+ slack`` rounded once to ``dtype``.  A NaN reference gives NaN on both sides."""
    return to_storage(ref64 - slack64, dtype), to_storage(ref64 + slack64, dtype)


def pinned_share(lo: torch.Tensor, hi: torch.Tensor) -> float:
    same = (lo.double() == hi.double()) | (torch.isnan(lo) & torch.isnan(hi))
    return float(same.double().mean()) if same.numel() else 1.0


def assert_in_bracket(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, what: str = "") -> float:
    """Every element of ``got`` lies in ``[lo, hi]`` as a value (so +0 meets -0); nothing is skipped: an infinite bound must be met
    by that infinity, a NaN bracket by a NaN.  Returns the share of pinned elements and names it in the failure."""
    assert got.shape == lo.shape == hi.shape, (what, tuple(got.shape), tuple(lo.shape), tuple(hi.shape))
    assert got.dtype == lo.dtype == hi.dtype, (what, got.dtype, lo.dtype, hi.dtype)
    g, l, h = got.double(), lo.double(), hi.double()
    nan_ref = torch.isnan(l) | torch.isnan(h)
    ok = torch.where(nan_ref, torch.isnan(g) & torch.isnan(l) & torch.isnan(h), (g >= l) & (g <= h))
    share = pinned_share(lo, hi)
    if not bool(ok.all()):
        bad = (~ok).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)) if got.dim() else ()
        raise AssertionError(f"{what}: {bad.numel()} of {ok.numel()} elements outside their bracket ({100 * share:.2f} % of the "
                             f"brackets are pinned to one value); first at {idx}: got {float(g.reshape(-1)[i])!r}, "
                             f"bracket [{float(l.reshape(-1)[i])!r}, {float(h.reshape(-1)[i])!r}]")
    return share


def in_bracket(got, lo, hi) -> bool:
    try:
        assert_in_bracket(got, lo, hi)
    except AssertionError:
        return False
    return True


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def sentinel(shape, dtype, device=None) -> torch.Tensor:
    return torch.full(tuple(shape), SENT, dtype=torch.int16, device=device).view(dtype)


def is_sentinel(t: torch.Tensor) -> torch.Tensor:
    return bits(t) == SENT


# ------------------------------------------------------------------------------------------------------------------------------ #
# dispatch, restated from csrc/norm_act.hip (``DISPATCH_TEXT`` quotes the lines; the CPU tests hold the quotes against the file)
# ------------------------------------------------------------------------------------------------------------------------------ #
NORM_CACHED = ((16, 16, 1), (32, 32, 1), (64, 64, 1), (256, 256, 1), (512, 256, 2), (1024, 256, 4))  # (nv <=, TPR, VPT): 142-147
DISPATCH_TEXT = (
    # launch_skip_rmsnorm, norm_act.hip:132-148
    "const bool vec = (n % 8 == 0) && ll_aligned16(y) && ll_aligned16(x) && ll_aligned16(w) &&",
    "if (nv <= 16) LL_NORM_CASE(16, 1);", "else if (nv <= 32) LL_NORM_CASE(32, 1);", "else if (nv <= 64) LL_NORM_CASE(64, 1);",
    "else if (nv <= 256) LL_NORM_CASE(256, 1);", "else if (nv <= 512) LL_NORM_CASE(256, 2);",
    "else if (nv <= 1024) LL_NORM_CASE(256, 4);",
    "else skip_rmsnorm_twopass<DT, 8, HAS_RES><<<dim3((unsigned)rows), 256, 0, st>>>(y, x, r, w, rows, n, eps);",
    "if (rows < 0 || n <= 0 || n > 65536) return LL_ERR_SHAPE;",
    # ll_skip_rmsnorm_partials, :233, :246-249
    "if (rows < 0 || n <= 0 || n % 8 != 0 || n > 8192 || s_count < 1 || s_count > 12) return LL_ERR_SHAPE;",
    "if (s_count <= 4) LL_PART_CASE(DT, VPT, 4); else if (s_count <= 6) LL_PART_CASE(DT, VPT, 6);",
    "else if (s_count <= 8) LL_PART_CASE(DT, VPT, 8); else LL_PART_CASE(DT, VPT, 12)",
    "if (nv <= 256) { LL_PART_S(DT, 1); } else if (nv <= 512) { LL_PART_S(DT, 2); } else { LL_PART_S(DT, 4); }",
    # ll_skip_rmsnorm_slots, :314, :325-327
    "if (rows < 0 || n <= 0 || n % 8 != 0 || n > 8192 || k_count < 1 || k_count > 8) return LL_ERR_SHAPE;",
    "if (k_count <= 2) LL_SLOT_CASE(DT, VPT, 2); else if (k_count <= 4) LL_SLOT_CASE(DT, VPT, 4); else LL_SLOT_CASE(DT, VPT, 8)",
    "if (nv <= 256) { LL_SLOT_K(DT, 1); } else if (nv <= 512) { LL_SLOT_K(DT, 2); } else { LL_SLOT_K(DT, 4); }",
    # launch_swiglu :391-393, ll_activation :452-454, ll_moe_sum :498-500
    "const bool vec = (n % 8 == 0) && ll_aligned16(c) && ll_aligned16(a) && (MODE != 0 || ll_aligned16(b));",
    "const unsigned grid = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);",
    "const bool vec = (n % 8 == 0) && ll_aligned16(y) && ll_aligned16(x);",
    "const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);",
    "const bool vec = (n % 8 == 0) && ll_aligned16(out) && ll_aligned16(x);",
    # ll_rope :566-571, ll_rope_kv_update :670-676
    "const bool vec = (hd % 16 == 0) && ll_aligned16(q) && ll_aligned16(k) && (q_row_stride % 8 == 0) &&",
    "rope_kernel<DT, CS, VEC><<<dim3((unsigned)tokens), 256, 0, st>>>(",
    "const bool vec = (hd % 16 == 0) && ll_aligned16(q) && ll_aligned16(kv) && ll_aligned16(kv_buffer) &&",
    "const bool csv = vec && cs_dtype != LL_F32 && ll_aligned16(cos_t) && ll_aligned16(sin_t) &&",
    "((cos_b_stride | cos_s_stride | sin_b_stride | sin_s_stride) % 8 == 0);",
    "const int work = (n_qh + 2 * n_kh) * (hd / 2 / (vec ? 8 : 1));",
    "const unsigned threads = (unsigned)(work >= 1024 ? 1024 : (work + 63) / 64 * 64);",
)


def dispatch_text_missing():
    """The quotes of ``DISPATCH_TEXT`` that csrc/norm_act.hip no longer holds (whitespace-insensitive)."""
    with open(HIP) as f:
        src = re.sub(r"\s+", "", f.read().replace("\\\n", ""))
    return [t for t in DISPATCH_TEXT if re.sub(r"\s+", "", t) not in src]


def norm_instance(n: int, aligned: bool = True):
    """``("cached", TPR, VPT)`` or ``("twopass", VEC)`` -- launch_skip_rmsnorm, norm_act.hip:132-148."""
    if n % 8 or not aligned:
        return ("twopass", 1)
    for nv_max, tpr, vpt in NORM_CACHED:
        if n // 8 <= nv_max:
            return ("cached", tpr, vpt)
    return ("twopass", 8)


def norm_rpb(n: int) -> int:
    """Rows per block of the instance ``n`` selects (``RPB = 256 / TPR``; the two-pass kernels take one row per block)."""
    inst = norm_instance(n)
    return 256 // inst[1] if inst[0] == "cached" else 1


def partials_instance(n: int, s: int):
    """``(VPT, SMAX)`` of skip_rmsnorm_partials_kernel -- norm_act.hip:246-249."""
    nv = n // 8
    return (1 if nv <= 256 else 2 if nv <= 512 else 4, 4 if s <= 4 else 6 if s <= 6 else 8 if s <= 8 else 12)


def slots_instance(n: int, k: int):
    """``(VPT, KMAX)`` of skip_rmsnorm_slots_kernel -- norm_act.hip:325-327."""
    nv = n // 8
    return (1 if nv <= 256 else 2 if nv <= 512 else 4, 2 if k <= 2 else 4 if k <= 4 else 8)


def grid_trips(rows: int, n: int, cap: int, aligned: bool = True):
    """``(VEC, blocks, trips)`` of the grid-stride kernels (swiglu / moe_sum: cap 4096, norm_act.hip:391-393, :498-500; activation
    with rows = 1: cap 8192, :452-454): ``trips`` is the largest number of loop iterations a thread runs."""
    vec = 8 if n % 8 == 0 and aligned else 1
    total = rows * (n // vec)
    blocks = min(-(-total // 256), cap)
    return vec, blocks, -(-total // (blocks * 256))


def rope_work(hq: int, hk: int, hd: int, vec: bool, cache: bool):
    """``(work items per token, trips)``: rope_kernel runs 256 threads (norm_act.hip:571), rope_cache_kernel
    ``min(1024, work rounded up to 64)`` over ``hq + 2 hk`` heads (:675-676)."""
    work = (hq + (2 if cache else 1) * hk) * (hd // 2 // (8 if vec else 1))
    threads = (1024 if work >= 1024 else -(-work // 64) * 64) if cache else 256
    return work, -(-work // threads)


# ------------------------------------------------------------------------------------------------------------------------------ #
# the cases of tests/test_rowops_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------ #
NORM_NS = (8, 128, 136, 256, 264, 512, 520, 2048, 2056, 4096, 4104, 8192, 8200, 65536, 300, 4103)
NORM_EPS = (1e-6, 1e-5)
PART_S = (1, 3, 4, 5, 6, 7, 8, 9, 11, 12)  # every load count (4, 6, 8, 12), one below it and one above it
SLOT_K = (1, 2, 3, 4, 5, 7, 8)  # load counts 2, 4, 8
PART_NS = (8, 2048, 2056, 4096, 4104, 8192)
PART_ROWS = (1, 3)
MOE_SUM_BIG = (129, 2, 65536)  # rows, k, n: rows * n / 8 = 1 056 768 vectors > 4096 * 256
SWIGLU_NS = (8, 256, 300, 5)
SWIGLU_BIG_VEC, SWIGLU_BIG_SCALAR = (129, 65536), (1025, 1027)
ACT_KINDS = ("relu", "leaky_relu", "tanh", "gelu")
ACT_NS = (7, 8, 257 * 3)
ACT_BIG_VEC, ACT_BIG_SCALAR = 2049 * 8192, 8192 * 256 + 257
ROPE_HDS = (2, 6, 16, 24, 32, 64, 128, 256)
ROPE_TOKENS = ((1, 1), (3, 5), (64, 1))
ROPE_TABLES = (F16, BF16, torch.float32)


def norm_rows(n: int):
    rpb = norm_rpb(n)
    return sorted({r for r in (1, rpb - 1, rpb, rpb + 1) if r > 0})


def rope_heads(hd: int):
    return {128: ((4, 2), (32, 8)), 24: ((4, 2), (28, 4))}.get(hd, ((4, 2),))


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def norm_inputs(kind: str, rows: int, n: int, dtype, seed: int = 0, with_res: bool = True):
    """``(x, r, w)`` on the CPU.  "randn": N(0, 1) rows, weight ``1 + 0.1 N(0, 1)``; "tiny" / "big": the rows scaled by 2**-12 /
    200, so that ``eps`` dominates the variance (2**-24 against 1e-6) or vanishes in it."""
    g = _gen(1000 * n + 10 * rows + seed)
    scale = {"randn": 1.0, "tiny": 2.0 ** -12, "big": 200.0}[kind]
    x = (torch.randn(rows, n, generator=g) * scale).to(dtype)
    r = (torch.randn(rows, n, generator=g) * scale).to(dtype) if with_res else None
    w = (1.0 + 0.1 * torch.randn(n, generator=g)).to(dtype)
    return x, r, w


def onehot_cols(n: int, aligned: bool = True):
    """Columns for the one-hot energy rows of width ``n``: the first and the last; the first and the last column of every vector index
    ``v < VPT`` (thread ``tr`` holds columns ``(v TPR + tr) 8 .. + 7``); both sides of every wave boundary inside the row (threads
    64, 128, 192 of a 256-thread row, for every ``v``).  Two-pass kernels (thread ``t`` takes items ``t, t + 256, ..``): the same
    around the wave and trip boundaries of the first and the last trip."""
    inst = norm_instance(n, aligned)
    cols = {0, n - 1}
    if inst[0] == "cached":
        _, tpr, vpt = inst
        for v in range(vpt):
            if v * tpr * 8 < n:
                cols |= {v * tpr * 8, min(n, (v + 1) * tpr * 8) - 1}
            for b in (64, 128, 192):
                c = (v * tpr + b) * 8
                if b < tpr and c < n:
                    cols |= {c - 1, c}
    else:
        vec = inst[1]
        trips = -(-(n // vec) // 256)
        for trip in {0, trips - 1}:
            for b in (0, 64, 128, 192, 256):
                c = (trip * 256 + b) * vec
                if 0 < c < n:
                    cols |= {c - 1, c}
    return sorted(cols)


def onehot_inputs(n: int, dtype, with_res: bool = True, aligned: bool = True):
    """One row per column of ``onehot_cols``: ``s = x + r`` is 1.0 there (0.5 + 0.5 with a residual) and 0 elsewhere, so
    ``var = 1 / n`` and ``y = sqrt(n) w`` at the column -- and about ``w / sqrt(eps)`` if the column is lost from the sum."""
    cols = onehot_cols(n, aligned)
    x = torch.zeros(len(cols), n, dtype=dtype)
    x[torch.arange(len(cols)), torch.tensor(cols)] = 0.5 if with_res else 1.0
    w = (1.0 + 0.1 * torch.randn(n, generator=_gen(n))).to(dtype)
    return x, (x.clone() if with_res else None), w


def plane_inputs(s: int, rows: int, n: int, dtype, seed: int = 0):
    """``(planes fp32 [s, rows, n], r, w)``: independent N(0, 1) planes -- a dropped or doubled plane moves ``x`` by order 1."""
    g = _gen(100000 * s + 10 * n + rows + seed)
    p = torch.randn(s, rows, n, generator=g)
    r = torch.randn(rows, n, generator=g).to(dtype)
    w = (1.0 + 0.1 * torch.randn(n, generator=g)).to(dtype)
    return p, r, w


def slot_inputs(k: int, rows: int, n: int, dtype, seed: int = 0):
    """``(slots [rows, k, n] in dtype, r, w)``."""
    p, r, w = plane_inputs(k, rows, n, dtype, seed + 7)
    return p.permute(1, 0, 2).contiguous().to(dtype), r, w


def swiglu_edges(dtype):
    """``(g, u)`` 1-D: every gate edge paired with every u of {+-1, +-65504}: g = +-0, +-2**-14, +-11, +-30, +-88, +-65504 and, for
    bf16, +-1e30 (all rounded to ``dtype``; 65504 is 65536 in bf16)."""
    gs = [0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 11.0, -11.0, 30.0, -30.0, 88.0, -88.0, 65504.0, -65504.0]
    if dtype == BF16:
        gs += [1e30, -1e30]
    us = [1.0, -1.0, 65504.0, -65504.0]
    g = torch.tensor([a for a in gs for _ in us], dtype=torch.float64).to(dtype)
    u = torch.tensor([b for _ in gs for b in us], dtype=torch.float64).to(dtype)
    return g, u


def swiglu_inputs(kind: str, rows: int, n: int, dtype, seed: int = 0):
    """``(g, u)`` [rows, n]: "randn": 3 N(0, 1); "edges": ``swiglu_edges`` repeated over the shape."""
    if kind == "randn":
        gen = _gen(31 * n + rows + seed)
        return (torch.randn(rows, n, generator=gen) * 3).to(dtype), (torch.randn(rows, n, generator=gen) * 3).to(dtype)
    g, u = swiglu_edges(dtype)
    idx = torch.arange(rows * n) % g.numel()
    return g[idx].reshape(rows, n), u[idx].reshape(rows, n)


def swiglu_edge_rows(n: int, dtype) -> int:
    return -(-swiglu_edges(dtype)[0].numel() // n)


def act_inputs(numel: int, dtype, device=None):
    """+-12 densely (an even ladder rounded to ``dtype``), with +0 and -0 at the ends and 0 in the middle when there is room."""
    x = torch.linspace(-12.0, 12.0, numel, dtype=torch.float64, device=device).to(dtype)
    if numel >= 3:
        x[0], x[-1], x[numel // 2] = 0.0, -0.0, 0.0
    return x


def rope_inputs(bs: int, sl: int, hq: int, hk: int, hd: int, dtype, table_dtype, width: int, seed: int = 0, rows=None):
    """``(q [N, hq, hd], k [N, hk, hd], cos, sin)``: N(0, 1) heads; tables ``[bs, sl, width]`` (or ``[rows, width]`` for the
    position-indexed form) of cos / sin of independent uniform angles -- a distinct row per token and no structure that a wrong row
    or column could share; columns past ``hd / 2`` hold other angles and must not be read."""
    g = _gen(7919 * hd + 31 * hq + bs * sl + seed)
    n = bs * sl
    q = torch.randn(n, hq, hd, generator=g).to(dtype)
    k = torch.randn(n, hk, hd, generator=g).to(dtype)
    shape = (bs, sl, width) if rows is None else (rows, width)
    ang = torch.rand(shape, generator=g, dtype=torch.float64) * (2 * math.pi)
    return q, k, ang.cos().to(table_dtype), ang.sin().to(table_dtype)


# ------------------------------------------------------------------------------------------------------------------------------ #
# references -> brackets
# ------------------------------------------------------------------------------------------------------------------------------ #
def seq_sum32(parts: torch.Tensor, dim: int) -> torch.Tensor:
    """The kernels' fp32 sum over planes / slots: ``0.f + p[0] + p[1] + ..`` in order, every add rounded to fp32."""
    acc = torch.zeros_like(parts.select(dim, 0), dtype=torch.float32)
    for i in range(parts.shape[dim]):
        acc = acc + parts.select(dim, i).float()
    return acc


def sum_bracket(parts: torch.Tensor, dim: int, dtype):
    """``storage(sum)`` over planes / slots: the fp32 sum narrowed; with a single plane or slot the sum is that value itself."""
    a = seq_sum32(parts, dim).to(dtype)
    return a, a


def residual_bracket(x: torch.Tensor, r: torch.Tensor):
    """``r_out = storage(x + r)``: the fp32 sum narrowed, or the exact sum rounded once."""
    return candidates((x.float() + r.float()).to(x.dtype), to_storage(x.double() + r.double(), x.dtype))


def norm_brackets(x: torch.Tensor, r, w: torch.Tensor, eps: float):
    """``((y_lo, y_hi), (r_lo, r_hi) | None)`` of skip_rmsnorm on 16-bit ``x [rows, n]``, ``r`` (or None), ``w [n]``."""
    dtype = x.dtype
    s32 = x.float() + r.float() if r is not None else x.float()
    s = s32.double()
    var = (s * s).sum(-1, keepdim=True) / x.shape[-1]
    eps32 = float(torch.tensor(eps, dtype=torch.float32))  # the kernel receives eps as an fp32 argument
    t = s / torch.sqrt(var + eps32)
    t1, t2 = t * (1.0 - NORM_DELTA), t * (1.0 + NORM_DELTA)
    a_lo, a_hi = to_storage(torch.minimum(t1, t2), dtype), to_storage(torch.maximum(t1, t2), dtype)
    wd = w.double()
    y = candidates(to_storage(a_lo.double() * wd, dtype), to_storage(a_hi.double() * wd, dtype))
    return y, (residual_bracket(x, r) if r is not None else None)


def partials_brackets(parts: torch.Tensor, dim: int, r: torch.Tensor, w: torch.Tensor, eps: float):
    """skip_rmsnorm_partials: ``x = storage(fp32 sum)`` (one candidate), then ``norm_brackets(x, r, w)``."""
    return norm_brackets(seq_sum32(parts, dim).to(r.dtype), r, w, eps)


def swiglu_bracket(g: torch.Tensor, u: torch.Tensor):
    gd, ud = g.double(), u.double()
    sig = torch.sigmoid(gd)
    ref = gd * sig * ud
    return bracket(ref, torch.where(sig < FP32_MIN_NORMAL, ref.abs(), SWIGLU_REL * ref.abs()), g.dtype)


def act_bracket(x: torch.Tensor, kind: str):
    xd = x.double()
    if kind == "relu":  # max(0, x); a NaN stays (the kernel keeps its bit pattern)
        y = torch.where(xd > 0, x, torch.zeros_like(x))
        y = torch.where(torch.isnan(x), x, y)
        return y, y
    if kind == "leaky_relu":  # x >= 0 ? x : storage(storage(0.01) * x): an exact fp32 product, one rounding
        slope = torch.tensor(0.01, dtype=torch.float32).to(x.dtype).double()
        y = torch.where(xd >= 0, x, to_storage(slope * xd, x.dtype))
        return y, y
    if kind == "tanh":
        ref = torch.tanh(xd)
        return bracket(ref, TANH_REL * ref.abs() + TANH_ABS, x.dtype)
    ref = xd * 0.5 * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    return bracket(ref, GELU_REL * ref.abs() + GELU_ABS * xd.abs(), x.dtype)


def _table_rows(t: torch.Tensor, half: int, token_rows=None) -> torch.Tensor:
    """``[N, 1, half]``: the table row of every token (``token_rows`` = positions for a position-indexed table)."""
    t = t.reshape(-1, t.shape[-1]) if token_rows is None else t[token_rows.long()]
    return t[:, None, :half]


def rope_bracket(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, token_rows=None, sin_sign: float = 1.0):
    """``(lo, hi)`` of the rotated heads ``x [N, H, hd]`` (token i reads row i of the flattened table, or row ``token_rows[i]``)."""
    half = x.shape[-1] // 2
    c, s = _table_rows(cos, half, token_rows), _table_rows(sin, half, token_rows) * sin_sign
    a, b = x[..., :half], x[..., half:]
    ad, bd, cd, sd = a.double(), b.double(), c.double(), s.double()
    ref = torch.cat([ad * cd - bd * sd, bd * cd + ad * sd], -1)
    if cos.dtype == torch.float32:
        mag = torch.cat([(ad * cd).abs() + (bd * sd).abs(), (bd * cd).abs() + (ad * sd).abs()], -1)
        return bracket(ref, ROPE_REL * ref.abs() + ROPE_ABS * mag, x.dtype)
    af, bf, cf, sf = a.float(), b.float(), c.float(), s.float()
    via32 = torch.cat([af * cf - bf * sf, bf * cf + af * sf], -1).to(x.dtype)
    return candidates(via32, to_storage(ref, x.dtype))


# ------------------------------------------------------------------------------------------------------------------------------ #
# the kernels restated in fp32 (torch CPU / device arithmetic, any summation order), correct or with ONE fault -- for the CPU tests
# ------------------------------------------------------------------------------------------------------------------------------ #
NORM_FAULTS = ("drop8", "eps_outside", "w_first")
SUM_FAULTS = ("plane0_twice", "drop_last", "drop_first")


def kernel_sum32(parts: torch.Tensor, dim: int, fault=None) -> torch.Tensor:
    acc = seq_sum32(parts, dim)
    if fault == "plane0_twice":
        acc = acc + parts.select(dim, 0).float()
    elif fault == "drop_last":
        acc = seq_sum32(parts.narrow(dim, 0, parts.shape[dim] - 1), dim) if parts.shape[dim] > 1 else torch.zeros_like(acc)
    elif fault == "drop_first":
        acc = seq_sum32(parts.narrow(dim, 1, parts.shape[dim] - 1), dim) if parts.shape[dim] > 1 else torch.zeros_like(acc)
    return acc


def kernel_norm32(x, r, w, eps, fault=None, drop_at=None):
    """``(y, r_out)`` the way the kernels compute them, in fp32.  Faults: "drop8": one vector of 8 columns (the last, or the one
    holding column ``drop_at``) missing from the sum of squares; "eps_outside": ``1 / (sqrt(var) + eps)``; "w_first": the weight
    multiplied before the first rounding, ``storage(s * rrms * w)``."""
    dtype, n = x.dtype, x.shape[-1]
    s = x.float() + r.float() if r is not None else x.float()
    terms = s * s / float(n)
    if fault == "drop8":
        c0 = (n - 1 if drop_at is None else drop_at) // 8 * 8
        terms = terms.clone()
        terms[:, c0:c0 + 8] = 0.0
    var = terms.sum(-1, keepdim=True)
    e = torch.tensor(eps, dtype=torch.float32)
    rrms = 1.0 / (torch.sqrt(var) + e) if fault == "eps_outside" else 1.0 / torch.sqrt(var + e)
    if fault == "w_first":
        y = (s * rrms * w.float()).to(dtype)
    else:
        y = ((s * rrms).to(dtype).float() * w.float()).to(dtype)
    return y, (s.to(dtype) if r is not None else None)


def kernel_swiglu32(g, u):
    gf = g.float()
    return (gf * torch.sigmoid(gf) * u.float()).to(g.dtype)


def kernel_act32(x, kind):
    xf = x.float()
    if kind == "relu":
        return torch.where(torch.isnan(x), x, torch.where(xf > 0, xf, torch.zeros_like(xf)).to(x.dtype))
    if kind == "leaky_relu":
        return torch.where(xf >= 0, x, (torch.tensor(0.01).to(x.dtype).float() * xf).to(x.dtype))
    if kind == "tanh":
        return (2.0 / (1.0 + torch.exp(-2.0 * xf)) - 1.0).to(x.dtype)
    return (xf * 0.5 * (1.0 + torch.erf(xf * 0.70710678118654752440))).to(x.dtype)


def kernel_rope32(x, cos, sin, token_rows=None, fault=None):
    """The rotation in fp32.  Faults: "sin_sign": the sign of sin flipped; "wrong_row": every token reads the next token's row."""
    half = x.shape[-1] // 2
    c, s = _table_rows(cos, half, token_rows).float(), _table_rows(sin, half, token_rows).float()
    if fault == "sin_sign":
        s = -s
    if fault == "wrong_row":
        c, s = c.roll(1, 0), s.roll(1, 0)
    a, b = x[..., :half].float(), x[..., half:].float()
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(x.dtype)
