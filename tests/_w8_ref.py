"""TEST INFRASTRUCTURE ONLY -- the arithmetic of the three engines behind ``w8a16_matmul`` (fp8-e4m3 block-scaled, int8 per-channel,
int8 group-wise weights under fp16 activations) in exact form, the reference's own meaning of the same weights, and the largest
distance a correct engine can keep from it.  Plain torch, device-agnostic (the GPU tests run it on the device,
``tests/test_w8_ref_cpu.py`` checks it on the CPU); nothing here calls a kernel of the project.  The float64 product, the derived
error bound of a sum and the input builders are those of ``tests/_w4_ref.py``, imported.

What the engines compute -- csrc/gemm_w8_common.h::d8_fp8 / d8_i8 (skinny and M-tiled engines) and csrc/gemm_wq.hip::dequant_fp8 /
dequant_i8 (generic engine) are the same instruction sequences, so ONE definition describes all three:

* the code is widened EXACTLY to fp16.  int8: the byte's integer value.  fp8 e4m3: the reference's bit surgery
  (w8a16.py:48-62, ``oracle.fp8e4m3_bits_to_fp16``) ``bits = ((b & 0x80) << 8) | ((b & 0x7F) << 7)`` -- the e4m3 value / 256, the
  e4m3 subnormals landing on fp16 subnormals, and the two NaN encodings 0x7F / 0xFF on +-480 / 256 (finite: no code is a NaN
  under this definition, in the reference or here);
* the multiplier is the block's fp32 scale narrowed once to fp16, to nearest even with subnormals kept: ``fp16(s)`` for int8,
  ``fp16(fp32(s * 256))`` for fp8 (the fp32 product by a power of two is exact short of overflow);
* ONE fp16 multiply ``w = widened * multiplier``, rounded to nearest even with subnormals kept;
* the block of weight ``[n, k]`` is ``scales[n // group_n, k // group_k]`` with ``group_k`` clamped to K, partial last groups in
  both directions;
* ``y[m, n] = fp16(sum_k x[m, k] * w[n, k] (+ bias[n]))``: exact fp16 x fp16 products, fp32 accumulation in an order the engine
  chooses, the bias added in fp32, one rounding to fp16 (split-K planes: the fp32 sums themselves, no bias).
"""

from __future__ import annotations

import torch

from tests._w4_ref import (abs_sum64, assert_bound_bites, assert_within, bound, one_hot_starts, ref64,  # noqa: F401  (re-exported)
                           sparse_int_rows, worst_ratio)

SCALE_CHOICES = (0.25, 0.5, 1.0, 2.0, 4.0)
MIN_NORMAL16 = 2.0 ** -14

# ------------------------------------------------------------------------------------------------------------------------------ #
# The shapes of tests/test_w8a16_engines_gpu.py (N, K), worked out by hand from gemm_w8_skinny.hip::d8_splits, with the engine a
# call of M <= 64 / M > 64 rows must take and the split-K planes a skinny launch leaves; tests/test_w8_ref_cpu.py checks the same
# table against the host-side route query, so both files fail when the dispatch is retuned.
# ------------------------------------------------------------------------------------------------------------------------------ #
SHAPES = {"S1": (132, 128), "S2": (256, 640), "S3": (388, 1152), "S4": (128, 2560), "G1": (130, 384), "G2": (256, 336),
          "T1": (160, 1152), "T2": (130, 384)}
SKINNY_PLANES = {"S1": 1, "S2": 2, "S3": 3, "S4": 10, "T1": 3}  # chunks 1, 5 (3 + 2), 9, 20, 9
DECODE_MS = (1, 17, 32, 33, 64)
# (format, group_n, group_k); group_k None = per output channel (one scale per row, group_k = K)
FORMATS = (("fp8", 128, 128), ("fp8", 64, 256), ("int8", 1, None), ("int8", 1, 128), ("int8", 1, 256))


def want_engine(tag: str, m: int) -> str:
    """The engine the table expects for a contiguous call of ``m`` rows at shape ``tag``."""
    n, k = SHAPES[tag]
    if m > 64:
        return "mtiled" if n % 32 == 0 and k % 64 == 0 else "generic"
    return "skinny" if n % 4 == 0 and k % 128 == 0 else "generic"


def formats_for(tag: str):
    """The formats of a shape: every ``group_k <= K`` (``group_k == K`` is one k-group; 256 is left out at K = 128), a group-wise
    format that coincides with the per-channel one (K = 128) listed once."""
    k = SHAPES[tag][1]
    out = []
    for f, gn, gk in FORMATS:
        c = (f, gn, k if gk is None else gk)
        if c[2] <= k and c not in out:
            out.append(c)
    return out


def skinny_planes(partial_words: int, n: int, k: int) -> int:
    """Split-K planes a skinny-engine launch leaves for its finish pass, derived on the host the way the launch does from
    ``partial_words = ll_dense8_partial_words(1, n, k)``: ``s = words / n`` wanted splits, ``cps = ceil(chunks / s)`` 128-k chunks per
    split, ``ceil(chunks / cps)`` planes.  0 for a shape the engine does not take."""
    if partial_words == 0:
        return 0
    s, chunks = partial_words // n, k // 128
    cps = -(-chunks // s)
    return -(-chunks // cps)


def streaming_planes(n: int, k: int, cap: int) -> int:
    """Planes of a partial-mode launch of the streaming engine (``dense8_kernel``) under a cap: ``d8_splits`` restated -- about three
    workgroups per CU over the 128-row tiles, at least two chunks per split, at most ``cap`` -- then the same ``cps`` rule."""
    chunks, tiles = k // 128, -(-n // 128)
    s = max(1, min(-(-768 // tiles), chunks // 2, cap))
    cps = -(-chunks // s)
    return -(-chunks // cps)


def bounded_cases():
    """``(tag, format, group_n, group_k, rows)`` of every checkpoint-scale case the GPU tests hold to the derived bound."""
    out = []
    for tag in ("S1", "S2", "S3", "G1", "G2", "T1", "T2"):
        ms = {"T1": (65, 129, 200), "T2": (100,)}.get(tag, DECODE_MS)
        out += [(tag, f, gn, gk, ms) for f, gn, gk in formats_for(tag)]
    return out


# Partial mode (``dense_matmul_partials``) takes any group_k that is a multiple of 64: 64 and 192 put the two 64-k halves of a 128-k
# chunk into different scale groups, which no group_k the finished entry accepts (multiples of 128, or K) can.
PARTIAL_CASES = (("S2", "fp8", 128, 128), ("S2", "int8", 1, 256), ("S3", "fp8", 64, 256), ("S3", "int8", 1, 1152),
                 ("S2", "fp8", 128, 64), ("S2", "int8", 1, 192), ("S3", "fp8", 64, 192), ("S3", "int8", 1, 64))


def case_seed(tag: str, fmt: str, gn: int, gk: int) -> int:
    return 1000 * sorted(SHAPES).index(tag) + 100 * (fmt == "fp8") + gn + gk


# ------------------------------------------------------------------------------------------------------------------------------ #
# the engines' dequantisation, the reference's, and the distance between them
# ------------------------------------------------------------------------------------------------------------------------------ #
def expand_scales(scales: torch.Tensor, n: int, k: int, group_n: int, group_k: int) -> torch.Tensor:
    """``[ceil(N / group_n), ceil(K / group_k)]`` (or 1-D per row) block scales -> ``[N, K]`` fp32, partial last groups in both
    directions; ``group_k`` is clamped to K like the entry point does."""
    s = scales.float()
    if s.dim() == 1:
        s = s.unsqueeze(-1)
    gk = min(int(group_k), k)
    assert s.shape == (-(-n // group_n), -(-k // gk)), (tuple(s.shape), n, k, group_n, gk)
    rows = torch.arange(n, device=s.device) // group_n
    cols = torch.arange(k, device=s.device) // gk
    return s[rows][:, cols]


def widen_fp8(codes_u8: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> fp16 holding value / 256, exactly (``oracle.fp8e4m3_bits_to_fp16`` on any device)."""
    b = codes_u8.to(torch.int32)
    bits = ((b & 0x80) << 8) | ((b & 0x7F) << 7)
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16)


def _round16(v64: torch.Tensor) -> torch.Tensor:
    """One rounding of an exact float64 product to fp16.  The product of two fp16 values has at most 22 significant bits and an
    exponent far inside fp32's range, so the narrowing through fp32 is exact and ``.half()`` rounds once (to nearest even,
    subnormals kept)."""
    assert bool((v64.float().double() == v64).all())
    return v64.float().half()


def dequant16_fp8(codes_u8: torch.Tensor, scales: torch.Tensor, group_n: int, group_k: int) -> torch.Tensor:
    """The ``[N, K]`` fp16 weights exactly as the engines define them for fp8 codes: ``fp16(widened * fp16(fp32(s * 256)))``.  The
    product is evaluated in float64, where an 11 x 11-bit product is exact, and rounded once."""
    n, k = codes_u8.shape
    mult = (expand_scales(scales, n, k, group_n, group_k) * 256.0).half()
    return _round16(widen_fp8(codes_u8).double() * mult.double())


def dequant16_int8(codes_i8: torch.Tensor, scales: torch.Tensor, group_n: int, group_k: int) -> torch.Tensor:
    """The same for int8 codes: ``fp16(code * fp16(s))``, an 8 x 11-bit product, rounded once."""
    n, k = codes_i8.shape
    mult = expand_scales(scales, n, k, group_n, group_k).half()
    return _round16(codes_i8.double() * mult.double())


def dequant16(fmt: str, codes: torch.Tensor, scales: torch.Tensor, group_n: int, group_k: int) -> torch.Tensor:
    return (dequant16_fp8 if fmt == "fp8" else dequant16_int8)(codes, scales, group_n, group_k)


def code_values64(fmt: str, codes: torch.Tensor) -> torch.Tensor:
    """``value(code)`` in float64: the integer for int8; for fp8 the widened pattern times 256 (every finite e4m3 value exactly, and
    +-480 for the two NaN encodings, which is what the reference's bit surgery makes of them)."""
    return widen_fp8(codes).double() * 256.0 if fmt == "fp8" else codes.double()


def true64(fmt: str, codes: torch.Tensor, scales: torch.Tensor, group_n: int, group_k: int) -> torch.Tensor:
    """The reference's own meaning of the weights (w8a16.py: the scale applied in fp32 to the sums of a block):
    ``value(code) * s`` in float64 with the fp32 scale unrounded."""
    n, k = codes.shape
    return code_values64(fmt, codes) * expand_scales(scales, n, k, group_n, group_k).double()


def semantic_bound(t64: torch.Tensor) -> torch.Tensor:
    """The largest ``|dequant16 - true64|`` a correct engine can show, elementwise: ``|w| (2**-10 + 2**-22) + 2**-25``.

    Two roundings to fp16 separate the two: of the multiplier (relative ``2**-11``) and of the product (relative ``2**-11``, or
    half the subnormal spacing ``2**-25`` absolute where the product falls below ``2**-14``): ``(1 + 2**-11)**2 - 1 = 2**-10 + 2**-22``.

    Valid while the fp16 multiplier is a NORMAL number and the product is finite:
      fp8   ``s * 256 >= 2**-14`` (s >= 2**-22, 2.4e-7),
      int8  ``s >= 2**-14`` (6.1e-5; a per-channel scale ``amax / 127`` leaves the range when ``amax < 7.75e-3``),
      both  ``|w| < 65504``.
    Below the range the multiplier is an fp16 subnormal: its absolute error stays ``2**-25`` while it shrinks, so the weight's
    relative error grows like ``2**-25 / multiplier`` (0.3 % at s = 1e-5 for int8; a multiplier below ``2**-25`` is zero).  The
    engines keep that arithmetic -- ``dequant16`` restates it, and the bit-exact tests hold them to it -- but this bound no
    longer applies; ``supported_scale`` says where."""
    return t64.abs() * (2.0 ** -10 + 2.0 ** -22) + 2.0 ** -25


def multiplier64(fmt: str, scales: torch.Tensor) -> torch.Tensor:
    """The fp32 value the engines narrow to fp16: ``s`` (int8) or ``fp32(s * 256)`` (fp8), in float64."""
    s = scales.float()
    return (s * 256.0 if fmt == "fp8" else s).double()


def supported_scale(fmt: str, scales: torch.Tensor) -> torch.Tensor:
    """Elementwise: the scale's fp16 multiplier is a normal number (``semantic_bound`` applies to the weights of its block)."""
    m = multiplier64(fmt, scales).abs()
    return (m >= MIN_NORMAL16) & (m < 65504.0)


def one_hot_wrapped(m: int, k: int, k0: int, device=None) -> torch.Tensor:
    """fp16 ``[m, k]``: row ``i`` is the unit vector of position ``(k0 + i) mod k`` (``_w4_ref.one_hot_rows`` with the rows wrapping
    inside K: more rows than K has left, or more rows than a chunk)."""
    x = torch.zeros(m, k, dtype=torch.float16, device=device)
    i = torch.arange(m, device=device)
    x[i, (k0 + i) % k] = 1.0
    return x


def one_hot_starts8(m: int, k: int):
    """The ``k0`` values of a one-hot sweep with ``m`` wrapping rows: every k position for m = 32, m = 64 and the prefill batches
    (steps of ``m``); otherwise the first and the last k of every 128-chunk, the last chunk as short as K leaves it
    (``_w4_ref.one_hot_starts`` for a K that is a multiple of 128)."""
    if m in (32, 64) or m > 64:
        return list(range(0, k, m))
    if k % 128 == 0:
        return one_hot_starts(m, k)
    return sorted({c for c0 in range(0, k, 128) for c in (c0, min(c0 + 128, k) - m)})


# ------------------------------------------------------------------------------------------------------------------------------ #
# generators (CPU tensors; a fixed seed per case)
# ------------------------------------------------------------------------------------------------------------------------------ #
def _grid(n: int, k: int, group_n: int, group_k: int):
    return -(-n // group_n), -(-k // min(group_k, k))


def exact_case8(fmt: str, n: int, k: int, group_n: int, group_k: int, seed: int, codes: str = "all"):
    """``(codes, scales, bias)`` on which the scale is exact: random codes, per block a scale from {0.25, 0.5, 1, 2, 4}, an
    integer-valued fp16 bias in -8..8.  int8: the full range -128..127.  fp8, ``codes="all"``: all 256 byte values (the one-hot
    tests); ``codes="sum"``: only codes with ``1 <= |value| <= 448`` -- ``0x38 <= (code & 0x7F) <= 0x7E``, no subnormals, no NaN
    encodings -- whose values are multiples of 2**-3, so that every product with a {+-1, +-2} activation is a multiple of 2**-5
    (int8: of 2**-2).  ``dequant16`` equals ``value(code) * s`` outright on either."""
    g = torch.Generator().manual_seed(seed)
    if fmt == "int8":
        q = torch.randint(-128, 128, (n, k), generator=g).to(torch.int8)
    elif codes == "all":
        q = torch.randint(0, 256, (n, k), generator=g).to(torch.uint8)
    else:
        mag = torch.randint(0x38, 0x7F, (n, k), generator=g)
        q = (mag | (torch.randint(0, 2, (n, k), generator=g) << 7)).to(torch.uint8)
    sc = torch.tensor(SCALE_CHOICES)[torch.randint(0, len(SCALE_CHOICES), _grid(n, k, group_n, group_k), generator=g)]
    bias = torch.randint(-8, 9, (n,), generator=g).half()
    return q, sc, bias


def sum_quantum(fmt: str) -> float:
    """The common divisor of every term of the exact-sum tests (``exact_case8(..., codes="sum")`` times {+-1, +-2}, integer bias)."""
    return 2.0 ** -5 if fmt == "fp8" else 2.0 ** -2


def _block_amax(w: torch.Tensor, group_n: int, group_k: int) -> torch.Tensor:
    n, k = w.shape
    nb, kb = _grid(n, k, group_n, group_k)
    gk = min(group_k, k)
    pad = torch.zeros(nb * group_n, kb * gk)
    pad[:n, :k] = w.abs()
    return pad.reshape(nb, group_n, kb, gk).amax(dim=(1, 3))


def checkpoint_case8(fmt: str, m: int, n: int, k: int, group_n: int, group_k: int, seed: int, spread: str = "mild"):
    """``(x, codes, scales, bias)`` quantised the way a checkpoint is: ``x ~ 0.5 N(0, 1)`` fp16, weights ``~ 0.02 N(0, 1)`` times a
    per-row magnitude, bias ``~ 0.1 N(0, 1)`` fp16.  fp8: block scale ``amax / 448``, codes ``(w / s).to(float8_e4m3fn)``; int8:
    ``amax / 127`` per row and k-group, round, clamp +-127 (a block of zeros takes scale 1).

    ``spread="mild"``: row magnitudes log-uniform within a factor of 3 of each other (``3**(u - 0.5)``) -- the bounded tests: a wide
    spread lets the largest output's bound approach the rms of one product, and ``assert_bound_bites`` would stop biting.
    ``spread="subnormal"``: log-uniform over ``10**(-1.6 u)``, row amax from ~0.07 down to ~2e-3 -- every int8 scale of a row with
    ``amax < 7.75e-3`` is an fp16 subnormal, and a good share of both formats' weights are fp16 subnormals (one-hot tests only)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(m, k, generator=g) * 0.5).half()
    u = torch.rand(n, generator=g)
    mag = 3.0 ** (u - 0.5) if spread == "mild" else 10.0 ** (-1.6 * u)
    w = torch.randn(n, k, generator=g) * 0.02 * mag[:, None]
    bias = (torch.randn(n, generator=g) * 0.1).half()
    amax = _block_amax(w, group_n, group_k)
    sc = amax / (448.0 if fmt == "fp8" else 127.0)
    sc = torch.where(sc > 0, sc, torch.ones_like(sc))
    ws = w / expand_scales(sc, n, k, group_n, group_k)
    if fmt == "fp8":
        q = ws.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        q = ws.round().clamp(-127, 127).to(torch.int8)
    return x, q, sc, bias
