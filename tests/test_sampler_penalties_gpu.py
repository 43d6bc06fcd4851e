"""``ll_logit_penalties`` and ``ll_seeded_uniform`` (csrc/sampler_penalties.hip) against tests/_penalties_ref.py.

Exact cases: logits and biases are multiples of 1/8 with magnitude below 16 (below 2 where the output is bf16), r in {1, 2},
f in {0, 0.25}, p in {0, 0.5} and counts up to 8, so every intermediate and the result are multiples of 1/16 that fp32 and the
output dtype hold exactly (the test checks that of its own reference): neither a fused multiply-add nor a rounding can
excuse a mismatch, and the comparison is ``torch.equal``."""

import itertools

import pytest
import torch

from lite_llama_amd.sampling import LogitBias, apply_penalties, apply_repetition_penalty, seeded_uniform
from tests import _penalties_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
PAIRS = [(F16, F16), (F16, F32), (BF16, BF16), (BF16, F32), (F32, F32)]
VOCABS = [1, 7, 8191, 8192, 8193, 16385, 152064]
SPANS = [0, 1, 257, 1025]
B = 3
MAX_COUNT = 8
COMBOS = list(itertools.product((1.0, 2.0), (0.0, 0.5), (0.0, 0.25)))  # (r, p, f)


def _edges(vocab):
    """Token 0, token ``vocab - 1`` and the first and last token of every 4096-token chunk (which covers every 8192-token
    one): wherever a workgroup's range begins or ends."""
    e = {0, vocab - 1}
    for lo in range(4096, vocab, 4096):
        e.update((lo - 1, lo))
    return sorted(e)


def _exact_case(vocab, span, in_dtype, out_dtype, seed, stride_pad=0):
    """Logits ``[B, vocab]`` (row stride ``vocab + stride_pad``), a span with the edge tokens, duplicates, masked-out
    duplicates and out-of-range ids in it (no token masked in more than MAX_COUNT times), and per-row biases: row 0 names
    the edges and random tokens, with -inf on a token its span repeats; row 1 names nothing; row 2 names random tokens."""
    g = torch.Generator().manual_seed(seed)
    top = 15 if out_dtype == BF16 else 127
    store = torch.zeros(B, vocab + stride_pad, dtype=in_dtype)
    store[:, :vocab] = (torch.randint(-top, top + 1, (B, vocab), generator=g).double() / 8).to(in_dtype)
    logits = store.to(DEV)[:, :vocab]
    edges = _edges(vocab)
    ids = torch.zeros(B, span, dtype=torch.int64)
    mask = torch.zeros(B, span, dtype=torch.bool)
    junk = [-1, vocab, vocab + 5, 1 << 40, -(1 << 40)]
    for i in range(B):
        pool = edges + junk + torch.randint(0, vocab, (max(span // 4, 1),), generator=g).tolist()
        pick = torch.randint(0, len(pool), (span,), generator=g).tolist()
        row = [pool[j] for j in pick]
        for j, e in enumerate(edges[:span]):   # every edge at least once while the span has room
            row[j] = e
        seen = {}
        for j, tok in enumerate(row):
            on = seen.get(tok, 0) < MAX_COUNT and (j < len(edges) or j % 5 != 0)
            if on:
                seen[tok] = seen.get(tok, 0) + 1
            ids[i, j], mask[i, j] = tok, on
    eighths = lambda n: (torch.randint(-top, top + 1, (n,), generator=g).double() / 8).tolist()
    rand_toks = lambda n: torch.randint(0, vocab, (n,), generator=g).tolist()
    row0 = dict(zip(edges + rand_toks(16), eighths(len(edges) + 16)))
    row0[0] = float("-inf")                    # token 0 opens every row's span (span >= 1)
    row2 = dict(zip(rand_toks(5), eighths(5)))
    return logits, ids.to(DEV), mask.to(DEV), [row0, None, row2]


def _assert_exact(out, ref, out_dtype, what):
    assert out.dtype == out_dtype, what
    want = ref.to(out_dtype)
    assert torch.equal(want.double(), ref), f"{what}: the test's own data is not representable in {out_dtype}"
    assert torch.equal(out.cpu(), want), what


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("vocab", VOCABS)
def test_exact_on_representable_data(vocab, span, pair):
    """Every (r, p, f) as scalars where the dtype stays, and as per-row tensors with different values per row (which promote
    16-bit logits to fp32), with and without the bias."""
    in_dtype, out_dtype = pair
    logits, ids, mask, bias = _exact_case(vocab, span, in_dtype, out_dtype, seed=vocab * 31 + span)
    built = LogitBias(bias, B, vocab, DEV)
    if in_dtype == out_dtype:
        for r, p, f in COMBOS:
            for lb in (None, built):
                ref, counts, _ = R.penalties_ref(logits, ids, mask, r, p, f, None if lb is None else bias)
                assert counts.max() <= MAX_COUNT
                _assert_exact(apply_penalties(logits, ids, mask, r, p, f, lb), ref, out_dtype, (r, p, f, lb is not None))
    if out_dtype == F32:
        for shift in range(3):
            rows = [COMBOS[(3 * i + shift * 3 + 1) % len(COMBOS)] for i in range(B)]
            r, p, f = ([c[k] for c in rows] for k in range(3))
            t = lambda v: torch.tensor(v, dtype=F32, device=DEV)
            for lb in (None, built):
                ref, _, _ = R.penalties_ref(logits, ids, mask, r, p, f, None if lb is None else bias)
                _assert_exact(apply_penalties(logits, ids, mask, t(r), t(p).view(B, 1), t(f), lb), ref, F32, (rows, lb is not None))
                # one tensor among scalars promotes too
                ref, _, _ = R.penalties_ref(logits, ids, mask, 2.0, p, 0.25, None if lb is None else bias)
                _assert_exact(apply_penalties(logits, ids, mask, 2.0, t(p), 0.25, lb), ref, F32, ("mixed", rows))


@pytest.mark.parametrize("pair", [(F16, F16), (BF16, F32), (F32, F32)], ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("vocab", VOCABS)
def test_exact_with_a_row_stride_beyond_the_vocabulary(vocab, pair):
    """Rows ``vocab + 5`` elements apart: no row but the first starts on a 16-byte boundary."""
    in_dtype, out_dtype = pair
    logits, ids, mask, bias = _exact_case(vocab, 257, in_dtype, out_dtype, seed=vocab + 7, stride_pad=5)
    assert logits.stride(0) == vocab + 5
    pen = (lambda v: v) if in_dtype == out_dtype else (lambda v: torch.full((B,), v, dtype=F32, device=DEV))
    ref, _, _ = R.penalties_ref(logits, ids, mask, 2.0, 0.5, 0.25, bias)
    _assert_exact(apply_penalties(logits, ids, mask, pen(2.0), pen(0.5), pen(0.25), bias), ref, out_dtype, "padded")


@pytest.mark.parametrize("vocab", VOCABS)
def test_one_token_fills_the_whole_span(vocab):
    """1025 masked-in copies of the last token: count 1025, f = 0.25 -- exact in fp32 (output fp32), one hot LDS word."""
    logits, _, _, _ = _exact_case(vocab, 0, F16, F32, seed=vocab)
    ids = torch.full((B, 1025), vocab - 1, dtype=torch.int64, device=DEV)
    mask = torch.ones(B, 1025, dtype=torch.bool, device=DEV)
    mask[1, ::2] = False                       # row 1 counts 512
    f = torch.full((B,), 0.25, dtype=F32, device=DEV)
    ref, counts, _ = R.penalties_ref(logits, ids, mask, 2.0, 0.5, 0.25)
    assert counts[:, vocab - 1].tolist() == [1025, 512, 1025]
    _assert_exact(apply_penalties(logits, ids, mask, 2.0, 0.5, f), ref, F32, "hot token")


def test_bias_alone_needs_no_span():
    logits, _, _, bias = _exact_case(8193, 0, F16, F16, seed=1)
    ref, _, _ = R.penalties_ref(logits, None, None, 1.0, 0.0, 0.0, bias)
    _assert_exact(apply_penalties(logits, None, None, logit_bias=bias), ref, F16, "bias only")
    one = {8192: -2.5, 0: float("-inf")}
    ref, _, _ = R.penalties_ref(logits, None, None, 1.0, 0.0, 0.0, one)
    out = apply_penalties(logits, None, None, logit_bias=one)
    _assert_exact(out, ref, F16, "one dict for all rows")
    assert torch.isinf(out[:, 0]).all()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("vocab", [8193, 152064])
def test_bit_equal_to_the_repetition_penalty_when_the_rest_is_off(vocab, pair):
    in_dtype, out_dtype = pair
    g = torch.Generator().manual_seed(vocab)
    logits = (torch.randn(B, vocab, generator=g) * 4).to(in_dtype).to(DEV)
    logits[0, 5] = -0.0
    ids = torch.randint(-3, vocab + 3, (B, 257), generator=g).to(DEV)
    ids[:, :4] = torch.tensor([0, vocab - 1, 5, 5])
    mask = (torch.rand(B, 257, generator=g) < 0.8).to(DEV)
    pen = 1.3 if in_dtype == out_dtype else torch.tensor([1.3, 0.7, 2.5], dtype=F32, device=DEV)
    old = apply_repetition_penalty(logits, ids, mask, pen)
    new = apply_penalties(logits, ids, mask, pen, 0.0, 0.0, None)
    assert new.dtype == old.dtype == out_dtype
    bits = torch.int32 if out_dtype == F32 else torch.int16
    assert torch.equal(new.view(bits), old.view(bits))


def _half_ulp(y, dtype):
    """Half a unit in the last place of ``dtype`` at the float64 values ``y``."""
    mant, emin = {F16: (10, -14), F32: (23, -126)}[dtype]
    _, e = torch.frexp(y.abs())                # |y| = m 2^e, m in [0.5, 1): floor(log2 |y|) = e - 1
    return torch.ldexp(torch.ones_like(y), torch.clamp(e - 1, min=emin) - mant - 1)


@pytest.mark.parametrize("pair", [(F16, F16), (F16, F32), (F32, F32)], ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
@pytest.mark.parametrize("vocab", [8193, 152064])
def test_random_data_within_the_derived_bound(vocab, pair):
    """Arbitrary penalties on random data: at most four fp32 roundings (the bias add, the repetition multiply or divide, the
    fused frequency step, the presence subtraction), each of relative size 2^-24 on a magnitude that
    M = (|z| + |bias|) max(1, r, 1/r) + f c + p bounds, plus the rounding to the output dtype.  No output is exempt."""
    in_dtype, out_dtype = pair
    g = torch.Generator().manual_seed(vocab + 3)
    logits = (torch.randn(B, vocab, generator=g) * 6).to(in_dtype).to(DEV)
    ids = torch.randint(0, min(vocab, 600), (B, 1025), generator=g).to(DEV)
    ids[:, :2] = torch.tensor([0, vocab - 1])
    mask = (torch.rand(B, 1025, generator=g) < 0.9).to(DEV)
    toks = torch.randint(0, min(vocab, 600), (40,), generator=g).tolist() + [0, vocab - 1, 4095, 4096]
    bias = [dict(zip(toks, (torch.randn(len(toks), generator=g) * 5).tolist())), None, {7: -3.3}]
    r, p, f = [1.3, 0.7, 2.9], [0.37, 1.9, 0.0], [0.11, 0.013, 1.7]
    if in_dtype == out_dtype:
        r, p, f = r[0], p[0], f[0]
        out = apply_penalties(logits, ids, mask, r, p, f, bias)
    else:
        t = lambda v: torch.tensor(v, dtype=F32, device=DEV)
        out = apply_penalties(logits, ids, mask, t(r), t(p), t(f), bias)
    assert out.dtype == out_dtype
    ref, counts, dense = R.penalties_ref(logits, ids, mask, r, p, f, bias)
    f32 = lambda v: torch.tensor(v, dtype=F32).double().reshape(-1, 1)
    rr, pp, ff = f32(r), f32(p), f32(f)
    m = (logits.cpu().double().abs() + dense.abs()) * torch.maximum(torch.ones_like(rr), torch.maximum(rr, 1 / rr)) \
        + ff * counts.double() + pp
    bound = 4 * 2.0 ** -24 * m + _half_ulp(ref, out_dtype)
    err = (out.cpu().double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"vocab {vocab} {pair}: max err / bound = {worst:.3f}, max err = {err.max().item():.3e}")
    assert counts.max() > 1
    assert (err <= bound).all(), worst


def test_bad_arguments_are_refused():
    logits = torch.zeros(2, 16, dtype=F16, device=DEV)
    ids = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    mask = torch.ones(2, 3, dtype=torch.bool, device=DEV)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            apply_penalties(logits, ids, mask, bad)
    for bad in ({16: 1.0}, {-1: 1.0}, {3: float("nan")}, {3: float("inf")}, [{1: 1.0}], [None, None, None]):
        with pytest.raises(ValueError):
            apply_penalties(logits, ids, mask, logit_bias=bad)
    with pytest.raises(ValueError):
        apply_penalties(logits, ids, None)


# ---------------------------------------------------------------------------------------------- seeded_uniform
SEEDS = [0, 1, 2 ** 31, 2 ** 32 + 5, -1, 2 ** 63 - 1]


def test_python_philox_known_answers():
    R.check_known_answers()


@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("column", [0, 1, 2 ** 32])
def test_seeded_uniform_equals_the_python_philox(batch, column):
    """The counter comes from a device tensor that is incremented between the two launches."""
    seeds = [SEEDS[i % len(SEEDS)] - (i // len(SEEDS)) * 977 for i in range(batch)]
    if batch == 1:
        seeds = [SEEDS[3]]
    dev_seeds = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    col = torch.tensor([column], dtype=torch.int64, device=DEV)
    got = [seeded_uniform(dev_seeds, col).cpu()]
    col += 1
    got.append(seeded_uniform(dev_seeds, col).cpu())
    for k in range(2):
        want = torch.tensor([R.uniform_ref(s, column + k) for s in seeds], dtype=F32)
        assert got[k].dtype == F32 and torch.equal(got[k], want), (batch, column, k)
    assert not torch.equal(got[0], got[1])
    if column == 0:
        assert torch.equal(seeded_uniform(dev_seeds).cpu(), got[0])   # no counter: 0


def test_every_seed_of_the_list_alone_and_in_a_batch():
    for s in SEEDS:
        alone = seeded_uniform(torch.tensor([s], dtype=torch.int64, device=DEV)).item()
        assert alone == R.uniform_ref(s, 0), s
    both = seeded_uniform(torch.tensor(SEEDS, dtype=torch.int64, device=DEV)).tolist()
    assert both == [R.uniform_ref(s, 0) for s in SEEDS]


def test_seeded_uniform_stays_inside_the_unit_interval():
    u = seeded_uniform(torch.arange(4096, dtype=torch.int64, device=DEV), torch.tensor([3], dtype=torch.int64, device=DEV))
    assert (u >= 0).all() and (u < 1).all()
    assert u.unique().numel() > 4000 and 0.45 < u.mean().item() < 0.55


# ---------------------------------------------------------------------------------------------- Sampler
def test_sampler_reads_the_new_options():
    """``Sampler.sample`` / ``sample_batched`` run ``apply_penalties`` in the repetition penalty's place once an option is on
    -- a bias also without a generated span -- and the old path when all are off."""
    import types

    from lite_llama_amd.sampling import Sampler, SamplingParams, greedy_argmax

    g = torch.Generator().manual_seed(9)
    logits = torch.randn(4, 8193, generator=g).half().to(DEV)
    ids = torch.randint(0, 8193, (4, 33), generator=g).to(DEV)
    ids[:, 0] = greedy_argmax(logits)           # the best token has been emitted
    span = types.SimpleNamespace(token_ids=ids, mask=torch.ones(4, 33, dtype=torch.bool, device=DEV))
    s = Sampler()
    assert (s.sample(logits, SamplingParams(temperature=0.0, logit_bias={8192: 1000.0})) == 8192).all()
    got = s.sample(logits, SamplingParams(temperature=0.0, repetition_penalty=1.2, frequency_penalty=50.0), span)
    want = greedy_argmax(apply_penalties(logits, ids, span.mask, 1.2, 0.0, 50.0)).view(-1, 1)
    assert torch.equal(got, want) and not torch.equal(got.view(-1), ids[:, 0])
    neutral = SamplingParams(temperature=0.0, repetition_penalty=1.2)
    old = types.SimpleNamespace(temperature=0.0, top_p=1.0, repetition_penalty=1.2)
    assert torch.equal(s.sample(logits, neutral, span), s.sample(logits, old, span))
    batched = types.SimpleNamespace(temperature=None, top_p=None, greedy=None, all_greedy=True, any_penalty=False,
                                    repetition_penalty=1.0, presence_penalty=torch.full((4, 1), 50.0, device=DEV))
    got = s.sample_batched(logits, batched, span)
    assert torch.equal(got, greedy_argmax(apply_penalties(logits, ids, span.mask, 1.0, 50.0, 0.0)).view(-1, 1))
    assert not torch.equal(got.view(-1), ids[:, 0])
