"""DecodeEngine.decode(stop=...): rows end at stop ids, stop sequences and max_tokens inside the (captured) step.  On the
golden tiny fixtures and on a synthetic model, every result is compared with the plain-Python reference tests/_stop_ref.py
applied to the tokens of a decode without ``stop`` -- rows still running must not notice that others stopped, so those
tokens are the stream the reference needs."""

import functools
import types

import pytest
import torch

from lite_llama_amd.executor import DecodeEngine, StopCriteria
from tests import _stop_ref as R
from tests.test_chunked_prefill_gpu import FAMILIES, _load, _random_model
from tests.test_model_step import _hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 12
NO_LIMIT = 1000
MAX_SEQ = 128


def _check_against_reference(eng, toks, first0, toks0, crit, what=""):
    """``toks`` / the engine's lengths and reasons against the reference on the plain run ``first0, toks0``; returns the
    reference's ``(lengths, reasons)``."""
    want, lengths, reasons = R.apply(first0.tolist(), toks0.tolist(), crit.stop_token_ids, crit.stop_sequences,
                                     crit.max_tokens, crit.pad_token_id)
    assert eng.last_lengths.dtype == torch.int32 and eng.last_finish_reasons.dtype == torch.int32
    assert eng.last_lengths.tolist() == lengths, (what, eng.last_lengths.tolist(), lengths)
    assert eng.last_finish_reasons.tolist() == reasons, (what, eng.last_finish_reasons.tolist(), reasons)
    assert toks.tolist() == want, what                           # the plain run up to each length, the pad after it
    return lengths, reasons


# ------------------------------------------------------------------ golden fixtures ----- #
def _absent(row, other, avoid):
    """Column of the first token of ``row`` (from column 2 on) that ``other`` and ``avoid`` do not hold; else column 5."""
    for c in range(2, len(row) - 1):
        if row[c] not in other and row[c] not in avoid:
            return c
    return 5


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kv_block_size", [None, 4])
def test_stop_on_the_golden_fixtures(family, kv_block_size):
    d, params = _load(family)
    m = _hip_model(params, None, family)
    ids = torch.from_numpy(d["prompt_ids"]).to(DEV)
    lens = torch.from_numpy(d["lens"]).int().to(DEV)
    pad = 3
    got = {}
    for use_graph in (False, True):
        plain = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
        first0 = plain.prefill(ids, lens)
        toks0 = plain.decode(first0, STEPS, use_graph=use_graph)
        assert plain.last_lengths is None and plain.last_finish_reasons is None and plain.last_steps_run is None
        f, t = first0.tolist(), toks0.tolist()
        # a stop id row 0 emits and, where the run allows it, row 1 does not; the two tokens before it as a sequence that
        # can then end row 0 only earlier; second run: the sequence alone
        c = _absent(t[0], t[1], f)
        seq = [t[0][c - 1], t[0][c]]
        runs = []
        for crit in (StopCriteria(stop_token_ids=[t[0][c]], stop_sequences=[seq], pad_token_id=pad, check_every=4),
                     StopCriteria(stop_sequences=[seq], pad_token_id=pad, check_every=4)):
            eng = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
            first = eng.prefill(ids, lens)
            toks = eng.decode(first, STEPS, use_graph=use_graph, stop=crit)
            assert torch.equal(first, first0) and toks.shape == (2, STEPS)
            lengths, reasons = _check_against_reference(eng, toks, first0, toks0, crit, (family, use_graph))
            assert any(reasons) and min(lengths) < STEPS, "a row stops"
            print(f"{family} bs={kv_block_size} graph={use_graph}: lengths {lengths} reasons {reasons} "
                  f"steps run {eng.last_steps_run}")
            runs.append((toks.cpu(), lengths, reasons))
        assert runs[0][2][0] in (R.STOP_TOKEN, R.STOP_SEQUENCE) and runs[1][2][0] == R.STOP_SEQUENCE
        got[use_graph] = runs
    for a, b in zip(got[False], got[True]):                      # graph equals eager
        assert torch.equal(a[0], b[0]) and a[1:] == b[1:]


# ------------------------------------------------------------------ synthetic model, batch 8 ----- #
@functools.lru_cache(maxsize=None)
def _model():
    return _random_model()


def _prompts():
    g = torch.Generator().manual_seed(11)
    lens = [33, 17, 40, 25, 32, 19, 38, 28]                      # on and off the block boundaries of 16
    ids = torch.randint(0, _model().geo.vocab_size, (8, max(lens)), generator=g)
    for i, n in enumerate(lens):
        ids[i, n:] = 0
    return ids.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


def _engine(bs=None, share=False):
    return DecodeEngine(_model(), max_batch=8, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=share)


@functools.lru_cache(maxsize=None)
def _plain(bs, use_graph, steps, logprobs=None):
    """One decode without ``stop`` per configuration, shared by the tests: ``(engine, first tokens, tokens)``."""
    eng = _engine(bs)
    ids, lens = _prompts()
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, steps, use_graph=use_graph, logprobs=logprobs)
    return eng, first.clone(), toks.clone()


def _criteria(first, toks, **kw):
    """Stops that certainly occur in the plain run: two stop ids (rows 0, 1), a 2-token sequence (row 3), a max_tokens
    (row 4); rows 5 - 7 go on unless they meet one of these by chance."""
    t = toks.tolist()
    limits = [NO_LIMIT] * 8
    limits[4] = 6
    return StopCriteria(stop_token_ids=[t[0][3], t[1][7]], stop_sequences=[[t[3][4], t[3][5]]], max_tokens=limits,
                        pad_token_id=1, **kw)


def _kv_rows(eng, row, n):
    """The K/V of positions ``0 .. n - 1`` of batch row ``row``, reached through the token table, per layer."""
    rows = eng.info.b_req_tokens_table[int(eng.info.b_req_idx[row]), :n].long()
    return [kv[rows].view(torch.uint8) for kv in eng.pool.kv_buffer]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("bs", [None, 16])
def test_kv_of_finished_rows_stays_intact(bs, use_graph):
    plain, first0, toks0 = _plain(bs, use_graph, STEPS)
    crit = _criteria(first0, toks0)
    ids, lens = _prompts()
    eng = _engine(bs)
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, STEPS, use_graph=use_graph, stop=crit)
    lengths, reasons = _check_against_reference(eng, toks, first0, toks0, crit)
    assert {R.STOP_TOKEN, R.STOP_SEQUENCE, R.MAX_TOKENS, R.RUNNING} <= set(reasons), reasons
    ctx = eng.info.b_seq_len.tolist()
    for i, (n, why) in enumerate(zip(lengths, reasons)):
        # a row's context ends with the token it was fed at the step it finished at: the prompt and n returned tokens less
        # the finishing one, plus the prefill's token; a running row has named the row of the next step already
        assert ctx[i] == int(lens[i]) + (max(n, 1) if why else STEPS + 1), (i, ctx[i])
        if why:
            for layer, (a, b) in enumerate(zip(_kv_rows(eng, i, ctx[i]), _kv_rows(plain, i, ctx[i]))):
                assert torch.equal(a, b), (i, layer)
    if bs is not None:
        assert eng.pool.error == 0
        # a frozen row pops no block: it holds the blocks of its final context and no more
        held = eng.pool.req_blocks.tolist()
        for i, why in enumerate(reasons):
            if why:
                assert held[i] == (ctx[i] + bs - 1) // bs, (i, held[i], ctx[i])


@pytest.mark.parametrize("use_graph", [False, True])
def test_siblings_of_a_finished_sample_go_on_as_before(use_graph):
    """Two prompts x 4 samples on the shared paged pool, temperature 1 so that siblings diverge; the generator is seeded
    identically before each run, eager and captured (the draws of two captured runs coincide: the capture registers the
    generator's state, and both runs consume it alike)."""
    sp = types.SimpleNamespace(temperature=1.0, top_p=0.95, repetition_penalty=1.0)
    ids, lens = _prompts()
    ids, lens = ids[:2].contiguous(), lens[:2].contiguous()

    def run(stop):
        torch.manual_seed(77)
        eng = _engine(16, share=True)
        first = eng.prefill(ids, lens, sampling=sp, num_samples=4)
        return eng, first, eng.decode(first, STEPS, use_graph=use_graph, sampling=sp, stop=stop)

    plain, first0, toks0 = run(None)
    t = toks0.tolist()
    assert len({tuple(r) for r in t[:4]}) > 1 and len({tuple(r) for r in t[4:]}) > 1, "siblings diverge"
    # one sibling of each prompt finishes early; the others meet these ids only by chance
    crit = StopCriteria(stop_token_ids=[t[1][2], t[6][4]], pad_token_id=1, check_every=2)
    eng, first, toks = run(crit)
    assert torch.equal(first, first0)
    lengths, reasons = _check_against_reference(eng, toks, first0, toks0, crit)
    assert reasons[1] == 1 and reasons[6] == 1 and reasons.count(0) >= 2, reasons
    assert eng.pool.error == 0
    # the finished siblings' K/V, shared blocks included, is what the plain run holds
    ctx = eng.info.b_seq_len.tolist()
    for i, why in enumerate(reasons):
        if why:
            for a, b in zip(_kv_rows(eng, i, ctx[i]), _kv_rows(plain, i, ctx[i])):
                assert torch.equal(a, b), i
    assert torch.equal(eng.pool.block_share, plain.pool.block_share)


def test_after_a_shared_prefix_prefill():
    m = _model()
    g = torch.Generator().manual_seed(5)
    pre = torch.randint(0, m.geo.vocab_size, (80,), generator=g).to(DEV)
    tails = torch.randint(0, m.geo.vocab_size, (8, 6), generator=g).to(DEV)
    tl = torch.tensor([6, 3, 5, 6, 1, 4, 6, 2], dtype=torch.int32, device=DEV)
    runs = []
    for stop in (False, True):
        eng = _engine()
        first = eng.prefill(tails, tl, shared_prefix_ids=pre)
        crit = _criteria(runs[0][0], runs[0][1]) if stop else None
        toks = eng.decode(first, STEPS, use_graph=True, stop=crit)
        runs.append((first, toks))
    assert torch.equal(runs[0][0], runs[1][0])
    _, reasons = _check_against_reference(eng, runs[1][1], runs[0][0], runs[0][1], crit)
    assert any(reasons) and not all(reasons)


def test_results_do_not_depend_on_check_every_or_steps_per_graph():
    _, first0, toks0 = _plain(16, True, STEPS)
    ids, lens = _prompts()
    base = None
    for check_every in (0, 1, 4):
        for group in (1, 4):
            eng = _engine(16)
            first = eng.prefill(ids, lens)
            crit = _criteria(first0, toks0, check_every=check_every)
            toks = eng.decode(first, STEPS, use_graph=True, steps_per_graph=group, stop=crit)
            _check_against_reference(eng, toks, first0, toks0, crit, (check_every, group))
            ctx = eng.info.b_seq_len.tolist()
            kv = [_kv_rows(eng, i, ctx[i]) for i in range(8)]
            if base is None:
                base = (ctx, kv)
                continue
            assert ctx == base[0], (check_every, group)
            for mine, theirs in zip(kv, base[1]):
                for a, b in zip(mine, theirs):
                    assert torch.equal(a, b), (check_every, group)


@pytest.mark.parametrize("bs", [None, 16])
@pytest.mark.parametrize("use_graph,group", [(False, 1), (True, 1), (True, 4)])
def test_early_exit(bs, use_graph, group):
    steps, every = 40, 4
    _, first0, toks0 = _plain(bs, use_graph, steps)
    t = toks0.tolist()
    # every row has ended by its limit at the latest; rows 0 and 1 end earlier, by stop id
    crit = dict(stop_token_ids=[t[0][3], t[1][7]], max_tokens=[20, 20, 5, 9, 14, 3, 11, 17], pad_token_id=1)
    _, lengths, reasons = R.apply(first0.tolist(), t, crit["stop_token_ids"], (), crit["max_tokens"], 1)
    s = max(lengths)
    assert all(reasons) and s <= 20
    ids, lens = _prompts()
    out = {}
    for check_every in (every, 0):
        eng = _engine(bs)
        first = eng.prefill(ids, lens)
        c = StopCriteria(check_every=check_every, **crit)
        toks = eng.decode(first, steps, use_graph=use_graph, steps_per_graph=group, stop=c)
        assert toks.shape == (8, steps)
        _check_against_reference(eng, toks, first0, toks0, c, check_every)     # pads in the steps never run too
        out[check_every] = eng.last_steps_run
    print(f"bs={bs} graph={use_graph} group={group}: all rows done by step {s}, steps run {out}")
    assert s <= out[every] <= s + 2 * every, out
    assert out[0] == steps


@pytest.mark.parametrize("bs", [None, 16])
def test_logprobs_end_at_the_length(bs):
    plain, first0, toks0 = _plain(bs, True, STEPS, logprobs=5)
    want = plain.last_logprobs
    crit = _criteria(first0, toks0)
    ids, lens = _prompts()
    eng = _engine(bs)
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, STEPS, use_graph=True, logprobs=5, stop=crit)
    lengths, reasons = _check_against_reference(eng, toks, first0, toks0, crit)
    lp = eng.last_logprobs
    assert torch.equal(lp.cumulative(), lp.cumulative(eng.last_lengths))
    keep = torch.arange(STEPS, device=DEV).unsqueeze(0) < eng.last_lengths.view(-1, 1)
    assert not bool(keep.all()) and torch.all(lp.chosen[keep] < 0)
    # below each length: the plain run's; at and beyond it: the buffers' initial values
    assert torch.equal(lp.chosen[keep], want.chosen[keep])
    assert torch.equal(lp.top_logprobs[keep], want.top_logprobs[keep]) and torch.equal(lp.top_ids[keep], want.top_ids[keep])
    assert torch.all(lp.chosen[~keep] == 0.0) and torch.all(lp.top_logprobs[~keep] == 0.0)
    assert torch.all(lp.top_ids[~keep] == -1)


@pytest.mark.parametrize("bs", [None, 16])
def test_no_residue(bs):
    _, first0, toks0 = _plain(bs, True, STEPS)
    ids, lens = _prompts()
    eng = _engine(bs)
    first = eng.prefill(ids, lens)
    eng.decode(first, STEPS, use_graph=True, stop=_criteria(first0, toks0))
    assert eng.last_lengths is not None and eng.last_steps_run is not None
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, STEPS, use_graph=True)
    assert torch.equal(first, first0) and torch.equal(toks, toks0)
    assert eng.last_lengths is None and eng.last_finish_reasons is None and eng.last_steps_run is None


def test_refusals():
    ids, lens = _prompts()
    eng = _engine()
    first = eng.prefill(ids, lens)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        eng.decode(first, 4, stop=StopCriteria(stop_token_ids=[_model().geo.vocab_size]))
    with pytest.raises(ValueError, match="batch of 8"):
        eng.decode(first, 4, stop=StopCriteria(max_tokens=[3, 3]))
