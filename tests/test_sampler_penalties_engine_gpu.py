"""DecodeEngine.prefill / decode with ``presence_penalty`` / ``frequency_penalty`` / ``logit_bias`` / ``seed`` on the sampling
parameters, on the synthetic model of the filter engine tests and on both pools.  Every check is an equality or an order
statement read off the step's own raw log-probabilities (``logprobs = 20``: ordered by logit descending, token id
ascending -- the order the argmax breaks ties in), so no tie can blur it."""

import functools
import random
import types

import pytest
import torch

from lite_llama_amd.executor import ConstrainedRows, DecodeEngine, Speculation, StopCriteria, from_transitions
from lite_llama_amd.sampling import SamplingParams
from tests import _constraint_ref as C
from tests.test_chunked_prefill_gpu import _random_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_SEQ = 128
B = 8
STEPS = 12          # 13 tokens per row with the prefill's: fewer than the 20 alternatives a step reports
POOLS = {"bump": dict(), "paged": dict(kv_block_size=16)}
BIG = 1000.0


@functools.lru_cache(maxsize=None)
def _model():
    return _random_model()


def _vocab():
    return _model().geo.vocab_size


def _prompts():
    g = torch.Generator().manual_seed(11)
    lens = [33, 17, 40, 25, 32, 19, 38, 28]
    ids = torch.randint(0, _vocab(), (B, max(lens)), generator=g)
    for i, n in enumerate(lens):
        ids[i, n:] = 0
    return ids.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


def _run(pool, sp, steps=STEPS, torch_seed=3, flip=False, pre_kw=None, constraint=None, logprobs=20, **dec_kw):
    """Prefill + decode: the emitted tokens ``[rows, 1 + steps]`` (column 0 the prefill's) and, aligned with them, the raw
    ``top_ids [rows, 1 + steps, 20]``; ``flip`` reverses the order of the prompts."""
    eng = DecodeEngine(_model(), max_batch=B, max_seq_len=MAX_SEQ, **(POOLS[pool] if isinstance(pool, str) else pool))
    ids, lens = _prompts()
    if flip:
        ids, lens = ids.flip(0).contiguous(), lens.flip(0).contiguous()
    pre_kw = dict(pre_kw or {})
    if "num_samples" in pre_kw:
        ids, lens = ids[:B // pre_kw["num_samples"]].contiguous(), lens[:B // pre_kw["num_samples"]].contiguous()
    torch.manual_seed(torch_seed)
    first = eng.prefill(ids, lens, sampling=sp, logprobs=logprobs, constraint=constraint, **pre_kw)
    dec_kw.setdefault("use_graph", True)
    toks = eng.decode(first, steps, sampling=sp, logprobs=logprobs, constraint=constraint, **dec_kw)
    out = types.SimpleNamespace(tokens=torch.cat([first.view(-1, 1), toks], dim=1).cpu(), engine=eng)
    if logprobs is not None:
        out.ids = torch.cat([eng.first_logprobs.top_ids, eng.last_logprobs.top_ids], dim=1).cpu()
    return out


@functools.lru_cache(maxsize=None)
def _plain_greedy(pool):
    return _run(pool, None)


# ------------------------------------------------------------------------------------------------ neutral options
@pytest.mark.parametrize("dec_kw", [dict(use_graph=False), dict(use_graph=True), dict(use_graph=True, steps_per_graph=2)],
                         ids=["eager", "graph", "2-steps-per-graph"])
@pytest.mark.parametrize("pool", list(POOLS))
def test_neutral_options_draw_what_was_always_drawn(pool, dec_kw):
    old = types.SimpleNamespace(temperature=1.2, top_p=0.9, repetition_penalty=1.1)
    neutral = SamplingParams(temperature=1.2, top_p=0.9, repetition_penalty=1.1, presence_penalty=0.0, frequency_penalty=0.0,
                             logit_bias=None, seed=None)
    base = _run(pool, old, torch_seed=5, logprobs=None, **dec_kw).tokens
    assert torch.equal(_run(pool, neutral, torch_seed=5, logprobs=None, **dec_kw).tokens, base)
    assert not torch.equal(_run(pool, old, torch_seed=6, logprobs=None, **dec_kw).tokens, base), "the draws do vary"


# ------------------------------------------------------------------------------------------------ penalties
def _assert_first_unseen(run, banned=()):
    """Every token is the first entry of its step's raw ``top_ids`` that the row has not emitted (and that is not banned)."""
    for i in range(run.tokens.shape[0]):
        seen = set(banned)
        for c in range(run.tokens.shape[1]):
            fresh = [t for t in run.ids[i, c].tolist() if t not in seen]
            assert fresh, f"row {i} step {c}: all 20 alternatives are taken -- the case is too long to read"
            assert int(run.tokens[i, c]) == fresh[0], (i, c, int(run.tokens[i, c]), fresh[:3])
            if not banned:
                seen.add(fresh[0])


@pytest.mark.parametrize("dec_kw", [dict(use_graph=False), dict(use_graph=True, steps_per_graph=2)], ids=["eager", "2-steps-per-graph"])
@pytest.mark.parametrize("which", ["frequency_penalty", "presence_penalty"])
@pytest.mark.parametrize("pool", list(POOLS))
def test_a_huge_penalty_never_repeats_a_token(pool, which, dec_kw):
    plain = _plain_greedy(pool).tokens
    assert any(len(set(row.tolist())) < row.numel() for row in plain), "the plain greedy decode repeats no token"
    run = _run(pool, SamplingParams(temperature=0.0, **{which: BIG}), **dec_kw)
    for row in run.tokens:
        assert len(set(row.tolist())) == row.numel()
    _assert_first_unseen(run)
    assert not torch.equal(run.tokens, plain)


def test_the_frequency_penalty_counts():
    """frequency_penalty = f on a row forced to weigh two tokens only: with the bias ``{a: BIG, b: BIG - 2.5 f}`` the row
    emits ``a`` until its count has cost more than the head start -- three times -- then ``b``, and so on: the order is
    decided by counts alone (the model's own logits differ by far less than f / 2)."""
    a, b, f = 3, 700, 64.0
    sp = SamplingParams(temperature=0.0, frequency_penalty=f, logit_bias={a: BIG, b: BIG - 2.5 * f})
    run = _run("bump", sp, steps=9, logprobs=None)
    # a leads by (2.5 - (count of a - count of b)) f, never by less than f / 2: a a a b a b a b a b
    want, ca, cb = [], 0, 0
    for _ in range(10):
        if ca - cb < 2.5:
            want.append(a)
            ca += 1
        else:
            want.append(b)
            cb += 1
    assert set(want) == {a, b}
    for row in run.tokens.tolist():
        assert row == want


# ------------------------------------------------------------------------------------------------ bias
@pytest.mark.parametrize("dec_kw", [dict(use_graph=False), dict(use_graph=True)], ids=["eager", "graph"])
@pytest.mark.parametrize("pool", list(POOLS))
def test_minus_infinity_bans_tokens(pool, dec_kw):
    banned = set(_plain_greedy(pool).tokens[:, :7].reshape(-1).tolist())
    run = _run(pool, SamplingParams(temperature=0.0, logit_bias={t: float("-inf") for t in banned}), steps=6, **dec_kw)
    assert not banned & set(run.tokens.reshape(-1).tolist())
    _assert_first_unseen(run, banned)


@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("pool", list(POOLS))
def test_a_huge_bias_forces_its_token(pool, temperature):
    sp = SamplingParams(temperature=temperature, top_p=0.9, logit_bias={611: BIG})
    assert (_run(pool, sp, steps=5, logprobs=None).tokens == 611).all()
    rows = [{100 + i: BIG} for i in range(B)]
    rows[3] = None
    got = _run(pool, SamplingParams(temperature=temperature, top_p=0.9, logit_bias=rows, seed=1), steps=5).tokens
    for i in range(B):
        if i != 3:
            assert (got[i] == 100 + i).all()
    if temperature == 0.0:
        assert torch.equal(got[3], _plain_greedy(pool).tokens[3, :6])


def test_the_bias_reaches_every_prefill_route():
    sp = SamplingParams(temperature=0.0, logit_bias={77: BIG})
    for pool, pre_kw in (("bump", dict(chunk_size=16)), (dict(kv_block_size=16, kv_share_blocks=True), dict(num_samples=4))):
        assert (_run(pool, sp, steps=3, logprobs=None, pre_kw=pre_kw).tokens == 77).all()
    eng = DecodeEngine(_model(), max_batch=B, max_seq_len=MAX_SEQ)
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(0, _vocab(), (40,), generator=g).to(DEV)
    tails = torch.randint(0, _vocab(), (B, 4), generator=g).to(DEV)
    first = eng.prefill(tails, None, sampling=sp, shared_prefix_ids=prefix)
    assert (first == 77).all() and (eng.decode(first, 3, sampling=sp) == 77).all()


# ------------------------------------------------------------------------------------------------ seeds
def _seeded(seed, **kw):
    return SamplingParams(temperature=1.5, top_p=0.95, seed=seed, **kw)


@pytest.mark.parametrize("pool", list(POOLS))
def test_seeds_replay_on_every_route(pool):
    """Same seeds, same tokens -- whatever the global generator holds and however the steps are launched."""
    base = _run(pool, _seeded(7), torch_seed=1, logprobs=None, use_graph=False).tokens
    assert torch.equal(_run(pool, _seeded(7), torch_seed=2, logprobs=None, use_graph=False).tokens, base)
    assert torch.equal(_run(pool, _seeded(7), torch_seed=3, logprobs=None, use_graph=True).tokens, base)
    assert torch.equal(_run(pool, _seeded(7), torch_seed=4, logprobs=None, use_graph=True, steps_per_graph=2).tokens, base)
    assert torch.equal(_run(pool, _seeded(list(range(7, 7 + B))), logprobs=None).tokens, base), "s means s, s + 1, ..."
    other = _run(pool, _seeded(8), torch_seed=1, logprobs=None).tokens
    assert all(not torch.equal(other[i], base[i]) for i in range(B)), "other seeds, other tokens: in every row"


@pytest.mark.parametrize("pool", list(POOLS))
def test_reversing_rows_and_seeds_reverses_the_tokens(pool):
    seeds = [5, 900, -3, 2 ** 40, 17, 17, 2 ** 63 - 1, 0]
    sp = lambda s: _seeded(s, repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.2, top_k=50)
    fwd = _run(pool, sp(seeds), logprobs=None).tokens
    rev = _run(pool, sp(seeds[::-1]), logprobs=None, flip=True).tokens
    assert torch.equal(rev.flip(0), fwd)


@pytest.mark.parametrize("pool", list(POOLS))
def test_seeded_rows_still_running_do_not_see_the_others_stop(pool):
    free = _run(pool, _seeded(7), logprobs=None).tokens
    stop = StopCriteria(stop_token_ids=[int(free[5, 7])], max_tokens=[2, STEPS, 5, STEPS, STEPS, STEPS, 9, STEPS], check_every=0)
    run = _run(pool, _seeded(7), logprobs=None, stop=stop)
    lengths = run.engine.last_lengths.cpu().tolist()             # valid returned tokens; column 0 here is the prefill's
    assert lengths[0] == 2 and lengths[2] == 5 and lengths[5] <= 7 and max(lengths) == STEPS
    for i, n in enumerate(lengths):
        assert torch.equal(run.tokens[i, :n + 1], free[i, :n + 1]), i


def test_the_samples_of_a_prompt_draw_different_streams():
    run = _run(dict(kv_block_size=16, kv_share_blocks=True), _seeded(7), logprobs=None, pre_kw=dict(num_samples=2))
    assert run.tokens.shape == (B, STEPS + 1)
    for i in range(0, B, 2):
        assert not torch.equal(run.tokens[i], run.tokens[i + 1]), i
    again = _run(dict(kv_block_size=16, kv_share_blocks=True), _seeded(7), torch_seed=9, logprobs=None, pre_kw=dict(num_samples=2))
    assert torch.equal(again.tokens, run.tokens)


# ------------------------------------------------------------------------------------------------ other routes
@functools.lru_cache(maxsize=None)
def _half_automaton():
    rng = random.Random(16)
    return from_transitions({s: {t: rng.randrange(16) for t in rng.sample(range(1024), 512)} for s in range(16)})


@pytest.mark.parametrize("dec_kw", [dict(use_graph=False), dict(use_graph=True, steps_per_graph=2)], ids=["eager", "2-steps-per-graph"])
@pytest.mark.parametrize("pool", list(POOLS))
def test_a_constraint_still_holds_under_bias_penalties_and_seeds(pool, dec_kw):
    lists = C.lists(_half_automaton())
    rng = random.Random(2)
    sp = SamplingParams(temperature=1.3, top_p=0.9, repetition_penalty=1.1, presence_penalty=0.4, frequency_penalty=0.3,
                        logit_bias={t: 6.0 for t in rng.sample(range(1024), 64)}, seed=21)
    runs = []
    for _ in range(2):
        rows = ConstrainedRows(_half_automaton(), 0, B, DEV)
        run = _run(pool, sp, logprobs=None, constraint=rows, **dec_kw)
        assert rows.error.item() == 0
        for i in range(B):
            state = 0
            for tok in run.tokens[i].tolist():
                assert tok in set(C.allowed(lists, state)), (i, tok)
                state = C.advance(lists, state, tok)
        runs.append(run.tokens)
    assert torch.equal(runs[0], runs[1])


def test_speculation_still_refuses_sampling():
    eng = DecodeEngine(_model(), max_batch=B, max_seq_len=MAX_SEQ, kv_block_size=16)
    ids, lens = _prompts()
    first = eng.prefill(ids, lens)
    with pytest.raises(ValueError, match="sampling cannot be combined with speculate"):
        eng.decode(first, 4, speculate=Speculation(2), sampling=SamplingParams(temperature=0.0, presence_penalty=0.5, seed=1))
