"""DecodeEngine.prefill / decode(constraint=...): every row emits only what its automaton state allows, inside the
(captured) step.  On a synthetic model and the golden tiny fixtures; the automaton side of every check is the plain-Python
reference tests/_constraint_ref.py."""

import functools
import random
import types

import pytest
import torch

from lite_llama_amd.executor import (ConstrainedRows, DecodeEngine, StopCriteria, TokenAutomaton, from_choices,
                                     from_transitions, union)
from tests import _constraint_ref as R
from tests import _stop_ref as S
from tests.test_chunked_prefill_gpu import FAMILIES, _load, _random_model
from tests.test_model_step import _hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 12
MAX_SEQ = 128
B = 8


@functools.lru_cache(maxsize=None)
def _model():
    return _random_model()


def _prompts():
    g = torch.Generator().manual_seed(11)
    lens = [33, 17, 40, 25, 32, 19, 38, 28]                      # on and off the block boundaries of 16
    ids = torch.randint(0, _model().geo.vocab_size, (B, max(lens)), generator=g)
    for i, n in enumerate(lens):
        ids[i, n:] = 0
    return ids.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


def _engine(bs=None, share=False):
    return DecodeEngine(_model(), max_batch=B, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=share)


def _run(automaton, starts=0, bs=None, share=False, steps=STEPS, prefill_kw=None, **decode_kw):
    """Prefill + decode of the 8 prompts under ``automaton``: ``(engine, rows, first tokens, tokens)``."""
    eng = _engine(bs, share)
    rows = None if automaton is None else ConstrainedRows(automaton, starts, B, DEV)
    ids, lens = _prompts()
    first = eng.prefill(ids, lens, constraint=rows, **(prefill_kw or {}))
    toks = eng.decode(first, steps, constraint=rows, **decode_kw)
    return eng, rows, first.clone(), toks.clone()


@functools.lru_cache(maxsize=None)
def _plain(bs=None, use_graph=True):
    _, _, first, toks = _run(None, bs=bs, use_graph=use_graph)
    return first, toks


def _chain(seq):
    """State ``i`` allows ``seq[i]`` alone and leads to ``i + 1``; the last state loops."""
    n = len(seq)
    return from_transitions({i: {t: min(i + 1, n - 1)} for i, t in enumerate(seq)})


# ------------------------------------------------------------------ forced chain ----- #
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("bs", [None, 16])
def test_forced_chain(bs, use_graph):
    """One edge per state: the returned tokens are the chain's whatever the model says -- one chain per row."""
    rng = random.Random(3)
    seqs = [[rng.randrange(1024) for _ in range(STEPS + 2)] for _ in range(B)]
    aut, starts = union([_chain(s) for s in seqs])
    eng, rows, first, toks = _run(aut, starts, bs=bs, use_graph=use_graph)
    assert first.tolist() == [s[0] for s in seqs]
    assert toks.tolist() == [s[1:STEPS + 1] for s in seqs]
    assert rows.states.tolist() == [s0 + STEPS + 1 for s0 in starts] and rows.error.item() == 0
    first0, toks0 = _plain(bs, use_graph)
    assert not torch.equal(toks, toks0), "the model alone says something else"


@pytest.mark.parametrize("use_graph,group", [(False, 1), (True, 1), (True, 4)])
def test_forced_chain_with_stop_freezes_the_state(use_graph, group):
    """A stop id in the middle of the chain: the finishing step advances the state, later steps (``check_every=0``: they
    all run) do not."""
    seq = list(range(100, 100 + STEPS + 2))
    k = 5
    crit = StopCriteria(stop_token_ids=[seq[k]], pad_token_id=1, check_every=0)
    eng, rows, first, toks = _run(_chain(seq), use_graph=use_graph, steps_per_graph=group, stop=crit)
    assert eng.last_steps_run == STEPS
    assert eng.last_lengths.tolist() == [k] * B and eng.last_finish_reasons.tolist() == [S.STOP_TOKEN] * B
    assert toks.tolist() == [seq[1:k + 1] + [1] * (STEPS - k)] * B
    aut = R.lists(rows.automaton)
    assert rows.states.tolist() == [R.walk(aut, 0, seq[:k + 1])] * B == [k + 1] * B


# ------------------------------------------------------------------ full vocabulary ----- #
def _everything(vocab):
    return TokenAutomaton([0, vocab], list(range(vocab)), [0] * vocab)


@pytest.mark.parametrize("use_graph", [False, True])
def test_full_vocabulary_equals_unconstrained(use_graph):
    first0, toks0 = _plain(None, use_graph)
    _, rows, first, toks = _run(_everything(1024), use_graph=use_graph)
    assert torch.equal(first, first0) and torch.equal(toks, toks0)
    assert rows.states.tolist() == [0] * B


@pytest.mark.parametrize("family", FAMILIES)
def test_on_the_golden_fixtures(family):
    """Everything allowed: the tokens of a plain decode, bit for bit, prefill token included; a chain: the chain."""
    d, params = _load(family)
    m = _hip_model(params, None, family)
    vocab = m.geo.vocab_size
    ids = torch.from_numpy(d["prompt_ids"]).to(DEV)
    lens = torch.from_numpy(d["lens"]).int().to(DEV)
    seq = [(37 * i + 5) % vocab for i in range(STEPS + 2)]
    out = []
    for aut in (None, _everything(vocab), _chain(seq)):
        eng = DecodeEngine(m, max_batch=2, max_seq_len=64)
        rows = None if aut is None else ConstrainedRows(aut, 0, 2, DEV)
        first = eng.prefill(ids, lens, constraint=rows)
        out.append((first, eng.decode(first, STEPS, constraint=rows)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[2][0].tolist() == [seq[0]] * 2 and out[2][1].tolist() == [seq[1:STEPS + 1]] * 2


# ------------------------------------------------------------------ random automaton ----- #
@functools.lru_cache(maxsize=None)
def _half_automaton():
    """16 states, each allowing a seeded random half of the 1024 tokens, with random next states."""
    rng = random.Random(16)
    return from_transitions({s: {t: rng.randrange(16) for t in rng.sample(range(1024), 512)} for s in range(16)})


def _check_against_top20(aut, state, token, top_ids, where):
    """``token`` is the best allowed one of the step whose own top-20 ids (ordered by logit descending, id ascending, the
    kernel's order too) are ``top_ids``; returns the next state."""
    ok = set(R.allowed(aut, state))
    assert token in ok, where
    # with half the vocabulary allowed the best allowed token lies outside the top 20 with probability 2^-20
    assert token in top_ids, (where, "none of the top 20 is allowed?", [t in ok for t in top_ids])
    assert not any(t in ok for t in top_ids[:top_ids.index(token)]), where
    return R.advance(aut, state, token)


@pytest.mark.parametrize("use_graph", [False, True])
def test_random_automaton_against_the_steps_own_top20(use_graph):
    a = _half_automaton()
    aut = R.lists(a)
    eng, rows, first, toks = _run(a, use_graph=use_graph, prefill_kw=dict(logprobs=20), logprobs=20)
    first_top = eng.first_logprobs.top_ids[:, 0].tolist()
    top = eng.last_logprobs.top_ids.tolist()
    f, t = first.tolist(), toks.tolist()
    final = []
    for i in range(B):
        state = _check_against_top20(aut, 0, f[i], first_top[i], (i, "prefill"))
        for c in range(STEPS):
            state = _check_against_top20(aut, state, t[i][c], top[i][c], (i, c))
        final.append(state)
        assert state == R.walk(aut, 0, [f[i]] + t[i])
    assert rows.states.tolist() == final and rows.error.item() == 0
    first0, toks0 = _plain(None, use_graph)
    assert not torch.equal(toks, toks0), "the constraint does bind"


# ------------------------------------------------------------------ routes ----- #
def test_every_route_gives_the_same_tokens_and_states():
    a = _half_automaton()
    base = None
    for what, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True)),
                     ("4 steps per graph", dict(use_graph=True, steps_per_graph=4)),
                     ("paged 4", dict(bs=4)), ("paged 16, eager", dict(bs=16, use_graph=False)),
                     ("shared blocks", dict(bs=16, share=True))):
        _, rows, first, toks = _run(a, **kw)
        got = (first.tolist(), toks.tolist(), rows.states.tolist())
        base = base or got
        assert got == base, what
    # a chunked prefill computes its logits along another route (near-ties may fall the other way): the states follow
    # whatever tokens it gives
    _, rows, first, toks = _run(a, prefill_kw=dict(chunk_size=16))
    aut = R.lists(a)
    assert rows.states.tolist() == [R.walk(aut, 0, [f] + t) for f, t in zip(first.tolist(), toks.tolist())]


def test_after_a_shared_prefix_prefill():
    m = _model()
    a = _half_automaton()
    g = torch.Generator().manual_seed(5)
    pre = torch.randint(0, m.geo.vocab_size, (80,), generator=g).to(DEV)
    tails = torch.randint(0, m.geo.vocab_size, (B, 6), generator=g).to(DEV)
    tl = torch.tensor([6, 3, 5, 6, 1, 4, 6, 2], dtype=torch.int32, device=DEV)
    aut = R.lists(a)
    for bs, share in ((None, False), (16, True)):
        eng = _engine(bs, share)
        rows = ConstrainedRows(a, 0, B, DEV)
        first = eng.prefill(tails, tl, shared_prefix_ids=pre, constraint=rows)
        toks = eng.decode(first, STEPS, constraint=rows)
        walked = [R.walk(aut, 0, [f] + t) for f, t in zip(first.tolist(), toks.tolist())]
        assert None not in walked and rows.states.tolist() == walked, bs
        assert rows.error.item() == 0


# ------------------------------------------------------------------ choices ----- #
EOS = 7
CHOICES = [[11, 12, 13], [11, 12], [500], [640, 3, 3, 9], [11, 900, 2]]


def _spelled_choice(first, toks, length, choices):
    valid = [first] + toks[:length]
    assert valid[-1] == EOS and valid[:-1] in choices, valid
    return valid


@pytest.mark.parametrize("use_graph,group", [(False, 1), (True, 1), (True, 4)])
@pytest.mark.parametrize("bs", [None, 16])
def test_choices_with_stop_on_eos(bs, use_graph, group):
    a = from_choices(CHOICES, EOS)
    end = a.num_states - 1
    crit = StopCriteria(stop_token_ids=[EOS], pad_token_id=1, check_every=0)
    eng, rows, first, toks = _run(a, bs=bs, use_graph=use_graph, steps_per_graph=group, stop=crit)
    assert eng.last_steps_run == STEPS, "the steps went on after the rows had finished"
    assert eng.last_finish_reasons.tolist() == [S.STOP_TOKEN] * B
    aut = R.lists(a)
    for i in range(B):
        n = int(eng.last_lengths[i])
        valid = _spelled_choice(first[i].item(), toks[i].tolist(), n, CHOICES)
        assert toks[i].tolist()[n:] == [1] * (STEPS - n)
        assert rows.states[i].item() == R.walk(aut, 0, valid) == end
    assert rows.accepted().tolist() == [True] * B and rows.error.item() == 0
    if bs is not None:
        assert eng.pool.error == 0


def test_first_token_choice():
    """Two single-token choices, ranks 3 and 7 of row 0's prefill distribution: the constrained prefill returns rank 3."""
    ids, lens = _prompts()
    eng = _engine()
    eng.prefill(ids, lens, logprobs=20)
    ranked = eng.first_logprobs.top_ids[0, 0].tolist()
    a = from_choices([[ranked[7]], [ranked[3]]], EOS)
    assert EOS not in ranked
    for sampling in (None, types.SimpleNamespace(temperature=0.0, top_p=1.0, repetition_penalty=1.0)):
        rows = ConstrainedRows(a, 0, B, DEV)
        first = eng.prefill(ids, lens, constraint=rows, sampling=sampling)
        assert first[0].item() == ranked[3]
        assert set(first.tolist()) <= {ranked[3], ranked[7]}
        assert rows.accepted().tolist() == [True] * B


# ------------------------------------------------------------------ sampling ----- #
@pytest.mark.parametrize("use_graph", [False, True])
def test_samples_stay_inside_their_own_choice_set(use_graph):
    """Two prompts x 4 samples on the shared paged pool, a choice set per prompt (a union, one start state per row), drawn
    at temperature 1.5 with a repetition penalty; every sample spells a choice of its own set, then EOS."""
    sets = [[[21, 22, 23], [21, 30], [40, 41], [50], [60, 61, 62, 63]], [[700, 1], [700, 2, 3], [800], [810, 5], [820]]]
    aut, starts = union([from_choices(c, EOS) for c in sets])
    sp = types.SimpleNamespace(temperature=1.5, top_p=0.95, repetition_penalty=1.1)
    crit = StopCriteria(stop_token_ids=[EOS], pad_token_id=1, check_every=2)
    ids, lens = _prompts()
    ids, lens = ids[:2].contiguous(), lens[:2].contiguous()
    torch.manual_seed(77)
    eng = _engine(16, share=True)
    rows = ConstrainedRows(aut, [starts[i // 4] for i in range(8)], 8, DEV)
    first = eng.prefill(ids, lens, sampling=sp, num_samples=4, constraint=rows)
    toks = eng.decode(first, STEPS, use_graph=use_graph, sampling=sp, stop=crit, logprobs=3, constraint=rows)
    assert eng.last_finish_reasons.tolist() == [S.STOP_TOKEN] * 8
    spelled = [tuple(_spelled_choice(first[i].item(), toks[i].tolist(), int(eng.last_lengths[i]), sets[i // 4]))
               for i in range(8)]
    print(f"graph={use_graph}: {len(set(spelled))} distinct continuations among the 8 samples")
    assert rows.accepted().tolist() == [True] * 8 and rows.error.item() == 0 and eng.pool.error == 0
    # the log-probabilities are the model's own: of the raw logits, so the forced tokens are rarely its favourites
    assert torch.all(eng.last_logprobs.chosen <= 0)


def test_sampled_steps_on_every_route():
    """temperature > 0 under the random automaton: mask, draw, advance inside the step, eager, captured and 4 steps per
    graph; every token is allowed and the states follow the tokens."""
    a = _half_automaton()
    aut = R.lists(a)
    sp = types.SimpleNamespace(temperature=0.8, top_p=0.9, repetition_penalty=1.2)
    for kw in (dict(use_graph=False), dict(use_graph=True), dict(use_graph=True, steps_per_graph=4)):
        torch.manual_seed(5)
        _, rows, first, toks = _run(a, prefill_kw=dict(sampling=sp), sampling=sp, **kw)
        walked = [R.walk(aut, 0, [f] + t) for f, t in zip(first.tolist(), toks.tolist())]
        assert None not in walked and rows.states.tolist() == walked, kw
        assert rows.error.item() == 0
        assert len({tuple(t) for t in toks.tolist()}) == B, "the rows do differ"


# ------------------------------------------------------------------ no residue, refusals ----- #
def test_no_residue():
    first0, toks0 = _plain(None, True)
    eng = _engine()
    ids, lens = _prompts()
    rows = ConstrainedRows(_half_automaton(), 0, B, DEV)
    first = eng.prefill(ids, lens, constraint=rows)
    eng.decode(first, STEPS, constraint=rows)
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, STEPS)
    assert torch.equal(first, first0) and torch.equal(toks, toks0)
    # and the same rows object serves another generation: prefill puts it back to its start states
    first = eng.prefill(ids, lens, constraint=rows)
    toks = eng.decode(first, STEPS, constraint=rows)
    _, rows2, first2, toks2 = _run(_half_automaton())
    assert torch.equal(first, first2) and torch.equal(toks, toks2) and torch.equal(rows.states, rows2.states)


def test_refusals():
    ids, lens = _prompts()
    eng = _engine()
    a = _half_automaton()
    with pytest.raises(ValueError, match="batch of 8"):
        eng.prefill(ids, lens, constraint=ConstrainedRows(a, 0, 4, DEV))
    first = eng.prefill(ids, lens)
    with pytest.raises(ValueError, match="batch of 8"):
        eng.decode(first, 4, constraint=ConstrainedRows(a, 0, 4, DEV))
    beyond = from_transitions({0: {5: 0, _model().geo.vocab_size: 0}})
    with pytest.raises(ValueError, match="outside the vocabulary"):
        eng.prefill(ids, lens, constraint=ConstrainedRows(beyond, 0, B, DEV))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        eng.decode(first, 4, constraint=ConstrainedRows(beyond, 0, B, DEV))
    # a set error word is reported
    rows = ConstrainedRows(a, 0, B, DEV)
    rows.error.fill_(1)
    with pytest.raises(RuntimeError, match="constrained decoding reported"):
        eng.decode(first, 2, constraint=rows)
