"""DecodeEngine.prefill / decode with ``top_k`` / ``min_p`` on the sampling parameters: every route draws through the filtered
sampler.  On a synthetic model; every check reads the step's own log-probabilities (``logprobs = 20``: the model's own
distribution, ordered by logit descending), so it holds whatever the model says.  ``repetition_penalty`` is 1.0 throughout:
the filters then act on the very logits the log-probabilities describe."""

import functools
import math
import random
import types

import pytest
import torch

from lite_llama_amd.executor import ConstrainedRows, DecodeEngine, from_transitions
from tests import _constraint_ref as C
from tests.test_chunked_prefill_gpu import _random_model

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
    lens = [33, 17, 40, 25, 32, 19, 38, 28]
    ids = torch.randint(0, _model().geo.vocab_size, (B, max(lens)), generator=g)
    for i, n in enumerate(lens):
        ids[i, n:] = 0
    return ids.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _half_automaton():
    """16 states, each allowing a seeded random half of the 1024 tokens, with random next states."""
    rng = random.Random(16)
    return from_transitions({s: {t: rng.randrange(16) for t in rng.sample(range(1024), 512)} for s in range(16)})


# route name -> (engine kwargs, prefill kwargs, decode kwargs, constrained)
ROUTES = {
    "eager": (dict(), dict(), dict(use_graph=False), False),
    "graph": (dict(), dict(), dict(use_graph=True), False),
    "4-steps-per-graph": (dict(), dict(), dict(use_graph=True, steps_per_graph=4), False),
    "paged-eager": (dict(kv_block_size=16), dict(), dict(use_graph=False), False),
    "paged-graph": (dict(kv_block_size=16), dict(), dict(use_graph=True), False),
    "chunked-prefill": (dict(), dict(chunk_size=16), dict(use_graph=True), False),
    "shared-prefix": (dict(), dict(shared_prefix=True), dict(use_graph=True), False),
    "num-samples": (dict(kv_block_size=16, kv_share_blocks=True), dict(num_samples=4), dict(use_graph=True), False),
    "constraint-eager": (dict(), dict(), dict(use_graph=False), True),
    "constraint-graph": (dict(kv_block_size=16), dict(), dict(use_graph=True, steps_per_graph=4), True),
}


def _sp(**kw):
    return types.SimpleNamespace(repetition_penalty=1.0, **kw)


def _run(route, sp, seed=3):
    """Prefill + decode along ``route`` with ``sp``: per row the emitted tokens ``[1 + STEPS]`` and, aligned with them,
    ``chosen``, ``top_logprobs [.., 20]`` and ``top_ids [.., 20]``; and the automaton (lists) when the route has one."""
    eng_kw, pre_kw, dec_kw, constrained = ROUTES[route]
    eng = DecodeEngine(_model(), max_batch=B, max_seq_len=MAX_SEQ, **eng_kw)
    ids, lens = _prompts()
    if "num_samples" in pre_kw:
        ids, lens = ids[:2].contiguous(), lens[:2].contiguous()
    pre_kw = dict(pre_kw)
    if pre_kw.pop("shared_prefix", False):
        g = torch.Generator().manual_seed(5)
        pre_kw["shared_prefix_ids"] = torch.randint(0, _model().geo.vocab_size, (80,), generator=g).to(DEV)
        ids = torch.randint(0, _model().geo.vocab_size, (B, 6), generator=g).to(DEV)
        lens = torch.tensor([6, 3, 5, 6, 1, 4, 6, 2], dtype=torch.int32, device=DEV)
    rows = ConstrainedRows(_half_automaton(), 0, B, DEV) if constrained else None
    torch.manual_seed(seed)
    first = eng.prefill(ids, lens, sampling=sp, logprobs=20, constraint=rows, **pre_kw)
    assert first.shape == (B,)
    toks = eng.decode(first, STEPS, sampling=sp, logprobs=20, constraint=rows, **dec_kw)
    f, l = eng.first_logprobs, eng.last_logprobs
    out = types.SimpleNamespace(
        tokens=torch.cat([first.view(B, 1), toks], dim=1).cpu(), chosen=torch.cat([f.chosen, l.chosen], dim=1).cpu(),
        top=torch.cat([f.top_logprobs, l.top_logprobs], dim=1).cpu(), ids=torch.cat([f.top_ids, l.top_ids], dim=1).cpu(),
        automaton=C.lists(_half_automaton()) if constrained else None)
    if rows is not None:
        assert rows.error.item() == 0
    return out


def _candidates(run):
    """Per row and step: the emitted token, its own log-probability, and the log-probabilities and the ids of the step's top
    20 that the row's automaton state allowed (all 20 without a constraint), best first."""
    for i in range(B):
        state = 0
        for c in range(STEPS + 1):
            tok = int(run.tokens[i, c])
            top, ids = run.top[i, c].tolist(), run.ids[i, c].tolist()
            if run.automaton is not None:
                ok = set(C.allowed(run.automaton, state))
                assert tok in ok, (i, c)
                top, ids = [lp for lp, t in zip(top, ids) if t in ok], [t for t in ids if t in ok]
                state = C.advance(run.automaton, state, tok)
            yield (i, c), tok, float(run.chosen[i, c]), top, ids


@pytest.mark.parametrize("route", list(ROUTES))
def test_top_k_keeps_every_token_inside_the_five_best(route):
    """top_k = 5 at temperature 5 and top_p = 1: every emitted token is at least as likely as the fifth best (allowed) one.
    Without the filter a draw at T = 5 from 1024 tokens lands outside the best five almost every time."""
    run = _run(route, _sp(temperature=5.0, top_p=1.0, top_k=5))
    seen = set()
    for where, tok, chosen, top, ids in _candidates(run):
        # fewer than 5 allowed tokens among the step's top 20 (probability 0.6 % under the half automaton): no bound to read
        if len(top) >= 5:
            assert chosen >= top[4], (route, where, chosen, top[:6])
        seen.add(tok)
    assert len(seen) > 2 * B, "the draws do vary"


@pytest.mark.parametrize("route", list(ROUTES))
def test_min_p_keeps_every_token_above_the_floor(route):
    """min_p = 0.2 at temperature T: p_i / p_max = exp((l_i - l_max) / T) >= 0.2, i.e. the log-probabilities differ by at
    most T ln 5 (1e-3 for the fp32 of the log-softmax).  T = 0.5 puts the floor 0.8 nats below the best token, where the
    synthetic model's nearly flat distribution (a typical token lies 1.4 nats below its best) sends most unfiltered draws
    beneath it."""
    t = 0.5
    run = _run(route, _sp(temperature=t, top_p=1.0, min_p=0.2))
    spread = []
    for where, tok, chosen, top, ids in _candidates(run):
        if top:
            assert chosen - top[0] >= t * math.log(0.2) - 1e-3, (route, where, chosen, top[0])
            spread.append(top[0] - chosen)
    assert max(spread) > 0, "not every draw is the maximum"


@pytest.mark.parametrize("route", list(ROUTES))
def test_top_k_one_is_the_argmax(route):
    """top_k = 1 at temperature 5: the best (allowed) token wherever the two best differ."""
    run = _run(route, _sp(temperature=5.0, top_p=1.0, top_k=1))
    for where, tok, chosen, top, ids in _candidates(run):
        if len(top) >= 2 and top[0] != top[1]:
            assert tok == ids[0], (route, where, tok, ids[:3])


@pytest.mark.parametrize("route", ["eager", "graph", "4-steps-per-graph", "num-samples", "constraint-graph"])
def test_filters_off_draw_what_was_always_drawn(route):
    """A parameter object without the attributes, with both at their off values, and with ``top_k`` at the vocabulary size
    (off, by the filtered sampler's own rule): the same tokens under the same ``torch.manual_seed``."""
    base = _run(route, _sp(temperature=1.2, top_p=0.9), seed=5).tokens
    assert torch.equal(_run(route, _sp(temperature=1.2, top_p=0.9, top_k=0, min_p=0.0), seed=5).tokens, base)
    assert torch.equal(_run(route, _sp(temperature=1.2, top_p=0.9, top_k=_model().geo.vocab_size, min_p=0.0), seed=5).tokens, base)
    assert not torch.equal(_run(route, _sp(temperature=1.2, top_p=0.9, top_k=2), seed=5).tokens, base)
