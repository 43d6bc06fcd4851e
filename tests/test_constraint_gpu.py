"""The three launches of csrc/constrained.hip alone, exact against the plain-Python reference tests/_constraint_ref.py, and
the nucleus sampler on masked logits: a disallowed token is never drawn."""

import functools
import random

import pytest
import torch

from lite_llama_amd.executor import (ConstrainedRows, TokenAutomaton, constrained_argmax, constraint_advance,
                                     constraint_mask)
from lite_llama_amd.sampling import sample_top_p
from tests import _constraint_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG_VOCAB = 152064


@functools.lru_cache(maxsize=None)
def _automaton():
    off, tok, nxt = R.random_automaton()
    return TokenAutomaton(off, tok, nxt).to(DEV)


def _rows(states, automaton=None):
    rows = ConstrainedRows(automaton or _automaton(), 0, len(states), DEV)
    rows.states.copy_(torch.tensor(states, dtype=torch.int32))
    return rows


# ------------------------------------------------------------------ greedy kernel ----- #
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("batch", R.BATCHES)
def test_constrained_argmax_random_cases(batch, dtype):
    states, logits, finished, tokens, new_states = R.make_case(batch, dtype)
    z = torch.tensor(logits, dtype=torch.float32).to(getattr(torch, dtype)).to(DEV)
    assert torch.equal(z.float().cpu(), torch.tensor(logits)), "the values are exact in the dtype"
    fin = torch.tensor(finished, dtype=torch.int32, device=DEV)
    # packed rows, and a view whose row stride is larger than the vocabulary (the step passes logits[:, -1, :])
    wide = torch.full((batch, R.VOCAB + 40), 7.0, dtype=z.dtype, device=DEV)
    wide[:, :R.VOCAB] = z
    for what, view in (("packed", z), ("strided", wide[:, :R.VOCAB])):
        assert what == "packed" or view.stride(0) > R.VOCAB
        rows = _rows(states)
        got = constrained_argmax(view, rows, fin)
        assert got.dtype == torch.int64 and got.shape == (batch,)
        live = [i for i in range(batch) if not finished[i]]
        emitted = got.tolist()
        assert [emitted[i] for i in live] == [tokens[i] for i in live], what
        assert rows.states.tolist() == new_states, what
        assert rows.error.item() == 0
    # without finished: every row moves
    rows = _rows(states)
    got = constrained_argmax(z, rows)
    aut = R.random_automaton()
    assert got.tolist() == tokens
    assert rows.states.tolist() == [R.advance(aut, s, t) for s, t in zip(states, tokens)]


@functools.lru_cache(maxsize=None)
def _big_logits():
    g = torch.Generator().manual_seed(21)
    z = (torch.randn(3, BIG_VOCAB, generator=g) * 2).half()      # fp16: exact ties at the top are common
    z[1, 100000:] = z[1].max()                                   # a long run of tied maxima late in the row
    return z


@pytest.mark.parametrize("degree", [5000, BIG_VOCAB])
def test_constrained_argmax_full_vocabulary(degree):
    """Vocabulary 152 064: two states, of ``degree`` edges and of one; every row starts in state 0."""
    z = _big_logits()
    rng = random.Random(degree)
    toks = sorted(rng.sample(range(BIG_VOCAB), degree))
    a = TokenAutomaton([0, degree, degree + 1], toks + [17], [rng.randrange(2) for _ in toks] + [0])
    assert a.max_degree == degree
    aut = R.lists(a)
    want = [R.select(aut, 0, row) for row in z.float().tolist()]
    rows = _rows([0, 0, 0], a.to(DEV))
    got = constrained_argmax(z.to(DEV), rows)
    assert got.tolist() == [w[0] for w in want] and rows.states.tolist() == [w[1] for w in want]
    if degree == BIG_VOCAB:                                      # everything allowed: the plain first argmax
        assert got.tolist() == torch.argmax(z.float(), dim=-1).tolist()
    assert rows.error.item() == 0


def test_a_state_outside_the_automaton_is_reported():
    rows = _rows([0, R.NUM_STATES, 1])
    got = constrained_argmax(torch.zeros(3, R.VOCAB, device=DEV), rows)
    assert rows.error.item() == 2 and rows.states[1].item() == R.NUM_STATES and got[1].item() == 0


# ------------------------------------------------------------------ mask kernel ----- #
def _torch_mask(z, aut, states):
    keep = torch.zeros(z.shape, dtype=torch.bool)
    for i, s in enumerate(states):
        keep[i, R.allowed(aut, s)] = True
    return torch.where(keep.to(z.device), z, torch.full_like(z, float("-inf")))


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("batch,vocab", [(1, 1024), (64, 1024), (5, 1030), (3, 9001), (3, 9008)])
def test_constraint_mask_is_bit_exact(batch, vocab, dtype):
    """Against torch.where; rows that do and do not start on the 16-byte stores' boundary, one chunk and two."""
    dt = getattr(torch, dtype)
    aut = R.random_automaton(seed=vocab, vocab=vocab)
    a = TokenAutomaton(*aut).to(DEV)
    g = torch.Generator().manual_seed(batch)
    z = torch.randn(batch, vocab, generator=g).to(dt).to(DEV)
    z[0, ::7] = float("-inf")
    z[-1, 3] = float("nan")                                      # payloads travel too
    states = [(5 * i + 3) % R.NUM_STATES for i in range(batch)]
    rows = _rows(states, a)
    want = _torch_mask(z, aut, states)
    bits = torch.int32 if dt == torch.float32 else torch.int16
    for what, view in (("packed", z), ("strided", torch.cat([z, z], dim=1)[:, :vocab])):
        got = constraint_mask(view, rows)
        assert got.dtype == dt and got.shape == z.shape and got.data_ptr() != view.data_ptr()
        assert torch.equal(got.view(bits), want.view(bits)), what
    assert rows.states.tolist() == states and rows.error.item() == 0


# ------------------------------------------------------------------ sampling on masked logits ----- #
UNIFORMS = [0.0, 0.5, 1.0 - 2.0 ** -24] + [(i + 0.5) / 61 for i in range(61)]


@functools.lru_cache(maxsize=None)
def _sampling_case():
    """One automaton whose states allow 1, 2, 65 and 1024 tokens.  The allowed sets of the first three end well before the
    last token of the vocabulary -- within the first tenth of it and so inside the first two of the sampler's 16 segments,
    with disallowed tokens after them in their segment: the case a fallback to "the last kept token" can get wrong."""
    vocab = 4096
    rng = random.Random(8)
    offsets, tokens, nxt = [0], [], []
    for s, degree in enumerate((1, 2, 65, 1024)):
        toks = sorted(rng.sample(range(vocab // 10 if degree < 1024 else vocab - 50), degree))
        tokens += toks
        nxt += [rng.randrange(4) for _ in toks]
        offsets.append(len(tokens))
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(4, vocab, generator=g) * 3).half()
    return (offsets, tokens, nxt), z, vocab


@pytest.mark.parametrize("temperature", [0.7, 1.5])
@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_sampling_never_leaves_the_allowed_set(top_p, temperature):
    aut, z, vocab = _sampling_case()
    a = TokenAutomaton(*aut).to(DEV)
    n = len(UNIFORMS)
    states = [s for s in range(4) for _ in range(n)]             # every state at every uniform number
    logits = z.to(DEV)[torch.tensor(states)].contiguous()
    u = torch.tensor(UNIFORMS * 4, dtype=torch.float32, device=DEV)
    assert u.max().item() < 1.0
    rows = _rows(states, a)
    masked = constraint_mask(logits, rows)
    drawn = sample_top_p(masked, temperature, top_p, u).view(-1)
    # bit for bit the draw from a mask built by torch
    assert torch.equal(drawn, sample_top_p(_torch_mask(logits, aut, states), temperature, top_p, u).view(-1))
    constraint_advance(rows, drawn)
    assert rows.error.item() == 0, "every drawn token is allowed"
    got = drawn.tolist()
    for i, (s, t) in enumerate(zip(states, got)):
        assert t in R.allowed(aut, s), (s, UNIFORMS[i % n], t)
    assert rows.states.tolist() == [R.advance(aut, s, t) for s, t in zip(states, got)]
    assert set(got[:n]) == {R.allowed(aut, 0)[0]}, "a degree-1 state emits its token for every uniform number"
    assert len(set(got[3 * n:])) > 3, "the draws do spread over a wide state"


# ------------------------------------------------------------------ advance kernel ----- #
@pytest.mark.parametrize("batch", [1, 64, 257])
def test_constraint_advance(batch):
    aut = R.random_automaton()
    rng = random.Random(batch)
    states = [rng.randrange(R.NUM_STATES) for _ in range(batch)]
    toks = [rng.choice(R.allowed(aut, s)) for s in states]
    finished = [1 if rng.random() < 0.2 else 0 for _ in range(batch)]
    rows = _rows(states)
    constraint_advance(rows, torch.tensor(toks, device=DEV), torch.tensor(finished, dtype=torch.int32, device=DEV))
    assert rows.states.tolist() == [s if f else R.advance(aut, s, t) for s, t, f in zip(states, toks, finished)]
    assert rows.error.item() == 0
    # one absent token: the error word is set, that row's state stays, the others move
    rows = _rows(states)
    bad = batch // 2
    toks[bad] = next(t for t in range(R.VOCAB) if t not in R.allowed(aut, states[bad]))
    constraint_advance(rows, torch.tensor(toks, device=DEV))
    want = [R.advance(aut, s, t) for s, t in zip(states, toks)]
    assert want[bad] is None
    want[bad] = states[bad]
    assert rows.states.tolist() == want and rows.error.item() == 1
    # an absent token of a finished row is nobody's business
    rows = _rows(states)
    fin = [0] * batch
    fin[bad] = 1
    constraint_advance(rows, torch.tensor(toks, device=DEV), torch.tensor(fin, dtype=torch.int32, device=DEV))
    assert rows.states.tolist() == want and rows.error.item() == 0
    rows.error.fill_(1)
    rows.reset()
    assert rows.error.item() == 0 and rows.states.tolist() == [0] * batch
