"""CPU tier of constrained decoding: the plain-Python reference, the automaton builders and their validation, the C ABI
(header, ctypes table) and the coverage the kernel test's random cases must have -- shown by the reference alone."""

import itertools
import os
import re

import pytest
import torch

from lite_llama_amd.executor import (ConstrainedRows, TokenAutomaton, constrained_argmax, constraint_advance,
                                     constraint_mask, from_choices, from_transitions, union)
from tests import _constraint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 9


# ------------------------------------------------------------------ the reference itself ----- #
def test_reference_select_advance_walk():
    #        state 0: 2 -> 1, 5 -> 0, 7 -> 1        state 1: 3 -> 0
    aut = ([0, 3, 4], [2, 5, 7, 3], [1, 0, 1, 0])
    row = [0.0] * 8
    row[5], row[7], row[6] = 1.0, 1.0, 9.0                       # 6 is not allowed; 5 and 7 tie: the lower id
    assert R.select(aut, 0, row) == (5, 0)
    row[2] = 2.0
    assert R.select(aut, 0, row) == (2, 1)
    assert R.select(aut, 1, row) == (3, 0)
    dead = [R.NEG_INF] * 8
    assert R.select(aut, 0, dead) == (2, 1)                      # all -inf: the first edge
    assert R.advance(aut, 0, 7) == 1 and R.advance(aut, 0, 3) is None and R.advance(aut, 1, 3) == 0
    assert R.walk(aut, 0, [2, 3, 5, 7]) == 1 and R.walk(aut, 0, [2, 2]) is None and R.walk(aut, 1, []) == 1
    assert R.allowed(aut, 0) == [2, 5, 7]


# ------------------------------------------------------------------ validation ----- #
def test_automaton_validation():
    a = TokenAutomaton([0, 2, 3], [1, 4, 0], [1, 1, 0], accepting=[0, 1])
    assert (a.num_states, a.num_edges, a.max_degree, a.max_token) == (2, 3, 2, 4)
    assert a.offsets.dtype == a.tokens.dtype == a.next_states.dtype == torch.int32 and a.accepting.dtype == torch.uint8
    assert a.accepting.tolist() == [0, 1] and TokenAutomaton([0, 1], [0], [0]).accepting.tolist() == [0]
    with pytest.raises(ValueError, match="no edge"):
        TokenAutomaton([0, 2, 2, 3], [1, 4, 0], [1, 1, 0])       # an empty state
    with pytest.raises(ValueError, match="ascending"):
        TokenAutomaton([0, 2, 3], [4, 1, 0], [1, 1, 0])          # unsorted
    with pytest.raises(ValueError, match="ascending"):
        TokenAutomaton([0, 2, 3], [4, 4, 0], [1, 1, 0])          # duplicate
    with pytest.raises(ValueError, match="next states"):
        TokenAutomaton([0, 2, 3], [1, 4, 0], [1, 2, 0])          # next state out of range
    with pytest.raises(ValueError, match="next states"):
        TokenAutomaton([0, 2, 3], [1, 4, 0], [1, -1, 0])
    with pytest.raises(ValueError, match=">= 0"):
        TokenAutomaton([0, 2, 3], [-1, 4, 0], [1, 1, 0])
    with pytest.raises(ValueError, match="offsets"):
        TokenAutomaton([0, 2, 4], [1, 4, 0], [1, 1, 0])
    with pytest.raises(ValueError, match="accepting"):
        TokenAutomaton([0, 2, 3], [1, 4, 0], [1, 1, 0], accepting=[1])
    # a descent across a state boundary is fine
    assert TokenAutomaton([0, 1, 2], [7, 3], [1, 0]).num_states == 2
    a.validate(5)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        a.validate(4)


def test_from_transitions():
    a = from_transitions({0: {7: 1, 2: 0}, 1: {3: 0}}, accepting=[1])
    assert R.lists(a) == ([0, 2, 3], [2, 7, 3], [0, 1, 0]) and a.accepting.tolist() == [0, 1]
    with pytest.raises(ValueError, match="no edge"):
        from_transitions({0: {7: 1}})                            # state 1 is named and has nothing
    with pytest.raises(ValueError, match="no edge"):
        from_transitions({0: {7: 0}, 1: {}})
    with pytest.raises(ValueError, match="accepting"):
        from_transitions({0: {7: 0}}, accepting=[1])


def test_rows_validation():
    a = from_transitions({0: {7: 1, 2: 0}, 1: {3: 0}}, accepting=[1])
    rows = ConstrainedRows(a, [0, 1, 1], 3, "cpu")
    assert rows.states.dtype == torch.int32 and rows.states.tolist() == [0, 1, 1] and rows.error.tolist() == [0]
    assert rows.accepted().tolist() == [False, True, True]
    rows.states.fill_(0)
    rows.error.fill_(1)
    rows.reset()
    assert rows.states.tolist() == [0, 1, 1] and rows.error.tolist() == [0]
    assert ConstrainedRows(a, 1, 2, "cpu").states.tolist() == [1, 1]
    with pytest.raises(ValueError, match="batch of 3"):
        ConstrainedRows(a, [0, 1], 3, "cpu")
    with pytest.raises(ValueError, match="start state"):
        ConstrainedRows(a, [0, 2, 0], 3, "cpu")
    with pytest.raises(ValueError, match="batch of 4"):
        rows.validate(8, 4)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        rows.validate(7, 3)
    rows.validate(8, 3)


def test_wrappers_validate_before_launch():
    a = from_transitions({0: {7: 1, 2: 0}, 1: {3: 0}})
    rows = ConstrainedRows(a, 0, 2, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        constrained_argmax(torch.zeros(2, 8), rows)
    with pytest.raises(RuntimeError, match="GPU only"):
        constraint_mask(torch.zeros(2, 8), rows)
    with pytest.raises(RuntimeError, match="GPU only"):
        constraint_advance(rows, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="rows"):
        constrained_argmax(torch.zeros(3, 8), rows)
    with pytest.raises(ValueError, match="batch, vocab"):
        constraint_mask(torch.zeros(2, 1, 8), rows)


# ------------------------------------------------------------------ from_choices, through the reference ----- #
def _spelled(aut, max_len):
    """Every token sequence of ``max_len`` tokens that the automaton allows from state 0."""
    out = []

    def go(state, seq):
        if len(seq) == max_len:
            out.append(tuple(seq))
            return
        for t in R.allowed(aut, state):
            go(R.advance(aut, state, t), seq + [t])

    go(0, [])
    return out


def test_from_choices_spells_the_choices_then_eos_forever():
    choices = [[1, 2, 3], [1, 2], [4], [5, 1], [4], [1, 2, 3]]  # a prefix of another choice; duplicates
    a = from_choices(choices, EOS)
    aut = R.lists(a)
    n = 6
    want = {tuple(c) + (EOS,) * (n - len(c)) for c in choices}
    got = _spelled(aut, n)
    assert len(got) == len(set(got)) == 4 and set(got) == want
    # states: the root, one per distinct prefix (1, 1 2, 1 2 3, 4, 5, 5 1) and END, which only loops on EOS
    assert a.num_states == 8
    end = a.num_states - 1
    assert R.allowed(aut, end) == [EOS] and R.advance(aut, end, EOS) == end
    # accepting: exactly the choice-end nodes and END; the prefix's end node allows both going on and EOS
    for seq, acc in (([], False), ([1], False), ([1, 2], True), ([1, 2, 3], True), ([5], False), ([5, 1], True),
                     ([4], True), ([4, EOS], True), ([1, 2, EOS, EOS], True)):
        assert bool(a.accepting[R.walk(aut, 0, seq)]) == acc, seq
    assert R.allowed(aut, R.walk(aut, 0, [1, 2])) == [3, EOS]
    assert R.walk(aut, 0, [1, 2, EOS]) == end and R.walk(aut, 0, [2]) is None and R.walk(aut, 0, [EOS]) is None
    # duplicates change nothing
    assert R.lists(from_choices([[1, 2, 3], [1, 2], [4], [5, 1]], EOS)) == aut


def test_from_choices_refusals():
    with pytest.raises(ValueError, match="eos_token_id"):
        from_choices([[1, 2], [3, EOS]], EOS)
    with pytest.raises(ValueError, match="empty"):
        from_choices([[1], []], EOS)
    with pytest.raises(ValueError, match="at least one"):
        from_choices([], EOS)


def test_union_start_states():
    a = from_choices([[1, 2], [3]], EOS)
    b = from_transitions({0: {7: 1, 2: 0}, 1: {3: 0}}, accepting=[1])
    c = from_choices([[6]], EOS)
    u, starts = union([a, b, c])
    assert starts == [0, a.num_states, a.num_states + b.num_states]
    assert u.num_states == a.num_states + b.num_states + c.num_states
    assert u.num_edges == a.num_edges + b.num_edges + c.num_edges
    aut = R.lists(u)
    for part, s0 in zip((a, b, c), starts):
        p = R.lists(part)
        for state in range(part.num_states):                    # the same edges, next states shifted by the start
            assert R.allowed(aut, s0 + state) == R.allowed(p, state)
            assert [R.advance(aut, s0 + state, t) for t in R.allowed(p, state)] == \
                [s0 + R.advance(p, state, t) for t in R.allowed(p, state)]
        assert u.accepting[s0:s0 + part.num_states].tolist() == part.accepting.tolist()
    assert R.walk(aut, starts[2], [6, EOS, EOS]) == u.num_states - 1 and R.walk(aut, starts[2], [1]) is None


# ------------------------------------------------------------------ C ABI ----- #
def test_abi_declares_and_exports_the_constraint_kernels():
    from lite_llama_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lite_llama_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(ll_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name, nargs in (("ll_constrained_argmax", 14), ("ll_constraint_mask", 13), ("ll_constraint_advance", 10)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(name + r"\s*\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == nargs == len(_lib.SIGNATURES[name]), name


# ------------------------------------------------------------------ coverage of the kernel test's random cases ----- #
def test_random_cases_cover_ties_degrees_and_dead_rows():
    tied, one, wide, dead = R.coverage()
    print(f"shares over the random cases: tied maximum {tied:.2f}, degree 1 {one:.2f}, degree > 256 {wide:.2f}; "
          f"rows with every candidate at -inf: {dead}")
    assert tied >= 0.20 and one >= 0.10 and wide >= 0.10 and dead >= 1
    # every degree of the list occurs among the states the rows sit in
    aut = R.random_automaton()
    seen = {len(R.allowed(aut, s)) for b, d in itertools.product(R.BATCHES, R.DTYPES) for s in R.make_case(b, d)[0]}
    assert seen == set(R.DEGREES)
