"""The stop kernel alone (csrc/decode_stop.hip through executor.stopping.stop_advance), driven step by step with given
``next_tokens`` and compared, after every step and exactly, with the plain-Python reference tests/_stop_ref.py.

The streams.  Alphabet 0 .. 5; stop id 5; stop sequences of 1, 2, 3 and 8 tokens that all end in 3 or 4, so a row that
draws from {0, 1, 2} alone starts matches all the time (every sequence's prefix lies in {0, 1, 2}) and can never complete
one.  A row is of one of four kinds: it draws from {0 .. 3, 5} (the stop id ends it, or a sequence by chance), it follows
a sequence token by token and breaks off with probability 0.25 per token (partial matches, re-starts, in the end a match),
it draws from {0, 1, 2} under a small ``max_tokens``, or it draws from {0, 1, 2} and never ends.  One token in 16 of the
prefill tokens is the stop id (length 0)."""

import random

import pytest
import torch

from lite_llama_amd import _lib as L
from lite_llama_amd.executor.stopping import StopCriteria, StopState, redirect_finished, stop_advance
from tests import _stop_ref as R

DEV = "cuda"
STEPS = 24
BATCHES = [1, 3, 64, 257]
PAD = 7
STOP_IDS = [5]
STOP_SEQS = [[4], [0, 3], [1, 1, 3], [0, 1, 0, 1, 2, 0, 1, 3]]
SAFE = [0, 1, 2]
NO_LIMIT = 1000            # a max_tokens the 24 steps never reach
TABLE_COLS = 48


def make_case(batch, seed):
    """-> (first tokens [B], streams [B][STEPS], max_tokens [B])."""
    rng = random.Random(seed)
    first, streams, max_tokens = [], [], []
    for _ in range(batch):
        kind = rng.choice(["id", "id", "seq", "seq", "seq", "max", "max", "never", "never"])
        first.append(5 if rng.random() < 1 / 16 else rng.choice(SAFE))
        limit = NO_LIMIT
        row = []
        if kind == "id":
            row = [rng.choice([0, 1, 2, 3, 5, 0, 1, 2]) for _ in range(STEPS)]
        elif kind == "seq":
            seq, k = rng.choice(STOP_SEQS[1:] + STOP_SEQS), 0
            while len(row) < STEPS:
                if rng.random() < 0.75:
                    row.append(seq[k])
                    k = (k + 1) % len(seq)
                else:
                    row.append(rng.choice(SAFE))
                    k = 0
        else:
            row = [rng.choice(SAFE) for _ in range(STEPS)]
            if kind == "max":
                limit = rng.randint(1, STEPS - 1)
        streams.append(row)
        max_tokens.append(limit)
    return first, streams, max_tokens


def reference_shares():
    """Over all rows of the random cases: the share that finishes by stop id, by stop sequence, by max_tokens, never."""
    counts, rows = [0, 0, 0, 0], 0
    for batch in BATCHES:
        first, streams, max_tokens = make_case(batch, seed=batch)
        _, _, reasons = R.apply(first, streams, STOP_IDS, STOP_SEQS, max_tokens, PAD)
        for r in reasons:
            counts[r] += 1
        rows += batch
    return [c / rows for c in counts]


def test_no_reason_goes_untested():
    never, by_id, by_seq, by_max = reference_shares()
    print(f"shares: stop id {by_id:.2f}, stop sequence {by_seq:.2f}, max_tokens {by_max:.2f}, never {never:.2f}")
    assert by_id >= 0.20 and by_seq >= 0.20 and by_max >= 0.10 and never >= 0.10


def _setup(batch, paged):
    first, streams, max_tokens = make_case(batch, seed=batch)
    rng = random.Random(1000 + batch)
    positions = [rng.randint(0, 9) for _ in range(batch)]
    seq_lens = [p + 1 for p in positions]
    req_idx = list(range(batch))
    rng.shuffle(req_idx)
    cur_select = None if paged else [100 + i for i in range(batch)]
    table = [[-1] * TABLE_COLS for _ in range(batch)]
    ref = R.StopRef(first, STOP_IDS, STOP_SEQS, max_tokens, PAD, positions, seq_lens, cur_select,
                    None if paged else req_idx, None if paged else table)
    crit = StopCriteria(stop_token_ids=STOP_IDS, stop_sequences=STOP_SEQS, max_tokens=max_tokens, pad_token_id=PAD)
    dev = dict(
        out=torch.full((batch, STEPS + 1), PAD, dtype=torch.int64, device=DEV),
        step=torch.ones(1, dtype=torch.int64, device=DEV),
        input_ids=torch.tensor(first, dtype=torch.int64, device=DEV).view(batch, 1),
        positions=torch.tensor(positions, dtype=torch.int64, device=DEV).view(batch, 1),
        b_seq_len=torch.tensor(seq_lens, dtype=torch.int32, device=DEV),
        b_req_idx=torch.tensor(req_idx, dtype=torch.int32, device=DEV),
        table=torch.tensor(table, dtype=torch.int32, device=DEV),
        cur_select=None if paged else torch.tensor(cur_select, dtype=torch.int32, device=DEV),
        nxt=torch.zeros(batch, dtype=torch.int64, device=DEV),
        streams=torch.tensor(streams, dtype=torch.int64, device=DEV),
    )
    dev["out"][:, 0] = dev["input_ids"].view(-1)
    state = StopState(crit, dev["input_ids"].view(-1), DEV)
    return ref, dev, state


def _launch(dev, state, paged):
    stop_advance(dev["out"], dev["step"], dev["nxt"], dev["input_ids"], dev["positions"], dev["cur_select"],
                 dev["b_seq_len"], None if paged else dev["b_req_idx"], None if paged else dev["table"], state)


def _check(ref, dev, state, paged, what):
    done = ref.step                                 # history columns written so far
    assert dev["step"].item() == ref.step, what
    assert dev["out"][:, :done].tolist() == ref.history, what
    assert torch.all(dev["out"][:, done:] == PAD), what          # nothing beyond the column of the step
    assert dev["input_ids"].view(-1).tolist() == ref.fed, what
    assert dev["positions"].view(-1).tolist() == ref.positions, what
    assert dev["b_seq_len"].tolist() == ref.seq_lens, what
    assert state.finished.tolist() == ref.finished, what
    assert state.lengths.tolist() == ref.lengths, what
    assert state.reasons.tolist() == ref.reasons, what
    assert state.running.tolist() == [ref.running], what
    if paged:
        assert torch.all(dev["table"] == -1), what                # rows and table are the pool's business
    else:
        assert dev["cur_select"].tolist() == ref.cur_select, what
        assert dev["table"].tolist() == ref.table, what


@pytest.mark.gpu
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("batch", BATCHES)
def test_every_step_equals_the_reference(batch, paged):
    ref, dev, state = _setup(batch, paged)
    _check(ref, dev, state, paged, "before the first step")      # a prefill token that is a stop id: finished, length 0
    columns = dev["streams"].t().tolist()
    for t in range(STEPS):
        dev["nxt"].copy_(dev["streams"][:, t])
        _launch(dev, state, paged)
        ref.advance(columns[t])
        _check(ref, dev, state, paged, f"batch {batch} paged {paged} step {t}")
    assert ref.step == STEPS + 1


@pytest.mark.gpu
@pytest.mark.parametrize("paged", [False, True])
def test_captured_step_replayed_equals_eager(paged):
    batch = 64
    ref, eager, e_state = _setup(batch, paged)
    for t in range(STEPS):
        eager["nxt"].copy_(eager["streams"][:, t])
        _launch(eager, e_state, paged)
    _, dev, state = _setup(batch, paged)
    graph = torch.cuda.CUDAGraph()
    with L.graph_capture(graph):                    # a capture executes nothing: the state is still the initial one
        _launch(dev, state, paged)
    for t in range(STEPS):
        dev["nxt"].copy_(dev["streams"][:, t])
        graph.replay()
    torch.cuda.synchronize()
    for name in ("out", "step", "input_ids", "positions", "b_seq_len", "table") + (() if paged else ("cur_select",)):
        assert torch.equal(dev[name], eager[name]), name
    for a, b in zip(state.tensors(), e_state.tensors()):
        assert torch.equal(a, b)
    assert state.lengths.tolist() == R.apply(eager["out"][:, 0].tolist(), eager["streams"].tolist(), STOP_IDS, STOP_SEQS,
                                             e_state.criteria.max_tokens, PAD)[1]


@pytest.mark.gpu
def test_finished_rows_are_redirected_to_the_junk_block():
    batch, block_size, junk = 70, 4, 4000
    _, dev, state = _setup(64, True)
    state.finished = (torch.arange(batch, device=DEV) % 3 == 0).to(torch.int32)
    rows = torch.arange(batch, dtype=torch.int32, device=DEV) + 10
    redirect_finished(rows, state, junk, block_size)
    want = [junk + i % block_size if i % 3 == 0 else 10 + i for i in range(batch)]
    assert rows.tolist() == want


@pytest.mark.gpu
def test_a_full_history_is_left_alone():
    """A launch with no column left (step == columns) changes nothing, the step counter included."""
    ref, dev, state = _setup(3, False)
    dev["step"].fill_(STEPS + 1)
    before = {k: v.clone() for k, v in dev.items() if v is not None}
    _launch(dev, state, False)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(dev[k], v), k
