"""The two launches of csrc/speculative.hip, exact against the plain-Python reference (tests/_spec_ref.py): the draft rule
at its edges and sizes (history lengths around the wave, the workgroup and the LDS staging switch; batches 1, 3, 65; token
ids up to 151 935) and the accept rule (every ``a`` for every ``d``, stops and cuts inside an accepted run, frozen rows,
the running count; batches 1, 3, 257)."""

import random

import pytest
import torch

from lite_llama_amd.executor import LDS_HISTORY_TOKENS, SpecState, Speculation, StopCriteria, spec_accept, spec_draft
from tests import _spec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 151935


def _state(histories, k, max_new, max_seq_len, emitted=None, finished=None, max_tokens=None, stop_ids=(), predicted=None,
           pred_lens=None, **rule):
    """A SpecState whose rows hold ``histories`` (the last token of each plays the prefill's token)."""
    b = len(histories)
    width = max(len(h) for h in histories) - 1
    prompts = torch.zeros(b, max(width, 1), dtype=torch.long)
    for i, h in enumerate(histories):
        prompts[i, :len(h) - 1] = torch.tensor(h[:-1], dtype=torch.long)
    lens = torch.tensor([len(h) - 1 for h in histories], dtype=torch.int32)
    first = torch.tensor([h[-1] for h in histories], dtype=torch.long)
    pred = None
    if predicted is not None:
        p = max(len(x) for x in predicted)
        pred = torch.zeros(b, p, dtype=torch.long)
        for i, x in enumerate(predicted):
            pred[i, :len(x)] = torch.tensor(x, dtype=torch.long)
        if pred_lens is None:
            pred_lens = [len(x) for x in predicted]
    spec = Speculation(num_draft_tokens=k, predicted_ids=pred,
                       predicted_lens=None if pred is None else torch.tensor(pred_lens, dtype=torch.int32), **rule)
    stop = None
    if stop_ids or max_tokens is not None:
        stop = StopCriteria(stop_token_ids=list(stop_ids), max_tokens=max_tokens)
    st = SpecState(spec, stop, prompts.to(DEV), lens.to(DEV), first.to(DEV), max_new, max_seq_len, DEV)
    if emitted is not None:
        st.emitted.copy_(torch.tensor(emitted, dtype=torch.int32))
        st.lengths.copy_(st.emitted)
    if finished is not None:
        st.finished.copy_(torch.tensor(finished, dtype=torch.int32))
    return st


def _check_draft(histories, k, max_new=64, max_seq_len=64, emitted=None, finished=None, max_tokens=None, predicted=None,
                 pred_lens=None, **rule):
    b = len(histories)
    st = _state(histories, k, max_new, max_seq_len, emitted, finished, max_tokens, (), predicted, pred_lens, **rule)
    st.ids.fill_(-7)
    st.positions.fill_(-7)
    spec_draft(st)
    torch.cuda.synchronize()
    ids, pos, q, ctx = st.ids.cpu().tolist(), st.positions.cpu().tolist(), st.q_len.cpu().tolist(), st.ctx_len.cpu().tolist()
    for i in range(b):
        want = R.draft_step(list(histories[i]), 0 if emitted is None else emitted[i],
                            bool(finished[i]) if finished is not None else False, k, max_new,
                            None if max_tokens is None else max_tokens[i], max_seq_len,
                            predicted=None if predicted is None else predicted[i],
                            pred_len=None if predicted is None else (len(predicted[i]) if pred_lens is None else pred_lens[i]),
                            **rule)
        assert (ids[i], pos[i], q[i], ctx[i]) == want, (i, histories[i][-8:], (ids[i], pos[i], q[i], ctx[i]), want)
        assert max(pos[i]) < max_seq_len
    return q


def test_draft_cases():
    hs = [[7],                                   # hist_len < n
          [7, 7],
          [1, 2, 3, 9, 1, 2, 3],                 # a match ending at e = n
          [5, 1, 5, 2, 5, 3, 5],                 # several matches: the latest wins
          [4, 6, 4],                             # a continuation shorter than k
          [1, 2, 1, 2, 1, 2],                    # the periodic overlap
          [1, 2, 3, 4],                          # no match
          [BIG, 5, BIG - 1, BIG, 5]]             # large ids
    q = _check_draft(hs, 4)
    assert q == [1, 2, 5, 3, 3, 3, 1, 4]
    _check_draft(hs, 15)
    _check_draft(hs, 1)
    _check_draft(hs, 4, max_ngram=1)
    _check_draft(hs, 4, max_ngram=5, min_ngram=2)
    assert set(_check_draft(hs, 4, ngram=False)) == {1}


def test_draft_prediction_cases():
    pred = [1, 0, 1, 0, 1, 0, 1, 5]
    cases = [  # history, emitted, prediction
        ([1, 2, 7, 1, 2], 0, [1, 2, 5, 6]),           # the prediction wins at equal n
        ([3, 1, 2, 7, 3, 1, 2], 0, [0, 2, 5, 6]),     # a longer n in the history beats a shorter one in the prediction
        ([9, 8, 1, 2], 0, [3, 1, 2]),                 # nothing follows a match at the prediction's end
        ([4, 3, 3], 0, [3, 5]),                       # nothing matches across the seam
        ([6, 1], 3, pred), ([6, 1], 4, pred), ([6, 1], 6, pred),   # nearest to emitted; ties to the larger end
        ([6, 5], 0, pred),
        ([6, BIG], 2, [BIG, BIG - 1, BIG, 4]),
    ]
    hs, em, pr = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    q = _check_draft(hs, 2, emitted=em, predicted=pr, max_ngram=2)
    assert q[0] == 3 and q[1] == 3
    assert _check_draft(hs, 2, emitted=em, predicted=pr, max_ngram=2, min_ngram=2)[3] == 1
    _check_draft(hs, 2, emitted=em, predicted=pr, max_ngram=2, ngram=False)
    _check_draft(hs, 2, emitted=em, predicted=pr, pred_lens=[min(3, len(p)) for p in pr], max_ngram=1)


def test_draft_limits_and_finished_rows():
    per = [1, 2] * 40
    hs = [per[:5], per[:5], per[:63], per[:62], per[:61], per[:5], per[:64]]
    em = [9, 2, 0, 0, 0, 5, 3]
    mt = [100, 3, 100, 100, 100, 100, 100]
    fin = [0, 0, 0, 0, 0, 1, 1]
    q = _check_draft(hs, 4, max_new=10, emitted=em, max_tokens=mt, finished=fin)
    # lim = 0 from remaining = 1 (max_new_tokens, max_tokens) and from the table row's end; then 1 and 2; finished rows
    assert q == [1, 1, 1, 2, 3, 0, 0]


@pytest.mark.parametrize("batch", [1, 3, 65])
def test_draft_sizes(batch):
    rng = random.Random(batch)
    switch = LDS_HISTORY_TOKENS
    lengths = [1, 63, 64, 65, 255, 256, 257, switch - 1, switch, switch + 1]
    alphabet = [0, 7, 65536, BIG - 1, BIG]
    s = switch + 40
    for trial in range(len(lengths) if batch == 1 else 2):
        hs, pr = [], []
        for i in range(batch):
            n = lengths[(trial + i) % len(lengths)] if batch < 65 else (lengths[i] if i < len(lengths) else rng.randrange(1, 300))
            if (i + trial) % 3 == 2 and n > 8:
                # the only match lies at the very start of the history: e = n, found by one thread of the first stride
                h = [1000 + j for j in range(n)]
                h[-3:] = h[:3]
            else:
                h = [rng.choice(alphabet) for _ in range(n)]
            hs.append(h)
            pr.append([rng.choice(alphabet) for _ in range(rng.randrange(1, 40))])
        em = [rng.randrange(0, 20) for _ in range(batch)]
        _check_draft(hs, 7, max_new=64, max_seq_len=s, emitted=em)
        _check_draft(hs, 7, max_new=64, max_seq_len=s, emitted=em, predicted=pr, max_ngram=4)


def _check_accept(st, argmax, k, max_new, max_tokens=None, stop_ids=()):
    b = st.batch
    before = [t.clone() for t in st.tensors()]
    rows = []
    hist, hl = st.history.cpu().tolist(), st.hist_len.cpu().tolist()
    out = st.out.cpu().tolist()
    fin, em = st.finished.cpu().tolist(), st.emitted.cpu().tolist()
    for i in range(b):
        rows.append(R.Row(history=hist[i][:hl[i]], emitted=em[i], finished=bool(fin[i]), length=em[i],
                          reason=int(st.reasons[i]), out=out[i][1:1 + em[i]], verify_steps=int(st.verify_steps[i]),
                          drafted=int(st.drafted[i]), accepted=int(st.accepted[i])))
    ids, q = st.ids.cpu().tolist(), st.q_len.cpu().tolist()
    am = argmax.view(b, k + 1).cpu().tolist()
    live = 0
    for i in range(b):
        live += R.accept_step(rows[i], ids[i], q[i], am[i], max_new, None if max_tokens is None else max_tokens[i], stop_ids)
    step0 = int(st.step)
    spec_accept(st, argmax.to(DEV))
    torch.cuda.synchronize()
    assert int(st.running) == live and int(st.step) == step0 + 1
    got_out, got_hist = st.out.cpu().tolist(), st.history.cpu().tolist()
    for i, r in enumerate(rows):
        if fin[i]:
            for t, was in zip(st.tensors(), before):
                if t.shape[0] == b and t is not st.cur_select_index and t is not st.running and t is not st.step:
                    assert torch.equal(t[i], was[i]), i        # a finished row is bit-unchanged
            continue
        assert got_out[i][1:1 + r.emitted] == r.out and got_out[i][0] == out[i][0], i
        assert got_out[i][1 + r.emitted:] == out[i][1 + r.emitted:], i                     # nothing written beyond
        assert got_hist[i][:len(r.history)] == r.history and int(st.hist_len[i]) == len(r.history), i
        assert (int(st.emitted[i]), int(st.lengths[i]), int(st.finished[i]), int(st.reasons[i])) == (
            r.emitted, r.length, int(r.finished), r.reason), i
        assert (int(st.verify_steps[i]), int(st.drafted[i]), int(st.accepted[i])) == (r.verify_steps, r.drafted, r.accepted), i
        assert int(st.accepted_per_step[i, step0]) == r.accepted_per_step[-1], i
    return rows


def _grid(st, rows_spec, k):
    """Set the step's grid: per row (d, a, tokens the model gives) -> ids / q_len and the argmax tensor."""
    b = st.batch
    am = torch.zeros(b, k + 1, dtype=torch.long)
    for i, (d, a) in enumerate(rows_spec):
        ids = [int(st.out[i, 0])] + [2000 + 16 * i + j for j in range(d)] + [0] * (k - d)
        row = [2000 + 16 * i + j for j in range(a)] + [BIG - i % 5] + [3000 + j for j in range(k - a)]
        st.ids[i].copy_(torch.tensor(ids))
        st.q_len[i] = 1 + d
        am[i] = torch.tensor(row[:k + 1])
    return am.view(-1)


@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("k", [1, 4, 15])
def test_accept_every_a_for_every_d(batch, k):
    pairs = [(d, a) for d in range(k + 1) for a in range(d + 1)]
    for start in range(0, len(pairs), batch):
        spec = [pairs[(start + i) % len(pairs)] for i in range(batch)]
        hs = [[11 + i % 7, 5, 40 + i % 3] for i in range(batch)]
        fin = [1 if i % 11 == 10 else 0 for i in range(batch)]
        st = _state(hs, k, 40, 64, emitted=[i % 4 for i in range(batch)], finished=fin)
        st.step.fill_(3)
        am = _grid(st, spec, k)
        rows = _check_accept(st, am, k, 40)
        for (d, a), r, f in zip(spec, rows, fin):
            if not f:
                assert r.accepted_per_step[-1] == a and r.drafted == d


def test_accept_stops_and_cuts_inside_a_run():
    k = 4
    # a stop id at each kept position of a fully accepted run
    b = k + 1
    st = _state([[9, 8]] * b, k, 40, 64, stop_ids=[2000, 2017, 2034, 2051, BIG - 4])
    am = _grid(st, [(k, k)] * b, k)
    rows = _check_accept(st, am, k, 40, stop_ids=(2000, 2017, 2034, 2051, BIG - 4))
    assert [r.length for r in rows] == [1, 2, 3, 4, 5] and all(r.reason == 1 and r.finished for r in rows)
    assert int(st.running) == 0
    # max_tokens and max_new_tokens cut inside the run; the last out column is never overrun
    em = [0, 2, 5, 7, 9, 9]
    mt = [2, 3, 100, 9, 100, 10]
    st = _state([[9, 8]] * 6, k, 10, 64, emitted=em, max_tokens=mt)
    am = _grid(st, [(k, k)] * 6, k)
    guard = st.out.clone()
    rows = _check_accept(st, am, k, 10, max_tokens=mt)
    assert [r.length for r in rows] == [2, 3, 10, 9, 10, 10]
    assert [r.reason for r in rows] == [3, 3, 0, 3, 0, 3]
    assert st.out.shape == guard.shape and int(st.running) == 0
    # two steps in a row: the second continues where the first stopped, finished rows stay
    st = _state([[9, 8], [9, 8], [9, 8]], k, 6, 64, stop_ids=[BIG - 1])
    am = _grid(st, [(4, 2), (4, 0), (0, 0)], k)
    _check_accept(st, am, k, 6, stop_ids=(BIG - 1,))
    assert st.finished.cpu().tolist() == [0, 1, 0] and int(st.running) == 2
    am = _grid(st, [(4, 4), (4, 4), (2, 1)], k)
    rows = _check_accept(st, am, k, 6, stop_ids=(BIG - 1,))
    assert [r.length for r in rows] == [6, 1, 3] and int(st.running) == 1
    assert st.accepted_per_step[:, :2].cpu().tolist() == [[2, 2], [0, -1], [0, 1]]
