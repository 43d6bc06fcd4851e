"""Greedy speculative decoding without a device: the plain-Python reference (tests/_spec_ref.py) -- the draft rule at its
edges, the accept rule, and the whole-loop simulator, which must return plain greedy decoding whatever is drafted -- and
the validation of ``Speculation``.  The GPU tests compare the kernels and the engine against this reference."""

import random

import pytest
import torch

from lite_llama_amd.executor import MAX_DRAFT_TOKENS, MAX_NGRAM, Speculation
from tests import _spec_ref as R


def test_draft_rule_edges():
    # hist_len < n: only the n that fit are tried
    assert R.propose([7], 0, 4, max_ngram=3) == []
    assert R.propose([7, 7], 0, 4, max_ngram=3) == [7]              # n = 1, end 1, the draft overlaps the suffix
    # a match ending at e = n
    assert R.propose([1, 2, 3, 9, 1, 2, 3], 0, 2, max_ngram=3) == [9, 1]
    # several matches: the latest wins
    assert R.propose([5, 1, 5, 2, 5, 3, 5], 0, 1, max_ngram=1) == [3]
    # a continuation shorter than k
    assert R.propose([4, 6, 4], 0, 8, max_ngram=1) == [6, 4]
    # periodic text: the draft overlaps the suffix
    assert R.propose([1, 2, 1, 2, 1, 2], 0, 4, max_ngram=2) == [1, 2]
    assert R.propose([1, 2, 1, 2, 1, 2], 0, 4, max_ngram=3) == [1, 2]   # n = 3: the suffix 2, 1, 2 ends at 4 too
    # no match
    assert R.propose([1, 2, 3, 4], 0, 4) == []
    # min_ngram above what matches
    assert R.propose([5, 1, 5], 0, 4, max_ngram=3, min_ngram=2) == []
    # ngram off and no prediction: empty
    assert R.propose([5, 1, 5], 0, 4, ngram=False) == []


def test_prediction_rules():
    hist = [9, 8, 1, 2]
    # the prediction wins at equal n
    assert R.propose([1, 2, 7, 1, 2], 0, 2, max_ngram=2, predicted=[1, 2, 5, 6]) == [5, 6]
    # a longer n in the history beats a shorter one in the prediction
    assert R.propose([3, 1, 2, 7, 3, 1, 2], 0, 2, max_ngram=3, predicted=[0, 2, 5, 6]) == [7, 3]
    # nothing matches across the seam: the history ends 1, 2 and the prediction starts 3 -- (2, 3) is in neither text
    assert R.propose(hist, 0, 2, max_ngram=2, min_ngram=2, predicted=[3, 1, 2]) == []
    # ... the history ends 3, 3 and the prediction starts 3: the pair (3 | 3) spans the two texts
    assert R.propose([4, 3, 3], 0, 2, max_ngram=2, min_ngram=2, predicted=[3, 5]) == []
    # nearest to emitted, ties to the larger end
    pred = [1, 0, 1, 0, 1, 0, 1, 5]
    assert R.propose([6, 1], 3, 1, max_ngram=1, predicted=pred) == [0]       # ends 1, 3, 5, 7: 3 is aligned
    assert R.propose([6, 1], 4, 1, max_ngram=1, predicted=pred) == [0]       # 3 and 5 tie: 5 wins -> predicted[5]
    assert R.propose([6, 1], 6, 2, max_ngram=1, predicted=pred) == [5]       # 5 and 7 tie: 7 wins
    # a match at the prediction's very end (e = pred_len) is no candidate: nothing follows it
    assert R.propose([6, 5], 0, 2, max_ngram=1, ngram=False, predicted=pred) == []
    # predicted_lens cuts the text
    assert R.propose([6, 1], 0, 4, max_ngram=1, predicted=pred, pred_len=3) == [0, 1]


def test_draft_step_grid():
    ids, pos, q, ctx = R.draft_step([1, 2, 1, 2, 1], 0, False, 4, 10, None, 64)
    assert (ids, pos, q, ctx) == ([1, 2, 1, 0, 0], [4, 5, 6, 6, 6], 3, 4)    # pad positions clamped to ctx + d
    # lim = 0: remaining = 1, and the table row's end
    assert R.draft_step([1, 2, 1, 2, 1], 9, False, 4, 10, None, 64)[2] == 1
    assert R.draft_step([1, 2, 1, 2, 1], 2, False, 4, 10, 3, 64)[2] == 1
    assert R.draft_step([1, 2] * 31 + [1], 0, False, 4, 10, None, 64)[2] == 1
    assert R.draft_step([1, 2] * 30 + [1], 0, False, 4, 10, None, 64)[2] == 3  # 64 - 61 - 1 = 2 drafts
    # a finished row
    assert R.draft_step([1, 2, 1], 5, True, 2, 10, None, 64) == ([0, 0, 0], [2, 2, 2], 0, 2)


def test_accept_rule():
    for k in (1, 4):
        for d in range(k + 1):
            for a in range(d + 1):
                ids = [50] + [10 + j for j in range(d)] + [0] * (k - d)
                am = [10 + j for j in range(a)] + [99] + [7] * (k - a)
                row = R.Row(history=[50])
                assert R.accept_step(row, ids, 1 + d, am, 100)
                assert row.out == am[:a + 1] and row.history == [50] + am[:a + 1]
                assert (row.emitted, row.drafted, row.accepted, row.verify_steps) == (a + 1, d, a, 1)
    # a stop id inside the run: the finishing token is kept, the rest dropped
    row = R.Row(history=[50])
    assert not R.accept_step(row, [50, 1, 2, 3], 4, [1, 2, 3, 4], 100, stop_ids=(2,))
    assert (row.out, row.reason, row.length, row.accepted) == ([1, 2], 1, 2, 1)
    # max_tokens and max_new_tokens cut the run
    row = R.Row(history=[50], emitted=1, out=[8])
    assert not R.accept_step(row, [50, 1, 2, 3], 4, [1, 2, 3, 4], 100, max_tokens=3)
    assert (row.out, row.reason, row.length) == ([8, 1, 2], 3, 3)
    row = R.Row(history=[50], emitted=1, out=[8])
    assert not R.accept_step(row, [50, 1, 2, 3], 4, [1, 2, 3, 4], 2)
    assert (row.out, row.reason, row.finished) == ([8, 1], 0, True)
    # a finished row does not move
    before = R.Row(history=[1, 2], emitted=1, finished=True, length=1, reason=1, out=[2])
    assert not R.accept_step(before, [2, 3], 2, [3, 4], 100)
    assert (before.history, before.out, before.accepted_per_step) == ([1, 2], [2], [-1])


def _toy_model(seed, vocab=7):
    """A deterministic next-token function with short cycles (so that n-gram drafts hit) and some noise."""
    def next_token(seq):
        if len(seq) % 11 == seed % 11:
            return (seq[-1] * 3 + len(seq)) % vocab
        return (seq[-1] + seq[-2] if len(seq) > 1 else seq[-1] + 1) % vocab
    return next_token


def _greedy(next_token, prompt, first, n):
    seq, out = list(prompt) + [first], []
    for _ in range(n):
        out.append(next_token(seq))
        seq.append(out[-1])
    return out


@pytest.mark.parametrize("k", [1, 3, 7])
def test_simulator_returns_plain_greedy_for_any_drafts(k):
    rng = random.Random(k)
    for seed in range(6):
        model = _toy_model(seed)
        prompts = [[rng.randrange(7) for _ in range(rng.randrange(1, 9))] for _ in range(3)]
        firsts = [model(p) for p in prompts]
        n = 20
        want = [_greedy(model, p, f, n) for p, f in zip(prompts, firsts)]
        sources = {
            "ngram": {},
            "none": dict(ngram=False),
            "true": dict(predicted=want, ngram=False),
            "wrong": dict(predicted=[[(t + 1) % 7 for t in w] for w in want]),
            "random": dict(drafts=lambda i, s, h, lim: [rng.randrange(7) for _ in range(lim)]),
        }
        steps = {}
        for name, kw in sources.items():
            rows, steps[name] = R.simulate(model, prompts, firsts, n, k, 64, **kw)
            assert [r.out for r in rows] == want, (name, seed)
            for r in rows:
                assert r.accepted <= r.drafted and r.emitted == r.verify_steps + r.accepted == n
                assert all(0 <= a <= k for a in r.accepted_per_step if a >= 0)
        assert steps["none"] == n and steps["true"] < n
        # a recorded run replayed through the simulator gives the statistics of the run itself
        for name in ("ngram", "true"):
            kw = sources[name]
            rows, s = R.simulate(model, prompts, firsts, n, k, 64, **kw)
            again, s2 = R.replay(want, firsts, prompts, n, k, 64, **kw)
            assert s2 == s
            for r, q in zip(rows, again):
                assert (q.verify_steps, q.drafted, q.accepted) == (r.verify_steps, r.drafted, r.accepted)


@pytest.mark.parametrize("k", [1, 4, 15])
def test_true_prediction_is_fully_accepted(k):
    """A vocabulary large enough that no n-gram recurs by chance: the first step has nothing to align with (no returned
    token yet), every later one takes k + 1 tokens."""
    def model(seq):
        return (seq[-1] * 7919 + len(seq) * 104729 + 13) % 1000003

    prompt, n = [5, 6, 7], 33
    first = model(prompt)
    want = _greedy(model, prompt, first, n)
    rows, steps = R.simulate(model, [prompt], [first], n, k, 64, predicted=[want], ngram=False)
    assert rows[0].out == want and steps == 1 + -(-(n - 1) // (k + 1))
    assert rows[0].accepted == rows[0].drafted == n - steps


def test_simulator_stops():
    model = _toy_model(2)
    prompt, n, k = [1, 2, 3], 24, 3
    first = model(prompt)
    want = _greedy(model, prompt, first, n)
    stop = want[9]
    at = want.index(stop)
    rows, steps = R.simulate(model, [prompt, prompt], [first, first], n, k, 64, stop_ids=(stop,), max_tokens=[100, 4],
                             predicted=[want, want])
    assert rows[0].out == want[:at + 1] and (rows[0].length, rows[0].reason) == (at + 1, 1)
    want1 = want[:min(at + 1, 4)]
    assert rows[1].out == want1 and rows[1].reason == (1 if at + 1 <= 4 else 3)
    assert steps < n
    # a row whose prefill token is a stop id starts finished
    rows, steps = R.simulate(model, [prompt], [first], n, k, 64, stop_ids=(first,))
    assert (rows[0].out, rows[0].finished, rows[0].reason, steps) == ([], True, 1, 0)


def test_speculation_validation():
    Speculation(num_draft_tokens=1)
    Speculation(num_draft_tokens=MAX_DRAFT_TOKENS, max_ngram=MAX_NGRAM, ngram=False)
    for bad in (dict(num_draft_tokens=0), dict(num_draft_tokens=MAX_DRAFT_TOKENS + 1),
                dict(num_draft_tokens=2, min_ngram=0), dict(num_draft_tokens=2, min_ngram=3, max_ngram=2),
                dict(num_draft_tokens=2, max_ngram=MAX_NGRAM + 1), dict(num_draft_tokens=2, check_every=-1),
                dict(num_draft_tokens=2, predicted_ids=torch.zeros(2, 3)),
                dict(num_draft_tokens=2, predicted_ids=torch.zeros(3, dtype=torch.long)),
                dict(num_draft_tokens=2, predicted_lens=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            Speculation(**bad)
    sp = Speculation(num_draft_tokens=2, predicted_ids=torch.tensor([[1, 2, 3], [4, 5, 6]]),
                     predicted_lens=torch.tensor([3, 1]))
    sp.validate(vocab_size=7, batch=2)
    with pytest.raises(ValueError):
        sp.validate(vocab_size=6, batch=2)
    with pytest.raises(ValueError):
        sp.validate(vocab_size=7, batch=3)
    with pytest.raises(ValueError):
        Speculation(num_draft_tokens=2, predicted_ids=torch.tensor([[1, 2, 3]]),
                    predicted_lens=torch.tensor([4])).validate(vocab_size=7, batch=1)
