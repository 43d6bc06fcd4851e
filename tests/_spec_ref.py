"""Plain-Python statement of greedy speculative decoding (executor/speculative.py, csrc/speculative.hip): the draft rule,
the accept rule and a whole-loop simulator over a next-token function.  No torch, no device: lists of ints.

A row's ``history`` is its prompt, then the token prefill returned, then the tokens it emitted; ``emitted`` counts the
emitted ones (the returned tokens).  ``ctx = hist_len - 1`` positions are cached when a step starts: the step feeds
``history[-1]`` and the draft, ``1 + d`` tokens at positions ``ctx .. ctx + d``."""

from __future__ import annotations

from dataclasses import dataclass, field


def draft_limit(k: int, remaining: int, max_seq_len: int, hist_len: int) -> int:
    """The most draft tokens a running row may feed: never past the output row, never past the table row."""
    return max(0, min(k, remaining - 1, max_seq_len - hist_len - 1))


def _find(source, lo_len, n, suffix):
    """Ends ``e`` with ``n <= e < lo_len`` and ``source[e - n : e] == suffix``."""
    return [e for e in range(n, lo_len) if list(source[e - n:e]) == suffix]


def propose(history, emitted: int, lim: int, max_ngram: int = 3, min_ngram: int = 1, ngram: bool = True,
            predicted=None, pred_len: int | None = None):
    """The draft of one running row: the tokens (at most ``lim``).  For ``n = min(max_ngram, hist_len)`` down to
    ``min_ngram`` the last ``n`` tokens are looked up (a) in the prediction -- the end nearest to ``emitted`` wins, ties go
    to the larger end -- then (b) in the history itself -- the latest end wins; the first ``n`` with a candidate decides.
    The draft is what follows the end in that text, as far as the text and ``lim`` go."""
    hist_len = len(history)
    if predicted is not None and pred_len is None:
        pred_len = len(predicted)
    for n in range(min(max_ngram, hist_len), min_ngram - 1, -1):
        if n < 1:
            break
        suffix = list(history[hist_len - n:])
        if predicted is not None:
            ends = _find(predicted, pred_len, n, suffix)
            if ends:
                e = max(ends, key=lambda x: (-abs(x - emitted), x))
                return list(predicted[e:min(pred_len, e + lim)])
        if ngram:
            ends = _find(history, hist_len, n, suffix)
            if ends:
                e = max(ends)
                return list(history[e:min(hist_len, e + lim)])
    return []


def draft_step(history, emitted: int, finished: bool, k: int, max_new_tokens: int, max_tokens: int | None,
               max_seq_len: int, **rule):
    """What ``ll_spec_draft`` writes for one row: ``(ids [k + 1], positions [k + 1], q_len, ctx_len)``."""
    hist_len = len(history)
    ctx = min(hist_len - 1, max_seq_len - 1)
    if finished:
        return [0] * (k + 1), [ctx] * (k + 1), 0, ctx
    cap = max_new_tokens if max_tokens is None else min(max_new_tokens, max_tokens)
    lim = draft_limit(k, cap - emitted, max_seq_len, hist_len)
    draft = propose(history, emitted, lim, **rule) if lim > 0 else []
    d = len(draft)
    ids = [history[-1]] + draft + [0] * (k - d)
    positions = [ctx + min(j, d) for j in range(k + 1)]
    return ids, positions, 1 + d, ctx


@dataclass
class Row:
    """The state ``ll_spec_accept`` moves for one row."""

    history: list
    emitted: int = 0
    finished: bool = False
    length: int = 0
    reason: int = 0
    verify_steps: int = 0
    drafted: int = 0
    accepted: int = 0
    out: list = field(default_factory=list)          # the returned tokens (column 0 of the device's out is not here)
    accepted_per_step: list = field(default_factory=list)


def accept_step(row: Row, ids, q_len: int, argmax, max_new_tokens: int, max_tokens: int | None = None, stop_ids=()):
    """What ``ll_spec_accept`` does to one row; returns whether it is still running.  ``argmax [k + 1]``: the model's token
    after every grid column.  A finished row is left exactly as it is (``accepted_per_step`` gets -1)."""
    if row.finished:
        row.accepted_per_step.append(-1)
        return False
    d = q_len - 1
    a = 0
    while a < d and ids[a + 1] == argmax[a]:
        a += 1
    kept = 0
    for tok in argmax[:a + 1]:
        row.out.append(tok)
        row.history.append(tok)
        row.emitted += 1
        kept += 1
        if tok in stop_ids:
            row.finished, row.reason = True, 1
        elif max_tokens is not None and row.emitted >= max_tokens:
            row.finished, row.reason = True, 3
        elif row.emitted >= max_new_tokens:
            row.finished, row.reason = True, 0
        if row.finished:
            break
    row.length = row.emitted
    row.verify_steps += 1
    row.drafted += d
    row.accepted += kept - 1
    row.accepted_per_step.append(kept - 1)
    return not row.finished


def simulate(next_token, prompts, first_tokens, max_new_tokens: int, k: int, max_seq_len: int, max_tokens=None,
             stop_ids=(), predicted=None, pred_lens=None, drafts=None, **rule):
    """The whole loop.  ``next_token(tokens) -> int`` is the model: the greedy token after a token list.  ``drafts``
    (optional): ``drafts(row_index, step, history, lim) -> list`` replaces the draft rule (any tokens, cut to ``lim``) --
    whatever is drafted, the rows come out as plain greedy decoding gives them.  Returns ``(rows, steps)``: steps = the
    number of verify steps until no row was running."""
    rows = [Row(history=list(p) + [int(f)], finished=int(f) in stop_ids, reason=1 if int(f) in stop_ids else 0)
            for p, f in zip(prompts, first_tokens)]
    steps = 0
    while steps < max_new_tokens and any(not r.finished for r in rows):
        for i, r in enumerate(rows):
            mt = None if max_tokens is None else max_tokens[i]
            if drafts is not None and not r.finished:
                cap = max_new_tokens if mt is None else min(max_new_tokens, mt)
                lim = draft_limit(k, cap - r.emitted, max_seq_len, len(r.history))
                dr = list(drafts(i, steps, list(r.history), lim))[:lim]
                ids, q_len = [r.history[-1]] + dr + [0] * (k - len(dr)), 1 + len(dr)
            else:
                pred = None if predicted is None else predicted[i]
                pl = None if predicted is None else (len(pred) if pred_lens is None else pred_lens[i])
                ids, _, q_len, _ = draft_step(r.history, r.emitted, r.finished, k, max_new_tokens, mt, max_seq_len,
                                              predicted=pred, pred_len=pl, **rule)
            if r.finished:
                accept_step(r, ids, q_len, [0] * (k + 1), max_new_tokens, mt, stop_ids)
                continue
            ctx = len(r.history) - 1
            am = [next_token(r.history[:ctx] + ids[:j + 1]) for j in range(q_len)] + [0] * (k + 1 - q_len)
            accept_step(r, ids, q_len, am, max_new_tokens, mt, stop_ids)
        steps += 1
    return rows, steps


def replay(tokens, first_tokens, prompts, max_new_tokens: int, k: int, max_seq_len: int, **kw):
    """The simulator over a recorded run: ``tokens[i]`` are the tokens row ``i`` returned, which stand in for the model --
    the token after a history whose emitted part is a prefix of the record is the record's next one, anything else (a
    rejected draft's continuation) is -1, which no draft equals.  Returns what :func:`simulate` returns."""
    bases = [len(p) + 1 for p in prompts]
    index = {}

    def next_token(seq):
        i = index["row"]
        done = len(seq) - bases[i]
        rec = tokens[i]
        if done < 0 or done >= len(rec) or list(seq[bases[i]:]) != list(rec[:done]):
            return -1
        return int(rec[done])

    rows = []
    steps = 0
    for i in range(len(prompts)):
        index["row"] = i
        mt = None if kw.get("max_tokens") is None else [kw["max_tokens"][i]]
        pred = None if kw.get("predicted") is None else [kw["predicted"][i]]
        pl = None if kw.get("pred_lens") is None else [kw["pred_lens"][i]]
        rest = {key: v for key, v in kw.items() if key not in ("max_tokens", "predicted", "pred_lens")}
        r, s = simulate(next_token, [prompts[i]], [first_tokens[i]], max_new_tokens, k, max_seq_len, max_tokens=mt,
                        predicted=pred, pred_lens=pl, **rest)
        rows.append(r[0])
        steps = max(steps, s)
    for r in rows:                                   # rows that finished early sat out the later steps
        r.accepted_per_step += [-1] * (steps - len(r.accepted_per_step))
    return rows, steps
