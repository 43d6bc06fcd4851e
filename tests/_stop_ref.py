"""Plain-Python statement of the stopping semantics of lite_llama_amd/executor/stopping.py (lists, no torch): what the
kernel of csrc/decode_stop.hip and DecodeEngine.decode(stop=...) are compared against.

Column 0 of a row's history is the token prefill returned; returned column ``t`` is history column ``t + 1``.  A row
finishes at the step whose sampled token (1) is a stop id, (2) completes a stop sequence as the tail of the history (column
0 may take part, nothing left of it does), (3) brings the count of returned tokens to ``max_tokens[i]``; the lowest number
wins.  The finishing token is kept and counted.  A finished row is frozen: it emits and is fed the pad and advances
nothing, the step it finishes at included."""

RUNNING, STOP_TOKEN, STOP_SEQUENCE, MAX_TOKENS = 0, 1, 2, 3


def finish_reason(history, stop_ids, stop_seqs, max_tokens):
    """``history``: columns 0 .. step of one row, the token just sampled last.  0: the row goes on."""
    tok, returned = history[-1], len(history) - 1
    if tok in stop_ids:
        return STOP_TOKEN
    for seq in stop_seqs:
        n = len(seq)
        if n <= len(history) and history[len(history) - n:] == list(seq):
            return STOP_SEQUENCE
    if max_tokens is not None and returned >= max_tokens:
        return MAX_TOKENS
    return RUNNING


class StopRef:
    """All the state the step keeps, advanced one step at a time.  ``cur_select`` / ``req_idx`` / ``table`` (bump form):
    every row's KV row moves on by the batch each step, and a row still running names it in ``table[req][seq_len - 1]``;
    without them (paged form) rows and table are not this step's business."""

    def __init__(self, first_tokens, stop_ids=(), stop_seqs=(), max_tokens=None, pad=0, positions=None, seq_lens=None,
                 cur_select=None, req_idx=None, table=None):
        b = len(first_tokens)
        self.stop_ids = set(int(t) for t in stop_ids)
        self.stop_seqs = [[int(t) for t in s] for s in stop_seqs]
        self.max_tokens = None if max_tokens is None else [int(v) for v in max_tokens]
        self.pad = int(pad)
        self.history = [[int(t)] for t in first_tokens]
        self.fed = [int(t) for t in first_tokens]
        self.positions = [0] * b if positions is None else [int(v) for v in positions]
        self.seq_lens = [1] * b if seq_lens is None else [int(v) for v in seq_lens]
        self.cur_select = None if cur_select is None else [int(v) for v in cur_select]
        self.req_idx = None if req_idx is None else [int(v) for v in req_idx]
        self.table = None if table is None else [[int(v) for v in row] for row in table]
        # a prefill token that is a stop id: finished before the first step, nothing returned
        self.finished = [1 if t in self.stop_ids else 0 for t in self.fed]
        self.reasons = [STOP_TOKEN if f else RUNNING for f in self.finished]
        self.lengths = [0] * b
        self.running = b - sum(self.finished)
        self.step = 1                      # the history column the next step writes

    def advance(self, next_tokens):
        b = len(self.history)
        for i in range(b):
            tok = self.pad if self.finished[i] else int(next_tokens[i])
            self.history[i].append(tok)
            self.fed[i] = tok
            if not self.finished[i]:
                self.lengths[i] = self.step
                why = finish_reason(self.history[i], self.stop_ids, self.stop_seqs,
                                    None if self.max_tokens is None else self.max_tokens[i])
                if why:
                    self.finished[i], self.reasons[i] = 1, why
            if self.cur_select is not None:
                self.cur_select[i] += b
            if not self.finished[i]:
                self.positions[i] += 1
                self.seq_lens[i] += 1
                if self.cur_select is not None:
                    self.table[self.req_idx[i]][self.seq_lens[i] - 1] = self.cur_select[i]
        self.running = b - sum(self.finished)
        self.step += 1


def apply(first_tokens, tokens, stop_ids=(), stop_seqs=(), max_tokens=None, pad=0):
    """``tokens [B][T]``: what a run without stopping returned.  -> ``(tokens with stopping [B][T], lengths, reasons)``;
    a row still running after ``T`` steps has length ``T`` and reason 0."""
    ref = StopRef(first_tokens, stop_ids, stop_seqs, max_tokens, pad)
    steps = len(tokens[0]) if tokens else 0
    for t in range(steps):
        ref.advance([row[t] for row in tokens])
    return [h[1:] for h in ref.history], list(ref.lengths), list(ref.reasons)
