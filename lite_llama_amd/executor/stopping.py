"""Per-row stopping of a lockstep decode (extension; the reference's loop is "greedy, no EOS stop, lockstep batch",
engine/llm_engine.py:137-213): the criteria the caller states (:class:`StopCriteria`), the device state one decode keeps
for them (:class:`StopState`), the host's early exit (:class:`RunningWatch`) and the thin wrappers of the two launches of
csrc/decode_stop.hip.

Semantics (tests/_stop_ref.py is their plain-Python statement).  Column 0 of the engine's token history is the token
prefill returned; returned column ``t`` is history column ``t + 1``.  A row finishes at the step whose sampled token (1) is
a stop id, (2) completes a stop sequence as the tail of the row's history -- column 0 may be part of a match, the prompt
never is -- or (3) brings the row's count of returned tokens to ``max_tokens[i]``; the lowest number is the reason.  The
finishing token is kept and counted: ``length`` is the number of valid returned tokens.  Reason 0: still running when the
call's ``max_new_tokens`` ran out.  A row whose prefill token is a stop id is finished before the first step (length 0,
reason 1).  From the step after it finishes a row is frozen: it emits and is fed ``pad_token_id``, does not advance
``positions`` / ``b_seq_len``, pops no KV block and cannot finish again; the K/V of its real tokens stays intact (its later
writes go to rows nobody reads)."""

from __future__ import annotations

from dataclasses import dataclass, field

import torch

from .. import _lib as L

# the limits of csrc/decode_stop.hip (LL_STOP_MAX_* of include/lite_llama_amd.h): ids and sequences sit in LDS
MAX_STOP_TOKEN_IDS = 32
MAX_STOP_SEQUENCES = 16
MAX_STOP_SEQUENCE_LEN = 8

REASON_RUNNING, REASON_STOP_TOKEN, REASON_STOP_SEQUENCE, REASON_MAX_TOKENS = 0, 1, 2, 3


@dataclass
class StopCriteria:
    """When the rows of a decode end.  ``stop_token_ids`` (at most ``MAX_STOP_TOKEN_IDS``) and ``stop_sequences`` (at most
    ``MAX_STOP_SEQUENCES`` sequences of 1 .. ``MAX_STOP_SEQUENCE_LEN`` token ids) are shared by the batch; ``max_tokens`` is
    ``None`` or one integer >= 1 per row.  Finished rows emit ``pad_token_id``.  ``check_every``: the host looks at the
    number of running rows every that many steps to leave the loop early (0: never, all ``max_new_tokens`` steps run); the
    results do not depend on it."""

    stop_token_ids: list = field(default_factory=list)
    stop_sequences: list = field(default_factory=list)
    max_tokens: list | None = None
    pad_token_id: int = 0
    check_every: int = 8

    def __post_init__(self):
        self.stop_token_ids = [int(t) for t in self.stop_token_ids]
        self.stop_sequences = [[int(t) for t in s] for s in self.stop_sequences]
        if self.max_tokens is not None:
            self.max_tokens = [int(v) for v in (self.max_tokens.tolist() if isinstance(self.max_tokens, torch.Tensor)
                                                else self.max_tokens)]
        self.pad_token_id = int(self.pad_token_id)
        self.check_every = int(self.check_every)
        if not self.stop_token_ids and not self.stop_sequences and self.max_tokens is None:
            raise ValueError("StopCriteria needs a criterion: stop_token_ids, stop_sequences or max_tokens")
        if len(self.stop_token_ids) > MAX_STOP_TOKEN_IDS:
            raise ValueError(f"at most {MAX_STOP_TOKEN_IDS} stop_token_ids, got {len(self.stop_token_ids)}")
        if len(self.stop_sequences) > MAX_STOP_SEQUENCES:
            raise ValueError(f"at most {MAX_STOP_SEQUENCES} stop_sequences, got {len(self.stop_sequences)}")
        for s in self.stop_sequences:
            if not s:
                raise ValueError("a stop sequence is empty")
            if len(s) > MAX_STOP_SEQUENCE_LEN:
                raise ValueError(f"a stop sequence holds at most {MAX_STOP_SEQUENCE_LEN} ids, got {len(s)}")
        if self.max_tokens is not None and any(v < 1 for v in self.max_tokens):
            raise ValueError("every max_tokens value must be >= 1")
        if self.check_every < 0:
            raise ValueError("check_every must be >= 0 (0: never look)")

    def validate(self, vocab_size: int, batch: int) -> None:
        """What only the decode call can check: ids inside ``[0, vocab_size)``, one ``max_tokens`` per row."""
        ids = self.stop_token_ids + [t for s in self.stop_sequences for t in s] + [self.pad_token_id]
        for t in ids:
            if not 0 <= t < vocab_size:
                raise ValueError(f"token id {t} is outside the vocabulary [0, {vocab_size})")
        if self.max_tokens is not None and len(self.max_tokens) != batch:
            raise ValueError(f"max_tokens holds {len(self.max_tokens)} values for a batch of {batch}")


class StopState:
    """Device state of one decode with stopping: the criteria as the kernel reads them, and per row ``finished`` /
    ``lengths`` / ``reasons`` (int32), plus ``running`` (int32 ``[1]``: rows still running after the last step).
    ``first_tokens``: the tokens prefill returned -- a row whose token is a stop id starts finished."""

    def __init__(self, criteria: StopCriteria, first_tokens: torch.Tensor, device):
        b = first_tokens.numel()
        c = criteria
        self.criteria = c
        self.pad = c.pad_token_id
        self.n_ids, self.n_seqs = len(c.stop_token_ids), len(c.stop_sequences)
        self.stop_ids = torch.tensor(c.stop_token_ids or [0], dtype=torch.int64, device=device)
        grid = [s + [0] * (MAX_STOP_SEQUENCE_LEN - len(s)) for s in c.stop_sequences] or [[0] * MAX_STOP_SEQUENCE_LEN]
        self.stop_seqs = torch.tensor(grid, dtype=torch.int64, device=device)
        self.seq_lens = torch.tensor([len(s) for s in c.stop_sequences] or [0], dtype=torch.int32, device=device)
        self.max_tokens = None if c.max_tokens is None else torch.tensor(c.max_tokens, dtype=torch.int32, device=device)
        first = first_tokens.reshape(b).to(device)
        hit = torch.isin(first, self.stop_ids[:self.n_ids]) if self.n_ids else torch.zeros(b, dtype=torch.bool, device=device)
        self.finished = hit.to(torch.int32)
        self.reasons = self.finished.clone()                     # REASON_STOP_TOKEN where finished
        self.lengths = torch.zeros(b, dtype=torch.int32, device=device)
        self.running = (b - self.finished.sum()).to(torch.int32).view(1)

    def tensors(self):
        """What a snapshot of the decode state must cover."""
        return (self.finished, self.lengths, self.reasons, self.running)


class RunningWatch:
    """The early exit of a decode with ``stop``, without a synchronisation per step: every ``check_every`` steps a copy of
    the device's running-row count to pinned memory is enqueued, and the host waits only for the copy enqueued one
    interval earlier -- by then long done.  Finished rows are frozen, so the steps issued meanwhile change nothing."""

    def __init__(self, state: StopState):
        self._state = state
        self._every = state.criteria.check_every
        self._host = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._events = [torch.cuda.Event() for _ in range(2)]
        self._pending = None        # slot of the copy enqueued at the previous interval
        self._next_at = self._every

    def all_finished(self, steps_done: int) -> bool:
        """Call between steps (replays) with the number of steps issued so far."""
        if steps_done < self._next_at:
            return False
        self._next_at = (steps_done // self._every + 1) * self._every
        done = False
        slot = 0
        if self._pending is not None:
            self._events[self._pending].synchronize()
            done = int(self._host[self._pending][0]) == 0
            slot = 1 - self._pending
        if not done:
            self._host[slot].copy_(self._state.running, non_blocking=True)
            self._events[slot].record()
            self._pending = slot
        return done


def stop_advance(out: torch.Tensor, step: torch.Tensor, next_tokens: torch.Tensor, input_ids: torch.Tensor,
                 positions: torch.Tensor, cur_select_index: torch.Tensor | None, b_seq_len: torch.Tensor,
                 b_req_idx: torch.Tensor | None, table: torch.Tensor | None, state: StopState) -> None:
    """One launch: record ``next_tokens`` (or the pad) in column ``step`` of ``out``, feed it back, take the stop
    decision, advance the rows still running, count them into ``state.running``, ``step += 1``.  With
    ``cur_select_index`` (the bump pool) every row's KV row moves on by the batch and the running rows' table entries are
    written; ``None`` (the paged pool) leaves rows and table to ``PagedKVPool.append`` + :func:`redirect_finished`."""
    b = next_tokens.numel()
    L.require_cuda(out, step, next_tokens, input_ids, positions, b_seq_len, state.finished)
    for t in (out, step, next_tokens, input_ids, positions):
        if t.dtype != torch.int64:
            raise ValueError("stop_advance: out, step, next_tokens, input_ids and positions must be int64")
    ints = [b_seq_len] + ([cur_select_index, b_req_idx, table] if cur_select_index is not None else [])
    for t in ints:
        if t is None or t.dtype != torch.int32:
            raise ValueError("stop_advance: b_seq_len, cur_select_index, b_req_idx and the token table must be int32")
    for t in (next_tokens, input_ids, positions, b_seq_len, cur_select_index, b_req_idx):
        if t is not None and (not t.is_contiguous() or t.numel() != b):
            raise ValueError("stop_advance: per-row tensors must be contiguous with one entry per row")
    if out.dim() != 2 or out.shape[0] != b or out.stride(1) != 1 or state.finished.numel() != b:
        raise ValueError("stop_advance: out must be [batch, columns] with unit column stride, the state one entry per row")
    bump = cur_select_index is not None
    L.check(L.lib().ll_decode_stop_advance(
        out.data_ptr(), out.stride(0), out.shape[1], step.data_ptr(), next_tokens.data_ptr(), input_ids.data_ptr(),
        positions.data_ptr(), L.ptr(cur_select_index), b_seq_len.data_ptr(), L.ptr(b_req_idx) if bump else 0,
        L.ptr(table) if bump else 0, table.stride(0) if bump else 0, table.stride(1) if bump else 0,
        table.shape[1] if bump else 0, state.stop_ids.data_ptr(), state.n_ids, state.stop_seqs.data_ptr(),
        state.seq_lens.data_ptr(), state.n_seqs, L.ptr(state.max_tokens), state.pad, state.finished.data_ptr(),
        state.lengths.data_ptr(), state.reasons.data_ptr(), state.running.data_ptr(), b, L.stream_ptr()),
        "decode_stop_advance")


def redirect_finished(cur_select_index: torch.Tensor, state: StopState, junk_row: int, block_size: int) -> None:
    """Paged pool, after the step's append: the KV row of every finished row becomes a row of the junk block (whose first
    row is ``junk_row``) -- the append named the row of its last real position again, which must stay intact."""
    L.require_cuda(cur_select_index)
    if cur_select_index.dtype != torch.int32 or not cur_select_index.is_contiguous():
        raise ValueError("redirect_finished: cur_select_index must be a contiguous int32 tensor")
    L.check(L.lib().ll_decode_stop_redirect(cur_select_index.data_ptr(), state.finished.data_ptr(), junk_row, block_size,
                                            cur_select_index.numel(), L.stream_ptr()), "decode_stop_redirect")
