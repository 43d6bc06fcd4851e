"""Greedy speculative decoding over the paged KV pool (extension; the reference's loop emits one token per row per forward,
engine/llm_engine.py:137-213): what the caller asks for (:class:`Speculation`), the device state one such decode keeps
(:class:`SpecState`) and the thin wrappers of the two launches of csrc/speculative.hip.

Semantics (tests/_spec_ref.py is their plain-Python statement).  A row's *history* is its prompt, then the token prefill
returned, then the tokens it emitted: ``hist_len`` tokens, of which ``ctx = hist_len - 1`` are cached when a step starts.
Every step is ONE forward over a ``[B, k + 1]`` grid: column 0 is the row's last token, columns ``1 .. d`` a draft, the rest
token 0 (never stored to cells the row reads).  The draft comes from the row's last ``n`` tokens, ``n = min(max_ngram,
hist_len)`` down to ``min_ngram``: (a) looked up in the caller's prediction of the returned tokens -- the match whose end is
nearest to the number of tokens emitted so far (the aligned position) wins, ties go to the later one -- then (b) in the
history itself, where the latest match wins; the first ``n`` with a match decides, no match spans the two texts, and the
draft is what follows the match, at most ``min(k, remaining - 1, max_seq_len - hist_len - 1)`` tokens: a step can neither
emit past the output row nor outgrow the row's table row.  The step ends with greedy acceptance: with ``a`` the number of
leading drafts equal to the argmax one column earlier, the row emits those ``a`` tokens plus the argmax at column ``a`` --
what one-token greedy decoding over the same logits emits, never fewer than one token.  Stopping follows
executor/stopping.py for stop ids and ``max_tokens``: the finishing token is kept and counted, what the step emitted after
it is dropped, and the row is frozen (``q_len = 0``: it pops no block, its cells go to the junk block)."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _lib as L
from .stopping import StopCriteria

# the limits of csrc/speculative.hip (LL_SPEC_* of include/lite_llama_amd.h)
MAX_DRAFT_TOKENS = 15
MAX_NGRAM = 16
LDS_HISTORY_TOKENS = 4096    # histories up to this length are staged in LDS, longer ones are searched in global memory


@dataclass
class Speculation:
    """``num_draft_tokens`` = ``k`` (1 .. ``MAX_DRAFT_TOKENS``): every step verifies up to ``k`` drafted tokens per row.
    ``ngram``: look the row's last ``max_ngram`` .. ``min_ngram`` tokens up in its own history.  ``predicted_ids`` (int
    ``[B, P]``, ``predicted_lens`` default ``P``): the caller's guess of the returned tokens, looked up first.  Neither:
    every draft is empty -- legal, one token per step.  ``check_every``: as in :class:`StopCriteria`, how often the host
    looks at the number of running rows to leave the loop early (0: never); the results do not depend on it."""

    num_draft_tokens: int
    max_ngram: int = 3
    min_ngram: int = 1
    ngram: bool = True
    predicted_ids: torch.Tensor | None = None
    predicted_lens: torch.Tensor | None = None
    check_every: int = 4

    def __post_init__(self):
        self.num_draft_tokens = int(self.num_draft_tokens)
        self.max_ngram, self.min_ngram = int(self.max_ngram), int(self.min_ngram)
        self.ngram = bool(self.ngram)
        self.check_every = int(self.check_every)
        if not 1 <= self.num_draft_tokens <= MAX_DRAFT_TOKENS:
            raise ValueError(f"num_draft_tokens must be 1 .. {MAX_DRAFT_TOKENS}, got {self.num_draft_tokens}")
        if not 1 <= self.min_ngram <= self.max_ngram <= MAX_NGRAM:
            raise ValueError(f"need 1 <= min_ngram <= max_ngram <= {MAX_NGRAM}, got {self.min_ngram} and {self.max_ngram}")
        if self.check_every < 0:
            raise ValueError("check_every must be >= 0 (0: never look)")
        if self.predicted_ids is not None:
            p = self.predicted_ids
            if not isinstance(p, torch.Tensor) or p.dim() != 2 or p.is_floating_point() or p.dtype == torch.bool:
                raise ValueError("predicted_ids must be an integer tensor [batch, P]")
        elif self.predicted_lens is not None:
            raise ValueError("predicted_lens without predicted_ids")

    def validate(self, vocab_size: int, batch: int) -> None:
        """What only the decode call can check: one prediction row per batch row, ids inside the vocabulary, lengths inside
        the rows."""
        p = self.predicted_ids
        if p is None:
            return
        if p.shape[0] != batch:
            raise ValueError(f"predicted_ids holds {p.shape[0]} rows for a batch of {batch}")
        if p.numel() and (int(p.min()) < 0 or int(p.max()) >= vocab_size):
            raise ValueError(f"predicted_ids holds a token id outside the vocabulary [0, {vocab_size})")
        if self.predicted_lens is not None:
            n = self.predicted_lens
            if n.numel() != batch or (batch and (int(n.min()) < 0 or int(n.max()) > p.shape[1])):
                raise ValueError(f"predicted_lens needs one length in [0, {p.shape[1]}] per row")


@dataclass
class SpeculationStats:
    """What ``DecodeEngine.last_speculation`` holds after a speculative decode (int32 device tensors): per row the verify
    steps it took part in, the tokens drafted for it and the drafts accepted (tokens kept beyond the first of a step);
    ``accepted_per_step [B, steps_run]`` with -1 where the row was not running; ``steps_run``: the steps issued."""

    verify_steps: torch.Tensor
    drafted: torch.Tensor
    accepted: torch.Tensor
    accepted_per_step: torch.Tensor
    steps_run: int


class SpecState:
    """Device state of one speculative decode (all int32 unless said): ``history [B, max_seq_len]`` / ``hist_len`` /
    ``emitted`` / ``finished`` / ``lengths`` / ``reasons`` per row, ``running [1]``, the step's grid ``ids`` / ``positions``
    (int64 ``[B, k + 1]``), ``q_len`` / ``ctx_len``, the statistics ``verify_steps`` / ``drafted`` / ``accepted`` /
    ``accepted_per_step [B, max_new_tokens]`` (-1: the row was not running) and ``step [1]``, the column the next step
    writes -- a device word, so that a captured step replays.  ``out`` int64 ``[B, max_new_tokens + 1]``: column 0 the
    token prefill returned, then the returned tokens, the pad where none was written."""

    def __init__(self, spec: Speculation, stop: StopCriteria | None, prompt_ids: torch.Tensor, prompt_lens: torch.Tensor,
                 first_tokens: torch.Tensor, max_new_tokens: int, max_seq_len: int, device):
        b = first_tokens.numel()
        k = spec.num_draft_tokens
        i32 = dict(dtype=torch.int32, device=device)
        self.criteria = spec                                    # what RunningWatch reads: check_every
        self.k, self.max_new_tokens, self.max_seq_len, self.batch = k, int(max_new_tokens), int(max_seq_len), b
        self.pad = 0 if stop is None else stop.pad_token_id
        ids = [] if stop is None else stop.stop_token_ids
        self.n_ids = len(ids)
        self.stop_ids = torch.tensor(ids or [0], dtype=torch.int64, device=device)
        self.max_tokens = (None if stop is None or stop.max_tokens is None
                           else torch.tensor(stop.max_tokens, **i32))
        lens = prompt_lens.to(device=device, dtype=torch.int64).view(b)
        first = first_tokens.reshape(b).to(device=device, dtype=torch.int64)
        self.history = torch.zeros(b, max_seq_len, **i32)
        lp = min(prompt_ids.shape[1], max_seq_len)
        self.history[:, :lp] = prompt_ids[:, :lp].to(device=device, dtype=torch.int32)
        at = lens.clamp(max=max_seq_len - 1).view(b, 1)
        self.history.scatter_(1, at, first.to(torch.int32).view(b, 1))   # the prefill's token follows the prompt
        self.hist_len = (lens + 1).to(torch.int32)
        self.emitted = torch.zeros(b, **i32)
        hit = torch.isin(first, self.stop_ids[:self.n_ids]) if self.n_ids else torch.zeros(b, dtype=torch.bool, device=device)
        self.finished = hit.to(torch.int32)                      # a row whose prefill token is a stop id starts finished
        self.reasons = self.finished.clone()
        self.lengths = torch.zeros(b, **i32)
        self.running = (b - self.finished.sum()).to(torch.int32).view(1)
        self.ids = torch.zeros(b, k + 1, dtype=torch.int64, device=device)
        self.positions = torch.zeros(b, k + 1, dtype=torch.int64, device=device)
        self.q_len = torch.zeros(b, **i32)
        self.ctx_len = torch.zeros(b, **i32)
        self.b_start_loc = torch.arange(b, **i32) * (k + 1)
        self.cur_select_index = torch.zeros(b * (k + 1), **i32)
        self.verify_steps = torch.zeros(b, **i32)
        self.drafted = torch.zeros(b, **i32)
        self.accepted = torch.zeros(b, **i32)
        self.accepted_per_step = torch.full((b, self.max_new_tokens), -1, **i32)
        self.step = torch.zeros(1, **i32)
        self.out = torch.full((b, self.max_new_tokens + 1), self.pad, dtype=torch.int64, device=device)
        self.out[:, 0] = first
        p = spec.predicted_ids
        self.predicted = None if p is None else p.to(device=device, dtype=torch.int32).contiguous()
        n = spec.predicted_lens
        self.predicted_lens = None if n is None else n.to(device=device, dtype=torch.int32).contiguous().view(b)

    def tensors(self):
        """What a snapshot of the decode state must cover: everything a step writes."""
        return (self.history, self.hist_len, self.emitted, self.finished, self.lengths, self.reasons, self.running,
                self.ids, self.positions, self.q_len, self.ctx_len, self.cur_select_index, self.verify_steps, self.drafted,
                self.accepted, self.accepted_per_step, self.step, self.out)


def spec_draft(state: SpecState) -> None:
    """One launch: the step's grid -- ``ids``, ``positions``, ``q_len``, ``ctx_len`` -- from the rows' histories."""
    s, sp = state, state.criteria
    L.require_cuda(s.history, s.ids)
    p = s.predicted
    L.check(L.lib().ll_spec_draft(
        s.history.data_ptr(), s.history.stride(0), s.hist_len.data_ptr(), s.emitted.data_ptr(), s.finished.data_ptr(),
        L.ptr(s.max_tokens), s.max_new_tokens, s.max_seq_len, s.k, sp.max_ngram, sp.min_ngram, int(sp.ngram), L.ptr(p),
        0 if p is None else p.stride(0), 0 if p is None else p.shape[1], L.ptr(s.predicted_lens), s.ids.data_ptr(),
        s.positions.data_ptr(), s.q_len.data_ptr(), s.ctx_len.data_ptr(), s.batch, L.stream_ptr()), "spec_draft")


def spec_accept(state: SpecState, argmax: torch.Tensor) -> None:
    """One launch: greedy acceptance of the step's drafts against ``argmax`` (int64, one per grid cell), the kept tokens
    appended to ``out`` and the histories, the stop decision, the statistics, ``running``."""
    s = state
    L.require_cuda(argmax, s.out)
    if argmax.dtype != torch.int64 or not argmax.is_contiguous() or argmax.numel() != s.batch * (s.k + 1):
        raise ValueError("spec_accept: argmax must be a contiguous int64 tensor with one entry per grid cell")
    L.check(L.lib().ll_spec_accept(
        argmax.data_ptr(), s.ids.data_ptr(), s.q_len.data_ptr(), s.out.data_ptr(), s.out.stride(0), s.out.shape[1],
        s.history.data_ptr(), s.history.stride(0), s.history.shape[1], s.hist_len.data_ptr(), s.emitted.data_ptr(),
        s.finished.data_ptr(), s.lengths.data_ptr(), s.reasons.data_ptr(), L.ptr(s.max_tokens), s.max_new_tokens,
        s.stop_ids.data_ptr(), s.n_ids, s.verify_steps.data_ptr(), s.drafted.data_ptr(), s.accepted.data_ptr(),
        s.accepted_per_step.data_ptr(), s.accepted_per_step.stride(0), s.accepted_per_step.shape[1], s.step.data_ptr(),
        s.running.data_ptr(), s.batch, s.k, L.stream_ptr()), "spec_accept")
