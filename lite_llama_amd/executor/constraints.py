"""Constrained decoding over a token automaton (extension; the reference's sampler restricts nothing): the automaton the
caller states (:class:`TokenAutomaton` and its builders), the device state one generation keeps for it
(:class:`ConstrainedRows`) and the thin wrappers of the three launches of csrc/constrained.hip.

Semantics (tests/_constraint_ref.py is their plain-Python statement).  The automaton has ``S`` states and ``E`` edges in CSR
form: ``offsets [S + 1]``, ``tokens [E]`` strictly ascending inside a state, ``next_states [E]``, ``accepting [S]``.  Every
state has at least one edge, so no row can get stuck; there is no special "unconstrained" state -- one that allows
everything lists every token.  A row holds one int32 state.  Greedy selection: a row in state ``s`` looks only at the edges
``offsets[s] .. offsets[s + 1]`` and emits the token of the edge with the largest logit (the stored value compared as
fp32); ties go to the lowest token id, which is the first maximum in edge order; if every candidate is ``-inf`` the first
edge wins; the state becomes that edge's ``next_states`` entry.  Sampling: disallowed logits become ``-inf`` in a copy
(taken after the repetition penalty), the temperature + nucleus sampler draws from the copy, and the state follows the
drawn token.  With ``stop``: a row that was finished when the step began keeps its state; the step at which it finishes
does advance it (the finishing token is kept and counted), so at the end ``states`` describes the valid tokens of every
row.  NaN logits are not specified."""

from __future__ import annotations

import torch

from .. import _lib as L

ERROR_ABSENT_TOKEN, ERROR_BAD_STATE = 1, 2


def _int32(values, what: str) -> torch.Tensor:
    t = values.detach().cpu() if isinstance(values, torch.Tensor) else torch.tensor(list(values), dtype=torch.int64)
    if t.dim() != 1 or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{what} must be a flat sequence of integers")
    t = t.to(torch.int64)
    if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 31)):
        raise ValueError(f"{what} does not fit int32")
    return t.to(torch.int32).contiguous()


class TokenAutomaton:
    """A finite automaton over token ids in CSR form, validated on the host when it is built: every state has at least one
    edge, tokens are non-negative and strictly ascending inside a state, next states lie in ``[0, num_states)``.  That the
    tokens lie inside a model's vocabulary is checked where the model is known (:meth:`validate`, called by the engine).
    ``accepting``: the accepting states (a bool / 0-1 value per state, default none)."""

    def __init__(self, offsets, tokens, next_states, accepting=None):
        off, tok, nxt = _int32(offsets, "offsets"), _int32(tokens, "tokens"), _int32(next_states, "next_states")
        s, e = off.numel() - 1, tok.numel()
        if s < 1:
            raise ValueError("an automaton needs at least one state (offsets holds num_states + 1 entries)")
        if nxt.numel() != e:
            raise ValueError(f"tokens holds {e} edges, next_states {nxt.numel()}")
        if int(off[0]) != 0 or int(off[-1]) != e:
            raise ValueError(f"offsets must run from 0 to the number of edges {e}")
        degree = off[1:].long() - off[:-1].long()
        if int(degree.min()) < 1:
            bad = int((degree < 1).nonzero()[0])
            raise ValueError(f"state {bad} has no edge: a row reaching it would be stuck")
        if int(tok.min()) < 0:
            raise ValueError("token ids must be >= 0")
        if e > 1:
            first = torch.zeros(e, dtype=torch.bool)
            first[off[:-1].long()] = True
            if bool(((tok[1:] <= tok[:-1]) & ~first[1:]).any()):
                raise ValueError("the tokens of a state must be strictly ascending (sorted, no duplicates)")
        if int(nxt.min()) < 0 or int(nxt.max()) >= s:
            raise ValueError(f"next states must lie in [0, {s})")
        if accepting is None:
            acc = torch.zeros(s, dtype=torch.uint8)
        else:
            acc = (accepting.detach().cpu() if isinstance(accepting, torch.Tensor) else torch.tensor(list(accepting)))
            if acc.numel() != s:
                raise ValueError(f"accepting holds {acc.numel()} entries for {s} states")
            acc = (acc.reshape(s) != 0).to(torch.uint8)
        self.offsets, self.tokens, self.next_states, self.accepting = off, tok, nxt, acc
        self.num_states, self.num_edges = s, e
        self.max_degree = int(degree.max())
        self.max_token = int(tok.max())

    def to(self, device) -> "TokenAutomaton":
        """The same automaton with its arrays on ``device`` (not validated again)."""
        other = object.__new__(TokenAutomaton)
        other.__dict__.update(self.__dict__)
        for name in ("offsets", "tokens", "next_states", "accepting"):
            setattr(other, name, getattr(self, name).to(device))
        return other

    @property
    def device(self):
        return self.offsets.device

    def validate(self, vocab_size: int) -> None:
        """What only the engine call can check: token ids inside ``[0, vocab_size)``."""
        if self.max_token >= vocab_size:
            raise ValueError(f"token id {self.max_token} is outside the vocabulary [0, {vocab_size})")


def from_transitions(transitions, accepting=()) -> TokenAutomaton:
    """``{state: {token: next_state}}`` over states ``0 .. S - 1`` (every state named, as a key or as a next state, and
    every state with at least one token) -> :class:`TokenAutomaton`; ``accepting``: the accepting states' numbers.  The
    form an external regex or JSON-schema compiler hands over."""
    keys = [int(s) for s in transitions]
    named = set(keys)
    for edges in transitions.values():
        named.update(int(n) for n in edges.values())
    if not named or min(named) < 0:
        raise ValueError("states are numbered from 0")
    s = max(named) + 1
    by_state = {int(k): v for k, v in transitions.items()}
    offsets, tokens, nxt = [0], [], []
    for state in range(s):
        edges = by_state.get(state) or {}
        if not edges:
            raise ValueError(f"state {state} has no edge: a row reaching it would be stuck")
        for tok in sorted(int(t) for t in edges):
            tokens.append(tok)
        nxt.extend(int(edges[t]) for t in sorted(edges, key=int))
        offsets.append(len(tokens))
    acc = [0] * s
    for a in accepting:
        if not 0 <= int(a) < s:
            raise ValueError(f"accepting state {a} is outside [0, {s})")
        acc[int(a)] = 1
    return TokenAutomaton(offsets, tokens, nxt, acc)


def from_choices(choices, eos_token_id: int) -> TokenAutomaton:
    """"Answer with one of these token sequences": a trie over ``choices`` (non-empty id sequences) with the root as state
    0; a node where a choice ends gets an extra edge ``eos -> END``, and ``END`` (the last state) has the single edge
    ``eos -> END``.  Accepting: the choice-end nodes and ``END``.  With ``stop=StopCriteria(stop_token_ids=[eos])`` a row
    ends one token after its choice is complete."""
    eos = int(eos_token_id)
    choices = [[int(t) for t in c] for c in choices]
    if not choices:
        raise ValueError("from_choices needs at least one choice")
    nodes, ends = [{}], set()
    for c in choices:
        if not c:
            raise ValueError("a choice is empty")
        if eos in c:
            raise ValueError(f"a choice contains eos_token_id {eos}")
        at = 0
        for t in c:
            if t not in nodes[at]:
                nodes.append({})
                nodes[at][t] = len(nodes) - 1
            at = nodes[at][t]
        ends.add(at)
    end = len(nodes)
    for n in ends:
        nodes[n][eos] = end
    nodes.append({eos: end})
    return from_transitions(dict(enumerate(nodes)), accepting=sorted(ends) + [end])


def union(automata) -> tuple:
    """Several automata side by side in one: ``(automaton, start_states)``, ``start_states[i]`` being state 0 of
    ``automata[i]`` -- so the rows of one batch can follow different constraints."""
    automata = list(automata)
    if not automata:
        raise ValueError("union needs at least one automaton")
    offsets, tokens, nxt, acc, starts = [torch.zeros(1, dtype=torch.int32)], [], [], [], []
    s0 = e0 = 0
    for a in automata:
        a = a.to("cpu")
        starts.append(s0)
        offsets.append(a.offsets[1:] + e0)
        tokens.append(a.tokens)
        nxt.append(a.next_states + s0)
        acc.append(a.accepting)
        s0 += a.num_states
        e0 += a.num_edges
    return TokenAutomaton(torch.cat(offsets), torch.cat(tokens), torch.cat(nxt), torch.cat(acc)), starts


class ConstrainedRows:
    """Device state of one constrained generation: ``states`` (int32 ``[batch]``, one per row) and the one-word sticky
    ``error`` the kernels set (bit 1: a token its row's state does not allow was to be followed, bit 2: a state outside the
    automaton).  ``start_states``: one int, or one per row."""

    def __init__(self, automaton: TokenAutomaton, start_states, batch: int, device):
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        starts = [int(start_states)] * batch if isinstance(start_states, int) else [int(v) for v in (
            start_states.tolist() if isinstance(start_states, torch.Tensor) else start_states)]
        if len(starts) != batch:
            raise ValueError(f"start_states holds {len(starts)} values for a batch of {batch}")
        for s in starts:
            if not 0 <= s < automaton.num_states:
                raise ValueError(f"start state {s} is outside [0, {automaton.num_states})")
        self.automaton = automaton if automaton.device == torch.device(device) else automaton.to(device)
        self.batch = batch
        self.start_states = torch.tensor(starts, dtype=torch.int32, device=device)
        self.states = self.start_states.clone()
        self.error = torch.zeros(1, dtype=torch.int32, device=device)

    def reset(self) -> None:
        """Back to the start states (and a clean error word)."""
        self.states.copy_(self.start_states)
        self.error.zero_()

    def accepted(self) -> torch.Tensor:
        """bool ``[batch]``: the row's state is accepting."""
        return self.automaton.accepting[self.states.long()] != 0

    def tensors(self):
        """What a snapshot of the decode state must cover."""
        return (self.states, self.error)

    def validate(self, vocab_size: int, batch: int) -> None:
        """What only the engine call can check."""
        if self.batch != batch:
            raise ValueError(f"the constraint holds {self.batch} rows for a batch of {batch}")
        self.automaton.validate(vocab_size)


def _check_rows(logits: torch.Tensor, rows: ConstrainedRows, what: str) -> torch.Tensor:
    if logits.dim() != 2:
        raise ValueError(f"{what}: logits must be [batch, vocab]")
    if logits.shape[0] != rows.batch:
        raise ValueError(f"{what}: logits hold {logits.shape[0]} rows, the constraint {rows.batch}")
    rows.automaton.validate(logits.shape[1])
    L.require_cuda(logits, rows.states)
    return logits if logits.stride(1) == 1 else logits.contiguous()


def _check_finished(finished, rows: ConstrainedRows, what: str) -> None:
    if finished is not None and (finished.dtype != torch.int32 or finished.numel() != rows.batch
                                 or not finished.is_contiguous()):
        raise ValueError(f"{what}: finished must be a contiguous int32 tensor with one entry per row")


def constrained_argmax(logits: torch.Tensor, rows: ConstrainedRows, finished: torch.Tensor | None = None) -> torch.Tensor:
    """``logits [batch, vocab]`` (fp16 / bf16 / fp32, any row stride) -> int64 ``[batch]``: every row's best allowed token;
    ``rows.states`` moves along the chosen edges.  One launch.  Rows with ``finished[b] != 0`` (int32, optional) keep
    their state; what they emit is unspecified."""
    logits = _check_rows(logits, rows, "constrained_argmax")
    _check_finished(finished, rows, "constrained_argmax")
    a = rows.automaton
    out = torch.empty(rows.batch, dtype=torch.int64, device=logits.device)
    L.check(L.lib().ll_constrained_argmax(out.data_ptr(), rows.states.data_ptr(), logits.data_ptr(), a.offsets.data_ptr(),
                                          a.tokens.data_ptr(), a.next_states.data_ptr(), L.ptr(finished),
                                          rows.error.data_ptr(), rows.batch, logits.shape[1], logits.stride(0),
                                          a.num_states, L.dtype_code(logits.dtype), L.stream_ptr()),
            "constrained_argmax")
    return out


def constraint_mask(logits: torch.Tensor, rows: ConstrainedRows) -> torch.Tensor:
    """A copy of ``logits [batch, vocab]`` with ``-inf`` wherever the row's state does not allow the token; the allowed
    entries are copied bit for bit.  The states are not moved."""
    logits = _check_rows(logits, rows, "constraint_mask")
    a = rows.automaton
    out = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    L.check(L.lib().ll_constraint_mask(out.data_ptr(), logits.data_ptr(), rows.states.data_ptr(), a.offsets.data_ptr(),
                                       a.tokens.data_ptr(), rows.error.data_ptr(), rows.batch, logits.shape[1],
                                       logits.stride(0), out.stride(0), a.num_states, L.dtype_code(logits.dtype),
                                       L.stream_ptr()),
            "constraint_mask")
    return out


def constraint_advance(rows: ConstrainedRows, tokens: torch.Tensor, finished: torch.Tensor | None = None) -> None:
    """``rows.states`` follows ``tokens`` (int64, one per row).  A token the row's state does not allow sets ``rows.error``
    and leaves the state; rows with ``finished[b] != 0`` keep theirs."""
    L.require_cuda(tokens, rows.states)
    if tokens.dtype != torch.int64 or tokens.numel() != rows.batch:
        raise ValueError(f"constraint_advance: tokens must be int64 with one id per row ({rows.batch})")
    _check_finished(finished, rows, "constraint_advance")
    tokens = tokens.reshape(-1).contiguous()
    a = rows.automaton
    L.check(L.lib().ll_constraint_advance(rows.states.data_ptr(), tokens.data_ptr(), a.offsets.data_ptr(),
                                          a.tokens.data_ptr(), a.next_states.data_ptr(), L.ptr(finished),
                                          rows.error.data_ptr(), rows.batch, a.num_states, L.stream_ptr()),
            "constraint_advance")
