"""Plain-Python statement of the constrained-decoding semantics (lite_llama_amd/executor/constraints.py) and the seeded
random cases the kernel tests run; no GPU, no kernels.  An automaton here is the tuple ``(offsets, tokens, next_states)`` of
Python lists; logits are rows of Python floats (the stored values, which convert to fp32 exactly)."""

import functools
import math
import random

NEG_INF = -math.inf


def edges(aut, state):
    offsets, _, _ = aut
    return range(offsets[state], offsets[state + 1])


def select(aut, state, logits_row):
    """Greedy selection: ``(token, next state)`` of the edge with the largest logit; the first maximum in edge order
    (= the lowest token id); the first edge when every candidate is -inf."""
    _, tokens, nxt = aut
    best = None
    for e in edges(aut, state):
        v = logits_row[tokens[e]]
        if best is None or v > best[0]:
            best = (v, e)
    return tokens[best[1]], nxt[best[1]]


def advance(aut, state, token):
    """The state after ``token``, or ``None`` when ``state`` does not allow it."""
    _, tokens, nxt = aut
    for e in edges(aut, state):
        if tokens[e] == token:
            return nxt[e]
    return None


def walk(aut, state, token_seq):
    """The state after the whole sequence; ``None`` as soon as a token is not allowed."""
    for t in token_seq:
        state = advance(aut, state, t)
        if state is None:
            return None
    return state


def allowed(aut, state):
    _, tokens, _ = aut
    return [tokens[e] for e in edges(aut, state)]


def lists(automaton):
    """``(offsets, tokens, next_states)`` of a lite_llama_amd TokenAutomaton as Python lists."""
    return automaton.offsets.tolist(), automaton.tokens.tolist(), automaton.next_states.tolist()


# ------------------------------------------------------------------ the kernel tests' random cases ----- #
VOCAB = 1024
BATCHES = (1, 3, 64, 257)
DTYPES = ("float16", "bfloat16", "float32")
# every degree at which the kernel's walk changes shape: one edge, less than / exactly / more than a wave, a workgroup, and
# several passes of a workgroup; degree 1 twice so that it reaches its share
DEGREES = (1, 1, 2, 63, 64, 65, 255, 256, 257, 1024)
# 8 distinct values, exact in fp16 and bf16: rows are full of ties; -inf among them
VALUES = (NEG_INF, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0)
NUM_STATES = 2 * len(DEGREES)


@functools.lru_cache(maxsize=None)
def random_automaton(seed=0, vocab=VOCAB):
    rng = random.Random(seed)
    offsets, tokens, nxt = [0], [], []
    for s in range(NUM_STATES):
        toks = sorted(rng.sample(range(vocab), DEGREES[s % len(DEGREES)]))
        tokens += toks
        nxt += [rng.randrange(NUM_STATES) for _ in toks]
        offsets.append(len(tokens))
    return offsets, tokens, nxt


@functools.lru_cache(maxsize=None)
def make_case(batch, dtype):
    """One random case: ``(states, logits rows, finished, expected tokens, expected states)``.  Row ``batch - 1`` has every
    candidate at -inf; about a fifth of the rows are finished (they keep their state; their token is not checked)."""
    aut = random_automaton()
    rng = random.Random(f"{batch}-{dtype}")
    states = [rng.randrange(NUM_STATES) for _ in range(batch)]
    logits = [[rng.choice(VALUES) for _ in range(VOCAB)] for _ in range(batch)]
    for t in allowed(aut, states[batch - 1]):
        logits[batch - 1][t] = NEG_INF
    finished = [1 if rng.random() < 0.2 else 0 for _ in range(batch)]
    finished[batch - 1] = 0
    want = [select(aut, s, row) for s, row in zip(states, logits)]
    tokens = [w[0] for w in want]
    new_states = [s if f else w[1] for s, f, w in zip(states, finished, want)]
    return states, logits, finished, tokens, new_states


def coverage():
    """Shares over all rows of the random cases, from the reference alone: ``(tied maximum, degree 1, degree > 256, rows
    whose candidates are all -inf)`` -- the last one a count."""
    aut = random_automaton()
    rows = tied = one = wide = dead = 0
    for batch in BATCHES:
        for dtype in DTYPES:
            states, logits, _, _, _ = make_case(batch, dtype)
            for s, row in zip(states, logits):
                cand = [row[t] for t in allowed(aut, s)]
                rows += 1
                tied += cand.count(max(cand)) > 1
                one += len(cand) == 1
                wide += len(cand) > 256
                dead += max(cand) == NEG_INF
    return tied / rows, one / rows, wide / rows, dead
