"""Constrained decoding (csrc/constrained.hip, DecodeEngine.decode(constraint=...)): what the three launches cost alone
and what a constrained step costs.  One JSON line.

    python benchmarks/constraint.py            # kernels and step
    python benchmarks/constraint.py --no-step  # kernels only

Kernels: batch 64, vocabulary 152 064, fp16 logits; device events around replays of a hipGraph holding 200 launches;
ll_constrained_argmax at degrees 2, 64, 4096 and the whole vocabulary (one state that loops on itself, its tokens spread
over the vocabulary), greedy_argmax on the same logits, ll_constraint_mask and ll_constraint_advance at degree 4096.
Alternated in one process, median of the rounds.
Step: median ms per replay of the captured step, Qwen2.5-7B W4A16, batch 64, context 512, set up as benchmarks/step_times.py
does: no constraint, a from_choices automaton (degree <= 48), a state of degree 64, one of 4096 and the whole vocabulary,
greedy; and the sampling route (temperature 0.8, top_p 0.9) without and with the degree-4096 constraint.  Every variant is
measured twice, alternated -- the difference of the two runs without a constraint is the run-to-run spread."""
import json, os, random, statistics, sys, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_llama_amd.executor import (ConstrainedRows, TokenAutomaton, constrained_argmax, constraint_advance,
                                     constraint_mask, from_choices)
from lite_llama_amd.sampling import greedy_argmax

DEV = "cuda"
ROUNDS = 7
LAUNCHES = 200
VOCAB = 152064


def replay_us(g, calls, replays=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def looping_state(degree, vocab=VOCAB, seed=0):
    """One state allowing ``degree`` tokens spread over the vocabulary, every edge leading back to it."""
    toks = list(range(vocab)) if degree >= vocab else sorted(random.Random(seed).sample(range(vocab), degree))
    return TokenAutomaton([0, len(toks)], toks, [0] * len(toks))


def kernel_numbers(batch=64):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(batch, VOCAB, generator=g) * 2).half().to(DEV)
    fns = {"greedy_argmax": lambda: greedy_argmax(logits)}
    keep = []
    for degree in (2, 64, 4096, VOCAB):
        rows = ConstrainedRows(looping_state(degree), 0, batch, DEV)
        keep.append(rows)
        fns[f"constrained_argmax_degree_{degree}"] = (lambda r: lambda: constrained_argmax(logits, r))(rows)
        if degree == 4096:
            allowed = constrained_argmax(logits, rows)
            fns["constraint_mask_degree_4096"] = (lambda r: lambda: constraint_mask(logits, r))(rows)
            fns["constraint_advance_degree_4096"] = (lambda r, t: lambda: constraint_advance(r, t))(rows, allowed)
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(LAUNCHES):
                fn()
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    assert all(int(r.error) == 0 for r in keep)
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):  # alternated
        for name, gr in graphs.items():
            times[name].append(replay_us(gr, LAUNCHES))
    res = {"batch": batch, "vocab": VOCAB, "dtype": "float16"}
    for name, t in times.items():
        res[name + "_us"] = round(statistics.median(t), 3)
        res[name + "_min_max_us"] = [round(min(t), 3), round(max(t), 3)]
    return res


def engine_numbers(steps=60):
    from lite_llama_amd.executor import DecodeEngine
    from lite_llama_amd.model import GEOMETRY, CausalLM
    from lite_llama_amd.quantization import QuantConfig

    geo = GEOMETRY["qwen2.5-7b"]
    quant = QuantConfig.for_runtime_scheme("int4")
    B = 64
    with torch.device(DEV):
        model = CausalLM(geo, quant)
    model.init_synthetic(seed=0, quant=quant, device=DEV)
    if hasattr(model, "compact_weights"):
        model.compact_weights()
    eng = DecodeEngine(model, max_batch=B, max_seq_len=512 + 256 + 8, device=DEV)
    rng = random.Random(1)
    # 48 choices of 1 - 6 tokens out of 64 distinct ids: the root's degree is at most 48, every other state's smaller
    ids = rng.sample(range(1000, geo.vocab_size), 64)
    choices = from_choices([[rng.choice(ids[:48])] + [rng.choice(ids) for _ in range(rng.randrange(6))] for _ in range(48)],
                           eos_token_id=7)
    # under ``choices`` a row reaches END (degree 1) within 7 steps and stays; ``degree_64`` keeps 64 candidates at every step
    automata = {"choices": choices, "degree_64": looping_state(64, geo.vocab_size),
                "degree_4096": looping_state(4096, geo.vocab_size),
                "full_vocab": looping_state(geo.vocab_size, geo.vocab_size)}
    sp = types.SimpleNamespace(temperature=0.8, top_p=0.9, repetition_penalty=1.0)

    def run(automaton, sampling=None, n=steps):
        first = eng.synthetic_context(B, 512, seed=1)
        rows = None if automaton is None else ConstrainedRows(automaton, 0, B, DEV)
        evs = []

        def on_step(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)

        eng.decode(first, n, use_graph=True, on_step=on_step, sampling=sampling, constraint=rows)
        torch.cuda.synchronize()
        d = [evs[i].elapsed_time(evs[i + 1]) for i in range(10, len(evs) - 1)]  # the first replays of a fresh graph are slow
        return statistics.median(d)

    run(None)  # warms every shape
    r = {"choices_max_degree": choices.max_degree}
    greedy = [("none", None)] + list(automata.items())
    for again in ("", "_again"):
        for name, a in greedy:
            r[name + again + "_ms"] = round(run(a), 4)
    for again in ("", "_again"):
        for name, a in (("sampling_none", None), ("sampling_degree_4096", automata["degree_4096"])):
            r[name + again + "_ms"] = round(run(a, sampling=sp), 4)
    r["none_spread_us"] = round(abs(r["none_again_ms"] - r["none_ms"]) * 1e3, 1)
    for name in automata:
        r[name + "_delta_us"] = round((r[name + "_ms"] + r[name + "_again_ms"] - r["none_ms"] - r["none_again_ms"]) * 500, 1)
    r["sampling_none_spread_us"] = round(abs(r["sampling_none_again_ms"] - r["sampling_none_ms"]) * 1e3, 1)
    r["sampling_degree_4096_delta_us"] = round((r["sampling_degree_4096_ms"] + r["sampling_degree_4096_again_ms"]
                                                - r["sampling_none_ms"] - r["sampling_none_again_ms"]) * 500, 1)
    return r


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    result = {"bench": "constraint", "kernel": kernel_numbers()}
    if "--no-step" not in sys.argv:
        result["engine"] = engine_numbers()
    print(json.dumps(result))
