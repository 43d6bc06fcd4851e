"""Presence / frequency penalties, logit bias and seeded draws (csrc/sampler_penalties.hip, sampling.apply_penalties /
seeded_uniform): what the one-pass penalty launch costs next to the repetition penalty whose place it takes, and what a
sampled step costs with the new options.  One JSON line.

    python benchmarks/sampler_penalties.py            # kernels and step
    python benchmarks/sampler_penalties.py --no-step  # kernels only

Kernels: batch 64, vocabulary 152 064, fp16 logits (randn x 2), a generated span of 256 tokens; device events around replays of
a hipGraph holding 100 launches; ll_repetition_penalty at 1.1 (the yardstick: the code of the parent commit, untouched),
ll_logit_penalties with the repetition penalty alone, with all three penalties, and with all three and a 16-entry bias per row;
ll_seeded_uniform next to torch.rand(64).  Every variant is timed in two alternated runs of ROUNDS rounds each: the difference
of the yardstick's two runs is the run-to-run spread.
Step: median ms per replay of the captured step, Qwen2.5-7B W4A16, batch 64, context 512, set up as benchmarks/step_times.py
does, with ``sampling`` set (temperature 0.8, top_p 0.9): with the repetition penalty 1.1 (the yardstick), with presence and
frequency penalties and a 16-entry bias on top, with neither (no penalty launch), and with seeds against torch.rand; each
measured twice, alternated."""
import json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_llama_amd.sampling import LogitBias, SamplingParams, apply_penalties, apply_repetition_penalty, seeded_uniform

DEV = "cuda"
ROUNDS = 7
LAUNCHES = 100
VOCAB = 152064
SPAN = 256


def replay_us(g, calls, replays=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def bias_rows(batch, g):
    return [{int(t): float(v) for t, v in zip(torch.randint(0, VOCAB, (16,), generator=g), torch.randn(16, generator=g))}
            for _ in range(batch)]


def timed(fns, yardstick):
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
    res = {}
    for again in ("", "_again"):
        times = {name: [] for name in graphs}
        for _ in range(ROUNDS):  # alternated
            for name, gr in graphs.items():
                times[name].append(replay_us(gr, LAUNCHES))
        for name, x in times.items():
            res[name + again + "_us"] = round(statistics.median(x), 2)
            res[name + again + "_min_max_us"] = [round(min(x), 2), round(max(x), 2)]
    res[yardstick + "_spread_us"] = round(abs(res[yardstick + "_again_us"] - res[yardstick + "_us"]), 2)
    for name in graphs:
        if name != yardstick:
            res[name + "_delta_us"] = round((res[name + "_us"] + res[name + "_again_us"] - res[yardstick + "_us"]
                                             - res[yardstick + "_again_us"]) / 2, 2)
    return res


def kernel_numbers(batch=64):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(batch, VOCAB, generator=g) * 2).half().to(DEV)
    ids = torch.randint(0, VOCAB, (batch, SPAN), generator=g).to(DEV)
    mask = torch.ones(batch, SPAN, dtype=torch.bool, device=DEV)
    bias = LogitBias(bias_rows(batch, g), batch, VOCAB, DEV)
    seeds = torch.arange(batch, dtype=torch.int64, device=DEV)
    column = torch.ones(1, dtype=torch.int64, device=DEV)
    fns = {
        "repetition_penalty": lambda: apply_repetition_penalty(logits, ids, mask, 1.1),
        "penalties_repetition_only": lambda: apply_penalties(logits, ids, mask, 1.1),
        "penalties_all_three": lambda: apply_penalties(logits, ids, mask, 1.1, 0.5, 0.25),
        "penalties_all_three_bias16": lambda: apply_penalties(logits, ids, mask, 1.1, 0.5, 0.25, bias),
    }
    assert torch.equal(fns["repetition_penalty"](), fns["penalties_repetition_only"]())
    res = {"batch": batch, "vocab": VOCAB, "dtype": "float16", "span": SPAN}
    res.update(timed(fns, "repetition_penalty"))
    res.update(timed({"torch_rand": lambda: torch.rand(batch, device=DEV),
                      "seeded_uniform": lambda: seeded_uniform(seeds, column)}, "torch_rand"))
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
    base = dict(temperature=0.8, top_p=0.9)
    bias = bias_rows(B, torch.Generator().manual_seed(1))
    variants = {
        "sampling_rep": SamplingParams(repetition_penalty=1.1, **base),
        "sampling_rep_presence_frequency_bias16": SamplingParams(repetition_penalty=1.1, presence_penalty=0.5,
                                                                 frequency_penalty=0.25, logit_bias=bias, **base),
        "sampling_rep_seeded": SamplingParams(repetition_penalty=1.1, seed=7, **base),
        "sampling_no_penalty": SamplingParams(**base),
    }

    def run(sampling, n=steps):
        first = eng.synthetic_context(B, 512, seed=1)
        evs = []

        def on_step(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)

        eng.decode(first, n, use_graph=True, on_step=on_step, sampling=sampling)
        torch.cuda.synchronize()
        d = [evs[i].elapsed_time(evs[i + 1]) for i in range(10, len(evs) - 1)]  # the first replays of a fresh graph are slow
        return statistics.median(d)

    run(None)  # warms every shape
    r = {"greedy_ms": round(run(None), 4)}
    for again in ("", "_again"):
        for name, sp in variants.items():
            r[name + again + "_ms"] = round(run(sp), 4)
    r["sampling_rep_spread_us"] = round(abs(r["sampling_rep_again_ms"] - r["sampling_rep_ms"]) * 1e3, 1)
    for name in variants:
        if name != "sampling_rep":
            r[name + "_delta_us"] = round((r[name + "_ms"] + r[name + "_again_ms"] - r["sampling_rep_ms"]
                                           - r["sampling_rep_again_ms"]) * 500, 1)
    return r


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    result = {"bench": "sampler_penalties", "kernel": kernel_numbers()}
    if "--no-step" not in sys.argv:
        result["engine"] = engine_numbers()
    print(json.dumps(result))
