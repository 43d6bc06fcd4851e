"""Top-k / min-p sampling (csrc/sampler_filters.hip, sampling.sample_filtered): what the filtered draw costs next to the
nucleus draw it extends, and what a sampled step costs with the filters.  One JSON line.

    python benchmarks/sampler_filters.py            # kernels and step
    python benchmarks/sampler_filters.py --no-step  # kernels only

Kernels: batch 64, vocabulary 152 064, fp16 logits (randn x 2), temperature 0.8, top_p 0.9; device events around replays of a
hipGraph holding 100 launches; ll_sample_top_p (the yardstick), ll_sample_filtered with both filters off, with k = 50, with
min_p = 0.05 and with both; and, for context, a torch composition of the k = 50 case (topk, whose values come sorted,
softmax, cumsum, nucleus mask and a searchsorted inverse CDF: several launches, exactly k tokens, no ties).  Every variant is
timed in two alternated runs of ROUNDS rounds each: the difference of the yardstick's two runs is the run-to-run spread.
Step: median ms per replay of the captured step, Qwen2.5-7B W4A16, batch 64, context 512, set up as benchmarks/step_times.py
does, with ``sampling`` set (temperature 0.8, top_p 0.9): without the filters, with k = 50, with min_p = 0.05 and with both,
each measured twice, alternated."""
import json, os, statistics, sys, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_llama_amd.sampling import sample_filtered, sample_top_p

DEV = "cuda"
ROUNDS = 7
LAUNCHES = 100
VOCAB = 152064


def replay_us(g, calls, replays=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def torch_top_k_top_p(logits, t, p, k, u):
    """The usual composition, for context: top-k values (sorted by topk), softmax, cumsum, nucleus mask, inverse CDF."""
    vals, idx = torch.topk(logits.float(), k, dim=-1)
    probs = torch.softmax(vals / t, dim=-1)
    cum = torch.cumsum(probs, dim=-1)
    probs = torch.where(cum - probs > p, torch.zeros_like(probs), probs)
    cdf = torch.cumsum(probs, dim=-1)
    pick = torch.searchsorted(cdf, (u * cdf[:, -1]).view(-1, 1), right=True).clamp(max=k - 1)
    return idx.gather(1, pick)


def kernel_numbers(batch=64):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(batch, VOCAB, generator=g) * 2).half().to(DEV)
    u = torch.rand(batch, generator=g).to(DEV)
    t = torch.full((batch,), 0.8, device=DEV)
    p = torch.full((batch,), 0.9, device=DEV)
    k50 = torch.full((batch,), 50, dtype=torch.int32, device=DEV)
    k0 = torch.zeros(batch, dtype=torch.int32, device=DEV)
    mp = torch.full((batch,), 0.05, device=DEV)
    mp0 = torch.zeros(batch, device=DEV)
    fns = {
        "sample_top_p": lambda: sample_top_p(logits, t, p, uniform=u),
        "filtered_off": lambda: sample_filtered(logits, t, p, k0, mp0, uniform=u),
        "filtered_k50": lambda: sample_filtered(logits, t, p, k50, mp0, uniform=u),
        "filtered_min_p": lambda: sample_filtered(logits, t, p, k0, mp, uniform=u),
        "filtered_k50_min_p": lambda: sample_filtered(logits, t, p, k50, mp, uniform=u),
        "torch_topk_sort_k50": lambda: torch_top_k_top_p(logits, 0.8, 0.9, 50, u),
    }
    assert torch.equal(fns["sample_top_p"](), fns["filtered_off"]())
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
    res = {"batch": batch, "vocab": VOCAB, "dtype": "float16", "temperature": 0.8, "top_p": 0.9}
    for again in ("", "_again"):
        times = {name: [] for name in graphs}
        for _ in range(ROUNDS):  # alternated
            for name, gr in graphs.items():
                times[name].append(replay_us(gr, LAUNCHES))
        for name, x in times.items():
            res[name + again + "_us"] = round(statistics.median(x), 2)
            res[name + again + "_min_max_us"] = [round(min(x), 2), round(max(x), 2)]
    res["sample_top_p_spread_us"] = round(abs(res["sample_top_p_again_us"] - res["sample_top_p_us"]), 2)
    for name in graphs:
        if name != "sample_top_p":
            res[name + "_delta_us"] = round((res[name + "_us"] + res[name + "_again_us"] - res["sample_top_p_us"]
                                             - res["sample_top_p_again_us"]) / 2, 2)
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
    base = dict(temperature=0.8, top_p=0.9, repetition_penalty=1.0)
    variants = {"sampling": types.SimpleNamespace(**base), "sampling_k50": types.SimpleNamespace(top_k=50, **base),
                "sampling_min_p": types.SimpleNamespace(min_p=0.05, **base),
                "sampling_k50_min_p": types.SimpleNamespace(top_k=50, min_p=0.05, **base)}

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
    r["sampling_spread_us"] = round(abs(r["sampling_again_ms"] - r["sampling_ms"]) * 1e3, 1)
    for name in variants:
        if name != "sampling":
            r[name + "_delta_us"] = round((r[name + "_ms"] + r[name + "_again_ms"] - r["sampling_ms"] - r["sampling_again_ms"]) * 500, 1)
    return r


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    result = {"bench": "sampler_filters", "kernel": kernel_numbers()}
    if "--no-step" not in sys.argv:
        result["engine"] = engine_numbers()
    print(json.dumps(result))
