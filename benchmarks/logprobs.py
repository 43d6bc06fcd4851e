"""Token log-probabilities (csrc/logprobs.hip): kernel time against the same result from tensor ops and against greedy_argmax
(one read of the same bytes), and the cost inside the captured headline decode step.  One JSON line.

    python benchmarks/logprobs.py            # kernel and step
    python benchmarks/logprobs.py --no-step  # kernel only

Kernel numbers: device events around replays of a hipGraph holding one call per buffer of a rotating set (the set exceeds
the 256 MiB Infinity Cache, so every call reads its logits from HBM; ``*_same_buffer_us`` re-reads one 19 MB buffer, which is
what the decode step does right after the lm_head wrote it); each pair alternated in one process, median of the rounds.
Step numbers: median ms per replay of the captured step, Qwen2.5-7B W4A16, batch 64, context 512, set up as
benchmarks/step_times.py does; ``None`` is measured twice (first and last) -- their difference is the run-to-run spread."""
import json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_llama_amd.sampling import greedy_argmax, token_logprobs

DEV = "cuda"
VOCAB = 152064
HBM_PEAK_TBS = 8.0       # spec; ~6.3 TB/s is what a float4 copy achieves on this part
ROUNDS = 7


def graph_us(fn, buffers, replays=5):
    """us per call of ``fn(buffer)``: one call per buffer captured into a graph, replayed."""
    for b in buffers[:2]:
        fn(b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for b in buffers:
            fn(b)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return g, e0.elapsed_time(e1) * 1e3 / (replays * len(buffers))


def regraph_us(g, calls, replays=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def torch_logprobs(logits, ids, k):
    """What a caller writes without the kernel."""
    lsm = torch.log_softmax(logits.float(), -1)
    chosen = lsm.gather(1, ids.view(-1, 1))
    if k:
        return chosen, torch.topk(lsm, k, dim=-1)
    return chosen


def kernel_numbers():
    out = {}
    for rows in (64, 4096):
        nbuf = max(2, -(-(320 << 20) // (rows * VOCAB * 2)))
        gen = torch.Generator(device=DEV).manual_seed(rows)
        buffers = [(torch.randn(rows, VOCAB, device=DEV, generator=gen) * 4).half() for _ in range(nbuf)]
        ids = torch.randint(0, VOCAB, (rows,), device=DEV, generator=gen)
        nbytes = rows * VOCAB * 2
        for k in (0, 5, 20):
            gk, _ = graph_us(lambda z: token_logprobs(z, ids, k), buffers)
            gt, _ = graph_us(lambda z: torch_logprobs(z, ids, k), buffers)
            tk, tt = [], []
            for _ in range(ROUNDS):  # alternated
                tk.append(regraph_us(gk, nbuf))
                tt.append(regraph_us(gt, nbuf))
            mk, mt = statistics.median(tk), statistics.median(tt)
            out[f"rows{rows}_k{k}"] = {"kernel_us": round(mk, 2), "tensor_ops_us": round(mt, 2), "ratio": round(mt / mk, 2),
                                       "kernel_min_max_us": [round(min(tk), 2), round(max(tk), 2)],
                                       "kernel_tb_per_s": round(nbytes / mk / 1e6, 3),
                                       "kernel_share_of_hbm_peak": round(nbytes / mk / 1e6 / HBM_PEAK_TBS, 3)}
            del gk, gt
        if rows == 64:
            ga, _ = graph_us(greedy_argmax, buffers)
            g0, _ = graph_us(lambda z: token_logprobs(z, ids, 0), buffers)
            same = [buffers[0]] * nbuf
            gs, _ = graph_us(lambda z: token_logprobs(z, ids, 0), same)
            gas, _ = graph_us(greedy_argmax, same)
            ta, t0, ts, tas = [], [], [], []
            for _ in range(ROUNDS):
                ta.append(regraph_us(ga, nbuf)); t0.append(regraph_us(g0, nbuf))
                ts.append(regraph_us(gs, nbuf)); tas.append(regraph_us(gas, nbuf))
            out["rows64_vs_argmax"] = {"argmax_us": round(statistics.median(ta), 2), "kernel_k0_us": round(statistics.median(t0), 2),
                                       "argmax_same_buffer_us": round(statistics.median(tas), 2),
                                       "kernel_k0_same_buffer_us": round(statistics.median(ts), 2),
                                       "argmax_tb_per_s": round(nbytes / statistics.median(ta) / 1e6, 3)}
            del ga, g0, gs, gas
        del buffers
        torch.cuda.empty_cache()
    return out


def step_numbers(steps=60):
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
    eng = DecodeEngine(model, max_batch=B, max_seq_len=512 + steps + 8, device=DEV)

    def run(logprobs):
        first = eng.synthetic_context(B, 512, seed=1)
        evs = []

        def on_step(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)

        eng.decode(first, steps, use_graph=True, on_step=on_step, logprobs=logprobs)
        torch.cuda.synchronize()
        d = [evs[i].elapsed_time(evs[i + 1]) for i in range(10, len(evs) - 1)]  # the first replays of a fresh graph are slow
        return statistics.median(d)

    run(None)  # warm every shape
    res = {}
    for name, lp in (("none", None), ("k0", 0), ("k5", 5), ("k20", 20), ("none_again", None)):
        res[name + "_ms"] = round(run(lp), 4)
    for name in ("k0", "k5", "k20"):
        res[name + "_delta_us"] = round((res[name + "_ms"] - res["none_ms"]) * 1e3, 1)
    res["none_spread_us"] = round(abs(res["none_again_ms"] - res["none_ms"]) * 1e3, 1)
    return res


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    result = {"bench": "logprobs", "vocab": VOCAB, "dtype": "fp16", "kernel": kernel_numbers()}
    if "--no-step" not in sys.argv:
        result["step"] = step_numbers()
    print(json.dumps(result))
