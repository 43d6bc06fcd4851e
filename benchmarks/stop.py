"""Per-row stopping (csrc/decode_stop.hip, DecodeEngine.decode(stop=...)): what it costs and what the early exit returns.
One JSON line.

    python benchmarks/stop.py            # kernel, step and early exit
    python benchmarks/stop.py --no-step  # kernel only

Kernel: ll_decode_stop_advance against ll_decode_advance at batch 64, device events around replays of a hipGraph holding
200 launches (the step counter and the lengths are put back by two fills at the head of the graph); the stop kernel runs with
one stop id and four 8-token sequences that match the history at every step in all but their last token but one, and no row
ever finishes -- its longest path.  Alternated in one process, median of the rounds.
Step: median ms per replay of the captured step, Qwen2.5-7B W4A16, batch 64, context 512, set up as benchmarks/step_times.py
does, with criteria that never match against no ``stop``, on the bump pool and on the paged pool; ``none`` is measured twice
(first and last) -- their difference is the run-to-run spread.
Early exit: wall time of a 256-token captured decode in which every row ends by token 32 (``max_tokens`` 8 .. 32,
``check_every`` 8) against the same decode without ``stop``."""
import json, os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_llama_amd import _lib as L
from lite_llama_amd.executor.stopping import StopCriteria, StopState, stop_advance

DEV = "cuda"
ROUNDS = 7
LAUNCHES = 200


def replay_us(g, calls, replays=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def kernel_numbers(batch=64):
    cols = LAUNCHES + 1
    out = torch.zeros(batch, cols, dtype=torch.int64, device=DEV)
    step = torch.ones(1, dtype=torch.int64, device=DEV)
    nxt = torch.zeros(batch, dtype=torch.int64, device=DEV)
    input_ids = torch.zeros(batch, 1, dtype=torch.int64, device=DEV)
    positions = torch.zeros(batch, 1, dtype=torch.int64, device=DEV)
    sel = torch.arange(batch, dtype=torch.int32, device=DEV)
    seq_len = torch.ones(batch, dtype=torch.int32, device=DEV)
    req = torch.arange(batch, dtype=torch.int32, device=DEV)
    table = torch.zeros(batch, cols + 1, dtype=torch.int32, device=DEV)
    crit = StopCriteria(stop_token_ids=[9], stop_sequences=[[0] * 6 + [k, 0] for k in (1, 2, 3, 4)])
    state = StopState(crit, nxt, DEV)

    def plain():
        L.check(L.lib().ll_decode_advance(out.data_ptr(), out.stride(0), step.data_ptr(), nxt.data_ptr(), input_ids.data_ptr(),
                                          positions.data_ptr(), sel.data_ptr(), seq_len.data_ptr(), req.data_ptr(),
                                          table.data_ptr(), table.stride(0), table.stride(1), batch, L.stream_ptr()),
                "decode_advance")

    def stop():
        stop_advance(out, step, nxt, input_ids, positions, sel, seq_len, req, table, state)

    graphs = {}
    for name, fn in (("advance", plain), ("stop_advance", stop)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step.fill_(1)
            seq_len.fill_(1)
            for _ in range(LAUNCHES):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    assert int(state.running) == batch and int(step) == cols
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):  # alternated
        for name, g in graphs.items():
            times[name].append(replay_us(g, LAUNCHES))
    res = {"batch": batch}
    for name, t in times.items():
        res[name + "_us"] = round(statistics.median(t), 3)
        res[name + "_min_max_us"] = [round(min(t), 3), round(max(t), 3)]
    res["delta_us"] = round(res["stop_advance_us"] - res["advance_us"], 3)
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
    res = {}
    for pool, bs in (("bump", None), ("paged", 16)):
        eng = DecodeEngine(model, max_batch=B, max_seq_len=512 + 256 + 8, device=DEV, kv_block_size=bs)

        def run(stop, n=steps, timed=True):
            first = eng.synthetic_context(B, 512, seed=1)
            evs = []

            def on_step(i):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs.append(e)

            toks = eng.decode(first, n, use_graph=True, on_step=on_step if timed else None, stop=stop)
            torch.cuda.synchronize()
            if not timed:
                return toks
            d = [evs[i].elapsed_time(evs[i + 1]) for i in range(10, len(evs) - 1)]  # the first replays of a fresh graph are slow
            return statistics.median(d)

        seen = set(run(None, timed=False).unique().tolist())  # warms every shape; ids the run never emits cannot match
        free = [t for t in range(geo.vocab_size - 1, 0, -1) if t not in seen][:12]
        never = StopCriteria(stop_token_ids=free[:4], stop_sequences=[free[4:12], free[4:6]], max_tokens=[1 << 20] * B)
        r = {}
        for name, stop in (("none", None), ("stop", never), ("none_again", None), ("stop_again", never)):
            r[name + "_ms"] = round(run(stop), 4)
        r["stop_delta_us"] = round((r["stop_ms"] + r["stop_again_ms"] - r["none_ms"] - r["none_again_ms"]) * 500, 1)
        r["none_spread_us"] = round(abs(r["none_again_ms"] - r["none_ms"]) * 1e3, 1)
        # early exit: every row ends by token 32 of 256
        gen = torch.Generator().manual_seed(2)
        limits = torch.randint(8, 33, (B,), generator=gen).tolist()
        limits[0] = 32
        early = StopCriteria(max_tokens=limits, check_every=8)
        wall = {}
        for name, stop in (("full", None), ("early", early), ("full_again", None), ("early_again", early)):
            first = eng.synthetic_context(B, 512, seed=1)
            torch.cuda.synchronize()
            marks = {}

            def first_replay(i):
                if i == 0:
                    marks["loop"] = time.perf_counter()   # warm-up and capture are behind, the device is idle

            t0 = time.perf_counter()
            eng.decode(first, 256, use_graph=True, stop=stop, on_step=first_replay)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            wall[name + "_ms"] = round((t1 - t0) * 1e3, 2)                  # with warm-up step and capture
            wall[name + "_loop_ms"] = round((t1 - marks["loop"]) * 1e3, 2)  # the replays alone
            if stop is not None:
                wall["steps_run"] = eng.last_steps_run
        wall["ratio"] = round((wall["full_ms"] + wall["full_again_ms"]) / (wall["early_ms"] + wall["early_again_ms"]), 2)
        wall["loop_ratio"] = round((wall["full_loop_ms"] + wall["full_again_loop_ms"])
                                   / (wall["early_loop_ms"] + wall["early_again_loop_ms"]), 2)
        r["early_exit_256"] = wall
        res[pool] = r
        del eng
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    result = {"bench": "stop", "kernel": kernel_numbers()}
    if "--no-step" not in sys.argv:
        result["engine"] = engine_numbers()
    print(json.dumps(result))
