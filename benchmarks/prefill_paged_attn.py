"""GPU time of prefill_paged_attention (causal prefill over the paged KV pool) at Qwen2.5-7B head geometry (Hq 28, Hkv 4,
D 128, fp16): cached context x chunk x batch, contiguous vs randomly permuted tables, causal TFLOP/s against
4 * D * sum over queries of the keys each attends; at ctx = 0 flash_attention2_no_pad on the same shape, alternated with
the new kernel in one process.  ``--e2e``: TTFT of one 8192-token prompt on the synthetic Qwen2.5-7B W4A16 model,
one-step prefill vs chunk_size 512 / 2048.  Device-event timing, warm-up and repeats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lite_llama_amd.kernels as K  # noqa: E402

dev = "cuda"
HQ, HKV, D = int(os.environ.get("HQ", 28)), int(os.environ.get("HKV", 4)), int(os.environ.get("D", 128))
SCALE = 1.4426950408889634 / D ** 0.5


def timed(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_case(batch, ctx, chunk, scattered, gen):
    total = ctx + chunk
    rows = batch * total
    pool = (torch.randn(rows, 2 * HKV, D, device=dev, generator=gen) * 0.5).half()
    order = torch.randperm(rows, device=dev, generator=gen) if scattered else torch.arange(rows, device=dev)
    table = order.view(batch, total).to(torch.int32).contiguous()
    q = torch.randn(batch * chunk, HQ, D, device=dev, generator=gen).half()
    i32 = dict(dtype=torch.int32, device=dev)
    req = torch.arange(batch, **i32)
    start = torch.arange(batch, **i32) * chunk
    qlen = torch.full((batch,), chunk, **i32)
    ctxl = torch.full((batch,), ctx, **i32)
    out = torch.empty_like(q)
    run = lambda: K.prefill_paged_attention(q, pool, SCALE, table, req, start, qlen, ctxl, chunk, ctx, out=out)  # noqa: E731
    keys = chunk * ctx + chunk * (chunk + 1) / 2  # keys attended, summed over the queries of one sequence
    flops = 4.0 * D * keys * HQ * batch
    return run, flops, (q, pool, start, qlen)


def kernels(args):
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for batch in (1, 8):
        for ctx in (0, 2048, 8192):
            for chunk in (512, 2048):
                for scattered in (False, True):
                    run, flops, (q, pool, start, qlen) = kernel_case(batch, ctx, chunk, scattered, gen)
                    key = f"b{batch}_ctx{ctx}_chunk{chunk}_{'scattered' if scattered else 'contiguous'}"
                    if ctx == 0 and not scattered:
                        # alternate the two kernels on the same shape (identity table): A B A B ...
                        k, v = pool[:, :HKV], pool[:, HKV:]
                        fa = lambda: K.flash_attention2_no_pad(q, k, v, SCALE, start, qlen, chunk)  # noqa: E731
                        a, b = [], []
                        for _ in range(args.alternations):
                            a.append(timed(run, args.warmup, args.reps))
                            b.append(timed(fa, args.warmup, args.reps))
                        ms, ms_fa = min(a), min(b)
                        res[key] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1),
                                    "fa_prefill_ms": round(ms_fa, 4), "ratio": round(ms / ms_fa, 3)}
                    else:
                        ms = min(timed(run, args.warmup, args.reps) for _ in range(args.alternations))
                        res[key] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1)}
                    print(key, res[key], flush=True)
                    del run
    return res


def e2e(args):
    from lite_llama_amd.executor import DecodeEngine
    from lite_llama_amd.model import GEOMETRY, CausalLM
    from lite_llama_amd.quantization import QuantConfig

    geo = GEOMETRY["qwen2.5-7b"]
    quant = QuantConfig.int4_groupwise(128)
    model = CausalLM(geo, quant).init_synthetic(seed=0, quant=quant, device=dev)
    lp = args.prompt
    ids = torch.randint(0, geo.vocab_size, (1, lp), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    eng = DecodeEngine(model, max_batch=1, max_seq_len=lp + 16)
    res = {}
    for chunk in (None, 512, 2048):
        times, firsts = [], []
        for _ in range(args.e2e_reps + 1):  # the first run is a warm-up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            first = eng.prefill(ids, chunk_size=chunk)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
            firsts.append(int(first[0]))
        key = f"ttft_{lp}_{'oneshot' if chunk is None else f'chunk{chunk}'}"
        res[key] = {"ms": round(min(times[1:]), 2), "first_token": firsts[-1]}
        print(key, res[key], flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--e2e", action="store_true", help="also time the end-to-end TTFT (builds the 7B-geometry model)")
    ap.add_argument("--e2e-only", action="store_true")
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=8192)
    a = ap.parse_args()
    out = {}
    if not a.e2e_only:
        out["kernel"] = kernels(a)
    if a.e2e or a.e2e_only:
        out["e2e"] = e2e(a)
    print(json.dumps(out))
