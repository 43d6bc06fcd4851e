"""Decode attention over a shared prompt prefix at Qwen2.5-7B head geometry (Hq 28, Hkv 4, D 128, fp16), per layer:
(a) the one-launch decode attention (rope + KV scatter + flash-decoding + merge) on the aliased table -- the route the engine
takes without the shared-prefix kernel -- against (b) rope_and_cache + shared_prefix_decode_attention, for prefix lengths
128 .. 4096, tails of 32 tokens, batch 64 and 16.  (a) and (b) are captured in hipGraphs (as the decode step runs them) and their replays timed alternately on device
events; every shape is warmed up first.  ``--mode profile`` launches each route a few times for a ``rocprofv3 --kernel-trace --stats`` run of its own;
``--mode step`` times the whole captured decode step of the synthetic Qwen2.5-7B W4A16 model, shared against unshared; with
``--kv-block-size`` on the paged pool (``--share-blocks``: per-block share counts, which ``shared`` and ``samples`` need there);
``--variants`` picks what is alternated: ``unshared`` (synthetic context), ``shared`` (one prefix + tails of 32), ``samples``
(ONE prompt of ``--prefix`` tokens x ``--batch`` samples) and ``repeated`` (that prompt prefilled ``--batch`` times: what a user
can do without shared blocks).  ``--mode fork`` times PagedKVPool.fork alone at that model's cache geometry.
The algorithmic bytes of (b) are computed from the shapes and printed next to the times."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lite_llama_amd._lib as L  # noqa: E402
from lite_llama_amd.kernels.attention import decode_attention, shared_prefix_decode_attention  # noqa: E402
from lite_llama_amd.kernels.norm_act import rope_and_cache  # noqa: E402

dev = "cuda"
HQ, HKV, D = int(os.environ.get("HQ", 28)), int(os.environ.get("HKV", 4)), int(os.environ.get("D", 128))
TAIL = 32
PREFIXES = (128, 256, 512, 1024, 2048, 4096)


def captured(fn, launches):
    """``launches`` calls of ``fn`` in one hipGraph: the decode step replays its launches from a graph, and eager launches of
    kernels this short would time the host's enqueue instead of the device."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    return graph


def timed(graph, launches, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (launches * replays) * 1e3  # us per call of the route


def case(batch, prefix, gen):
    """A decode step's attention inputs: every row holds the shared prefix + TAIL own tokens and feeds one new token."""
    own = TAIL + 1
    rows = prefix + batch * own
    pool = (torch.randn(rows, 2 * HKV, D, device=dev, generator=gen) * 0.5).half()
    table = torch.zeros(batch, prefix + own, dtype=torch.int32, device=dev)
    table[:, :prefix] = torch.arange(prefix, device=dev, dtype=torch.int32)
    table[:, prefix:] = (prefix + torch.arange(batch * own, device=dev, dtype=torch.int32)).view(batch, own)
    i32 = dict(dtype=torch.int32, device=dev)
    req = torch.arange(batch, **i32)
    seq = torch.full((batch,), prefix + own, **i32)
    sel = table[:, prefix + own - 1].contiguous()
    pos = torch.full((batch,), prefix + own - 1, dtype=torch.int64, device=dev)
    ang = torch.arange(prefix + own, device=dev).float()[:, None] * torch.logspace(0, -4, D // 2, device=dev)[None]
    cos, sin = torch.cos(ang).repeat(1, 2).half(), torch.sin(ang).repeat(1, 2).half()
    q = torch.randn(batch, HQ, D, device=dev, generator=gen).half()
    kv = torch.randn(batch, 2 * HKV, D, device=dev, generator=gen).half()
    scale, top = D ** -0.5, prefix + own
    out = torch.empty_like(q)

    def old():
        return decode_attention(q, kv, cos, sin, pos, sel, pool, scale, table, req, seq, top)

    def new():
        rope_and_cache(q, kv, cos, sin, batch, 1, sel, pool, positions=pos)
        return shared_prefix_decode_attention(q, pool[:, :HKV], pool[:, HKV:], scale, table, req, seq, top, prefix, 0, out=out)

    return old, new


def algorithmic_bytes(batch, prefix):
    """What route (b) has to move: the prefix K/V once, the tails' K/V, q, out and the fp32 records (written, then read)."""
    top = prefix + TAIL + 1
    splits = L.lib().ll_shared_prefix_num_splits(batch, HQ, HKV, D, prefix, top)
    parts = -(-(top - prefix) // 128)
    kv_row = 2 * HKV * D * 2
    return {"prefix_kv": prefix * kv_row, "tail_kv": batch * (TAIL + 1) * kv_row, "q_out": 2 * batch * HQ * D * 2,
            "records": 2 * batch * HQ * (splits + parts) * (D + 1) * 4, "splits": splits}


def ab(args):
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for batch in (64, 16):
        for prefix in PREFIXES:
            old, new = case(batch, prefix, gen)
            assert old() is not None and new() is not None
            ga, gb = captured(old, args.launches), captured(new, args.launches)
            for _ in range(args.warmup):
                ga.replay()
                gb.replay()
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(args.alternations):
                a.append(timed(ga, args.launches, args.replays))
                b.append(timed(gb, args.launches, args.replays))
            a.sort()
            b.sort()
            by = algorithmic_bytes(batch, prefix)
            key = f"b{batch}_p{prefix}"
            res[key] = {"old_us": round(a[len(a) // 2], 2), "new_us": round(b[len(b) // 2], 2),
                        "old_range_us": [round(a[0], 2), round(a[-1], 2)], "new_range_us": [round(b[0], 2), round(b[-1], 2)],
                        "bytes": by}
            print(key, res[key], flush=True)
    return res


def profile(args):
    gen = torch.Generator(device=dev).manual_seed(0)
    for batch in (64, 16):
        for prefix in (args.prefix,):
            old, new = case(batch, prefix, gen)
            for _ in range(20):
                old()
                new()
            torch.cuda.synchronize()
    return {"profiled": True}


def step(args):
    from lite_llama_amd.executor import DecodeEngine
    from lite_llama_amd.model import GEOMETRY, CausalLM
    from lite_llama_amd.quantization import QuantConfig

    geo = GEOMETRY["qwen2.5-7b"]
    quant = QuantConfig.int4_groupwise(128)
    with torch.device(dev):
        model = CausalLM(geo, quant)
    model.init_synthetic(seed=0, quant=quant, device=dev)
    model.compact_weights()
    b, p, steps = args.batch, args.prefix, args.steps
    gen = torch.Generator(device=dev).manual_seed(1)
    kw = {}
    if args.kv_block_size:
        kw["kv_block_size"] = args.kv_block_size
    if args.share_blocks:
        kw["kv_share_blocks"] = True
    eng = DecodeEngine(model, max_batch=b, max_seq_len=p + TAIL + steps + 8, device=dev, **kw)

    def run(first):
        evs = []

        def on_step(i):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)

        eng.decode(first, steps, use_graph=True, on_step=on_step)
        torch.cuda.synchronize()
        d = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(10, len(evs) - 1))
        return round(d[len(d) // 2], 4)

    def used():
        return {"blocks": eng.pool.num_blocks - 1 - eng.pool.free_blocks} if eng.paged else {"rows": eng.pool.used}

    def prefilled(variant, fn):
        """``fn`` = a prefill: host clock around it, ending in a device synchronise; the pool's use right after it."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = fn()
        torch.cuda.synchronize()
        res.setdefault(variant + "_prefill_ms", []).append(round((time.perf_counter() - t0) * 1e3, 2))
        res[variant + "_pool"] = used()
        if variant == "shared" and not eng.paged:
            res["pool_rows_shared"] = eng.pool.used
        return first

    res = {}
    pre = torch.randint(0, geo.vocab_size, (p,), device=dev, generator=gen)
    tails = torch.randint(0, geo.vocab_size, (b, TAIL), device=dev, generator=gen)
    chunk = args.chunk_size or None
    starts = {
        "unshared": lambda: eng.synthetic_context(b, p + TAIL, seed=1),
        "shared": lambda: prefilled("shared", lambda: eng.prefill(tails, shared_prefix_ids=pre)),
        "samples": lambda: prefilled("samples", lambda: eng.prefill(pre.view(1, p), chunk_size=chunk, num_samples=b)),
        "repeated": lambda: prefilled("repeated", lambda: eng.prefill(pre.view(1, p).repeat(b, 1), chunk_size=chunk)),
    }
    for _ in range(args.alternations):
        for variant in args.variants.split(","):
            res.setdefault(variant + "_ms", []).append(run(starts[variant]()))
            res[variant + "_shared_prefix_len"] = eng.info.shared_prefix_len
    res["pool_rows_unshared"] = b * (p + TAIL)
    res["geometry"] = {"batch": b, "prefix": p, "tail": TAIL, "steps": steps, **kw}
    print(res, flush=True)
    return res


def fork(args):
    """PagedKVPool.fork alone: the Qwen2.5-7B cache (28 layers, rows of 2 * 4 * 128 fp16 = 2 KB), one source of
    ``--prefix`` tokens, ``--batch - 1`` children.  The bytes are computed from the shapes: only the partial last block is
    copied -- ``prefix % block`` rows per child and layer, read and written once."""
    from lite_llama_amd.executor.paged_kv import PagedKVPool

    layers, bs, n, p = 28, args.kv_block_size or 16, args.batch - 1, args.prefix
    per_req = -(-(p + 1) // bs)
    pool = PagedKVPool(layers, args.batch * per_req + 1, bs, HKV, D, dev, args.batch, p + 1, share_blocks=True)
    table = torch.zeros(args.batch, p + 1, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    src, dst, lens = torch.zeros(n, **i32), torch.arange(1, n + 1, **i32), torch.full((n,), p, **i32)
    pool.admit(torch.zeros(1, **i32), torch.full((1,), p, **i32), p, table)
    times = []
    for _ in range(args.warmup + args.replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pool.fork(src, dst, lens, table)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
        pool.release(dst)
    assert pool.error == 0
    times = sorted(times[args.warmup:])
    us = times[len(times) // 2]
    copied = n * layers * (p % bs) * pool.row_bytes
    res = {"children": n, "block": bs, "prefix": p, "rows_copied_per_child_and_layer": p % bs, "bytes_read": copied,
           "bytes_written": copied, "fork_us": round(us, 1), "fork_range_us": [round(times[0], 1), round(times[-1], 1)],
           "copy_GBps_read_plus_write": round(2 * copied / (us * 1e-6) / 1e9, 1) if copied else None}
    print(res, flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ab", "profile", "step", "fork"), default="ab")
    ap.add_argument("--warmup", type=int, default=5, help="graph replays before the timed samples")
    ap.add_argument("--launches", type=int, default=20, help="calls of a route captured in one graph")
    ap.add_argument("--replays", type=int, default=20, help="graph replays per timed sample")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--kv-block-size", type=int, default=0, help="step / fork: the paged pool with blocks of that many rows")
    ap.add_argument("--share-blocks", action="store_true", help="step: per-block share counts (kv_share_blocks)")
    ap.add_argument("--variants", default="unshared,shared", help="step: comma-separated, alternated in this order")
    ap.add_argument("--chunk-size", type=int, default=0, help="step: chunk_size of the samples / repeated prefills")
    a = ap.parse_args()
    print(json.dumps({a.mode: {"ab": ab, "profile": profile, "step": step, "fork": fork}[a.mode](a)}))
