"""Greedy speculative decoding (csrc/speculative.hip, DecodeEngine.decode(speculate=...)): what a verify step costs next to
the plain decode step, and what acceptance it needs to pay.  One JSON line.

    python benchmarks/speculative.py

Qwen2.5-7B, synthetic W4A16 g128 weights, paged pool (blocks of 16), a real prefill of random 512-token prompts, batch 1
and 8, k = 2 and 4.  Per (batch, k), in one process: median ms per replay of
  plain        the captured one-token step of ``decode()``;
  verify_empty the captured verify step with empty drafts (``ngram=False``, no prediction): one token per row and step;
  verify_full  the captured verify step under full acceptance (``predicted_ids`` = the run's own output): k + 1 tokens per
               row and step after the first;
``break_even`` = verify_ms / plain_ms - 1, the mean number of accepted drafts per step from which speculation is faster,
tokens/s both ways, and ``attention_share``: the chunk-step attention launch at the verify shape (every row k + 1
queries over a context of 576), timed alone in a graph of one launch per layer, over the verify step.
Device events between replays; the first replays of a fresh graph are left out; the full-acceptance run, which is short,
is repeated four times and its intervals pooled."""
import json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
CTX = 512
NEW = 160
SKIP = 6


def step_ms(eng, prefill, n, reps=1, **kw):
    """Median ms between the replays of ``reps`` decodes (a fresh prefill each) -> (tokens, median, intervals timed)."""
    pooled = []
    for _ in range(reps):
        toks, d = _intervals(eng, prefill(), n, **kw)
        pooled += d
    return toks, statistics.median(pooled), len(pooled)


def _intervals(eng, first, n, **kw):
    evs = []

    def on_step(i):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)

    toks = eng.decode(first, n, use_graph=True, on_step=on_step, **kw)
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    evs.append(end)
    torch.cuda.synchronize()
    d = [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)]
    return toks, d[SKIP:-1]                           # the last interval holds the exit's bookkeeping


def attention_us(eng, model, batch, k, ctx, rounds=5):
    """The verify step's attention launches alone: one per layer in a graph, the engine's pool and table as they stand."""
    import math

    from lite_llama_amd.kernels.attention import prefill_paged_attention

    at = model.layers[0].self_attn
    layers = len(model.layers)
    w = k + 1
    q = (torch.randn(batch * w, at.num_heads, at.head_dim, device=DEV) * 0.5).half()
    out = torch.empty_like(q)
    i32 = dict(dtype=torch.int32, device=DEV)
    req, start = torch.arange(batch, **i32), torch.arange(batch, **i32) * w
    q_len, ctx_len = torch.full((batch,), w, **i32), torch.full((batch,), ctx, **i32)
    scale = 1.0 / math.sqrt(at.head_dim) * 1.4426950408889634

    def launches():
        for li in range(layers):
            prefill_paged_attention(q, eng.pool.kv_buffer[li], scale, eng.info.b_req_tokens_table, req, start, q_len, ctx_len,
                                    w, eng.max_seq_len, out=out)

    launches()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launches()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / 10)
    return statistics.median(times)               # us per step's worth of attention launches


def main():
    from lite_llama_amd.executor import DecodeEngine, Speculation
    from lite_llama_amd.model import GEOMETRY, CausalLM
    from lite_llama_amd.quantization import QuantConfig

    geo = GEOMETRY["qwen2.5-7b"]
    quant = QuantConfig.for_runtime_scheme("int4")
    with torch.device(DEV):
        model = CausalLM(geo, quant)
    model.init_synthetic(seed=0, quant=quant, device=DEV)
    if hasattr(model, "compact_weights"):
        model.compact_weights()
    res = {"bench": "speculative", "model": "qwen2.5-7b W4A16 g128 (synthetic)", "ctx": CTX, "new_tokens": NEW,
           "device": torch.cuda.get_device_name(0), "points": []}
    gen = torch.Generator().manual_seed(5)
    for batch in (1, 8):
        ids = torch.randint(0, geo.vocab_size, (batch, CTX), generator=gen).to(DEV)
        eng = DecodeEngine(model, max_batch=batch, max_seq_len=CTX + NEW + 24, device=DEV, kv_block_size=16)
        eng.decode(eng.prefill(ids), 8, use_graph=True)                        # warms every plain shape
        _, plain_ms, _ = step_ms(eng, lambda: eng.prefill(ids), NEW)
        for k in (2, 4):
            empty = Speculation(num_draft_tokens=k, ngram=False)
            eng.decode(eng.prefill(ids), 8, use_graph=True, speculate=empty)   # warms the verify shapes
            base, empty_ms, _ = step_ms(eng, lambda: eng.prefill(ids), NEW, speculate=empty)
            full = Speculation(num_draft_tokens=k, ngram=False, predicted_ids=base.clone(), check_every=1)
            toks, full_ms, n_full = step_ms(eng, lambda: eng.prefill(ids), NEW, reps=4, speculate=full)
            st = eng.last_speculation
            mean_acc = float(st.accepted.sum()) / max(1, int(st.verify_steps.sum()))
            _, plain_again_ms, _ = step_ms(eng, lambda: eng.prefill(ids), NEW)
            attn = attention_us(eng, model, batch, k, CTX + 64)
            p = 0.5 * (plain_ms + plain_again_ms)
            res["points"].append({
                "batch": batch, "k": k, "plain_ms": round(p, 4), "plain_spread_ms": round(abs(plain_again_ms - plain_ms), 4),
                "verify_empty_ms": round(empty_ms, 4), "verify_full_ms": round(full_ms, 4),
                "steps_full": st.steps_run, "timed_steps_full": n_full, "mean_accepted_full": round(mean_acc, 3),
                "same_tokens": bool(torch.equal(toks, base)),
                "break_even_accepted_per_step": round(full_ms / p - 1, 3),
                "tokens_per_s_plain": round(batch / p * 1e3, 1),
                "tokens_per_s_full_acceptance": round(batch * (1 + mean_acc) / full_ms * 1e3, 1),
                "tokens_per_s_empty_drafts": round(batch / empty_ms * 1e3, 1),
                "attention_us_per_step": round(attn, 1), "attention_share": round(attn / 1e3 / full_ms, 3),
            })
            plain_ms = plain_again_ms
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    main()
