"""Chunked prefill through the model: DecodeEngine.prefill(chunk_size=...) on the golden model-step fixtures (first
tokens, prompt K/V in the pool, then greedy decode eager / graph against the oracle), a long prompt against the one-step
prefill with both allocators, the e4m3 pool, and a SlotBatch slot continued by a second begin_prefill."""

import numpy as np
import pytest
import torch

from lite_llama_amd.executor import DecodeEngine, SlotRunner
from lite_llama_amd.model import CausalLM, tiny_geometry
from tests import _golden as G
from tests.test_model_step import _hip_model, _info, _oracle_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = ["llama", "qwen2", "qwen3", "qwen3_moe"]


def _load(family):
    d = np.load(G.GOLDEN_DIR + f"/model_step_{family}_tiny.npz")
    params = {k[len("param."):]: torch.from_numpy(d[k].copy()) for k in d.files if k.startswith("param.")}
    return d, params


def _oracle_ranks_engine_tokens(d, params, family, toks):
    """Teacher-forced oracle decode over the fixture prompt: at every step the engine's token is the oracle's argmax
    or within 2e-2 of it (test_model_step.test_engine_graph_equals_eager_and_oracle's margin)."""
    H, I, L, HQ, HKV, D, V = [int(x) for x in d["geometry"]]
    om = _oracle_model(params, None, family)
    lens_l = d["lens"].tolist()
    B, LP = len(lens_l), max(lens_l)
    kv = [torch.zeros(128, 2 * HKV, D, dtype=torch.float16) for _ in range(L)]
    table = torch.zeros(B, 64, dtype=torch.int32)
    sel = torch.arange(B * LP, dtype=torch.int32)
    for i, n in enumerate(lens_l):
        table[i, :n] = sel[i * LP: i * LP + n]
    info = _info(kv, table, sel, torch.tensor(lens_l, dtype=torch.int32), torch.arange(B, dtype=torch.int32) * LP, LP)
    pos = torch.arange(LP).unsqueeze(0).expand(B, LP).contiguous()
    logits = om.forward(torch.from_numpy(d["prompt_ids"]), pos, info)
    tok = torch.stack([logits[i, n - 1] for i, n in enumerate(lens_l)]).float().argmax(-1)
    seq = torch.tensor(lens_l, dtype=torch.int32)
    next_row = B * LP
    for step in range(toks.shape[1]):
        info.cur_select_index = torch.arange(next_row, next_row + B, dtype=torch.int32)
        next_row += B
        seq = seq + 1
        info.b_seq_len = seq
        info.max_actual_seq_len = int(seq.max())
        for i in range(B):
            table[i, int(seq[i]) - 1] = info.cur_select_index[i]
        lg = om.forward(tok.view(B, 1), (seq - 1).view(B, 1).long(), info)[:, -1].float()
        mine = toks[:, step]
        top = lg.max(-1).values
        chosen = lg.gather(1, mine.view(B, 1)).squeeze(1)
        assert torch.all(top - chosen <= 2e-2), (family, step, top - chosen)
        tok = mine


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kv_block_size", [None, 4])
def test_chunked_prefill_follows_the_golden_step(family, kv_block_size):
    d, params = _load(family)
    m = _hip_model(params, None, family)
    ids = torch.from_numpy(d["prompt_ids"]).to(DEV)
    lens = torch.from_numpy(d["lens"]).int().to(DEV)
    lens_l = d["lens"].tolist()
    LP = max(lens_l)
    for chunk in (1, 2, 3):
        outs = []
        for use_graph in (False, True):
            eng = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
            first = eng.prefill(ids, lens, chunk_size=chunk)
            assert torch.equal(first.cpu(), torch.from_numpy(d["first_tokens"])), (family, chunk)
            assert eng.info.b_ctx_len is None and eng.info.max_actual_seq_len == LP
            assert torch.equal(eng.info.b_seq_len.cpu(), lens.cpu())
            if not use_graph:
                table = eng.info.b_req_tokens_table.cpu()
                for li, kv in enumerate(eng.pool.kv_buffer):
                    rows = [int(table[i, j]) for i, n in enumerate(lens_l) for j in range(n)]
                    want = torch.from_numpy(d[f"kv_prefill.{li}"])[[i * LP + j for i, n in enumerate(lens_l)
                                                                   for j in range(n)]]
                    torch.testing.assert_close(kv[rows].float().cpu(), want.float(), rtol=2e-2, atol=2e-2)
            outs.append(eng.decode(first, 12, use_graph=use_graph).cpu())
        assert torch.equal(outs[0], outs[1]), (family, chunk)
        _oracle_ranks_engine_tokens(d, params, family, outs[0])


def _random_model(seed=3, **kw):
    geo = tiny_geometry(head_dim=128, num_heads=4, num_kv_heads=2, hidden_size=512, intermediate_size=1024, **kw)
    return CausalLM(geo).init_synthetic(seed=seed, device=DEV)


@pytest.mark.parametrize("kv_block_size", [None, 16])
def test_long_prompt_in_chunks_matches_one_step(kv_block_size):
    m = _random_model()
    gen = torch.Generator().manual_seed(4)
    lens = torch.tensor([700, 431], dtype=torch.int32)
    ids = torch.randint(0, m.geo.vocab_size, (2, 700), generator=gen).to(DEV)
    grabbed = []
    orig = m.forward

    def spy(*a, **k):
        out = orig(*a, **k)
        if k.get("logits_rows") is not None:
            grabbed.append(out.view(-1, out.shape[-1]).float().cpu())
        return out

    last = {}
    toks = {}
    for chunk in (None, 256):
        eng = DecodeEngine(m, max_batch=2, max_seq_len=1024, kv_block_size=kv_block_size)
        grabbed.clear()
        m.forward = spy
        try:
            first = eng.prefill(ids, lens.to(DEV), chunk_size=chunk)
        finally:
            m.forward = orig
        if chunk is None:
            last[chunk] = grabbed[0]
        else:  # chunk 2 ends sequence 1 (431 = 256 + 175), chunk 3 sequence 0
            last[chunk] = torch.stack([grabbed[2][0], grabbed[1][0]])
        toks[chunk] = (first.cpu(), eng.decode(first, 8, use_graph=True).cpu())
    torch.testing.assert_close(last[256], last[None], rtol=3e-2, atol=3e-2)
    assert torch.equal(toks[256][0], toks[None][0])


def test_fp8_pool_chunked_prefill():
    m = _random_model(seed=5)
    gen = torch.Generator().manual_seed(6)
    lens = torch.tensor([90, 37, 64], dtype=torch.int32, device=DEV)
    ids = torch.randint(0, m.geo.vocab_size, (3, 90), generator=gen).to(DEV)
    grabbed = []
    orig = m.forward

    def spy(*a, **k):
        out = orig(*a, **k)
        if k.get("logits_rows") is not None:
            grabbed.append(out.view(-1, out.shape[-1]).float().cpu())
        return out

    def last_logits(kv_dtype, chunk):
        eng = DecodeEngine(m, max_batch=3, max_seq_len=128, kv_dtype=kv_dtype)
        grabbed.clear()
        m.forward = spy
        try:
            first = eng.prefill(ids, lens, chunk_size=chunk)
        finally:
            m.forward = orig
        out = torch.empty(3, grabbed[0].shape[-1])
        if chunk is None:
            out[:] = grabbed[0]
        else:  # chunk 32: sequence 1 ends in chunk 1 (37), 2 in chunk 1 (64), 0 in chunk 2 (90)
            out[1], out[2], out[0] = grabbed[1][0], grabbed[1][1], grabbed[2][0]
        eager = eng.decode(first, 6, use_graph=False).cpu()
        return out, first.cpu(), eager, eng

    ref, ref_first, _, _ = last_logits(torch.float16, None)
    got, got_first, eager, eng = last_logits(torch.float8_e4m3fn, 32)
    # e4m3 keeps 3 mantissa bits of every cached K / V value the later chunks read: the logits move, by little
    err = (got - ref).abs().max().item()
    assert err <= 0.06 * ref.abs().max().item() + 0.02, err
    # and decode after a chunked fp8 prefill: captured == eager
    eng2 = DecodeEngine(m, max_batch=3, max_seq_len=128, kv_dtype=torch.float8_e4m3fn)
    first2 = eng2.prefill(ids, lens, chunk_size=32)
    assert torch.equal(first2.cpu(), got_first)
    assert torch.equal(eng2.decode(first2, 6, use_graph=True).cpu(), eager)


def test_slot_continuation_equals_one_prefill():
    m = _random_model(seed=7)
    gen = torch.Generator().manual_seed(8)
    ids = torch.randint(0, m.geo.vocab_size, (2, 150), generator=gen).to(DEV)
    lens, first_part = [150, 97], [61, 40]

    def runner():
        r = SlotRunner(m, max_request_num=4, max_seq_len=256)
        sb = r.enable_slot_kv_cache()
        for kv in r.pool.kv_buffer:
            kv.copy_(torch.randn(kv.shape, generator=gen).to(kv.dtype).to(DEV))
        return r, sb

    # one begin_prefill for both prompts
    r1, sb1 = runner()
    sb1.begin_prefill([0, 1], lens)
    pos = torch.arange(150, device=DEV).unsqueeze(0).expand(2, 150)
    full = r1.forward(ids, pos)
    one = torch.stack([full[0, 149], full[1, 96]]).float()
    # the same prompts admitted in two pieces: a ragged first piece, then continuations from cached_lens
    r2, sb2 = runner()
    before = [kv.clone() for kv in r2.pool.kv_buffer]
    w1 = max(first_part)
    sb2.begin_prefill([0, 1], first_part)
    ids1 = torch.stack([ids[0, :w1], ids[1, :w1]])
    r2.forward(ids1, torch.arange(w1, device=DEV).unsqueeze(0).expand(2, w1))
    rest = [lens[i] - first_part[i] for i in range(2)]
    w2 = max(rest)
    ids2 = torch.zeros(2, w2, dtype=ids.dtype, device=DEV)
    pos2 = torch.zeros(2, w2, dtype=torch.long, device=DEV)
    for i in range(2):
        ids2[i, :rest[i]] = ids[i, first_part[i]:lens[i]]
        pos2[i] = first_part[i] + torch.arange(w2, device=DEV).clamp(max=rest[i] - 1)
    sb2.begin_prefill([0, 1], rest, cached_lens=first_part)
    out2 = r2.forward(ids2, pos2)
    two = torch.stack([out2[0, rest[0] - 1], out2[1, rest[1] - 1]]).float()
    torch.testing.assert_close(two.cpu(), one.cpu(), rtol=3e-2, atol=3e-2)
    # rows past each sequence inside its slot, and the untouched slot 2, are bit-unchanged (pads went to the filler)
    L = r2.max_seq_len
    for kv, kb in zip(r2.pool.kv_buffer, before):
        for s, n in ((0, lens[0]), (1, lens[1])):
            assert torch.equal(kv[s * L + n:(s + 1) * L], kb[s * L + n:(s + 1) * L])
        assert torch.equal(kv[2 * L:3 * L], kb[2 * L:3 * L])
    # a one-token continuation reaches the model with seq_len == 1: it takes the paged prefill, not a decode route
    sb2.begin_prefill([0], [1], cached_lens=[lens[0]])
    nxt = torch.argmax(out2[0, rest[0] - 1]).view(1, 1)
    step = r2.forward(nxt, torch.tensor([[lens[0]]], device=DEV)).float()
    r3, sb3 = runner()
    sb3.begin_prefill([0], [lens[0] + 1])
    ids3 = torch.cat([ids[0:1], nxt], dim=1)
    ref3 = r3.forward(ids3, torch.arange(lens[0] + 1, device=DEV).unsqueeze(0)).float()
    torch.testing.assert_close(step[0, 0].cpu(), ref3[0, -1].cpu(), rtol=3e-2, atol=3e-2)
    # and a decode step afterwards still reads b_seq_len as the length including its token
    sb2.begin_decode([0], [lens[0] + 2])
    assert sb2._atten.b_ctx_len is None
