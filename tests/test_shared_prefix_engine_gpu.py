"""DecodeEngine.prefill(shared_prefix_ids=...): one prompt prefix cached once for the whole batch, the tails prefilled as
chunk steps on top of it, decode on the shared-prefix attention route.  The comparator is always an unshared DecodeEngine
fed the concatenated prompts: pool accounting, last-token logits, teacher-forced greedy tokens (the rule and margin of
tests/test_chunked_prefill_gpu.py), graph against eager, state leaks between prefills, chunk_size and the refusals."""

import numpy as np
import pytest
import torch

import lite_llama_amd.kernels.attention as A
from lite_llama_amd.executor import DecodeEngine
from lite_llama_amd.model import CausalLM, tiny_geometry
from tests import _golden as G
from tests.test_model_step import _hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = ["llama", "qwen2", "qwen3", "qwen3_moe"]
MAX_SEQ = 320
STEPS = 8


def _fixture_model(family):
    d = np.load(G.GOLDEN_DIR + f"/model_step_{family}_tiny.npz")
    params = {k[len("param."):]: torch.from_numpy(d[k].copy()) for k in d.files if k.startswith("param.")}
    return _hip_model(params, None, family)


def _random_model(seed=3, **kw):
    geo = tiny_geometry(head_dim=128, num_heads=4, num_kv_heads=2, hidden_size=512, intermediate_size=1024, **kw)
    return CausalLM(geo).init_synthetic(seed=seed, device=DEV)


def _prompts(vocab, prefix, batch, seed):
    """Seeded prompts that share their first ``prefix`` tokens; ragged tails of 1 .. 40 tokens (one of each extreme)."""
    g = torch.Generator().manual_seed(seed)
    pre = torch.randint(0, vocab, (prefix,), generator=g)
    tl = torch.randint(1, 41, (batch,), generator=g)
    tl[0], tl[-1] = 40, 1
    tails = torch.randint(0, vocab, (batch, 40), generator=g)
    full = torch.zeros(batch, prefix + 40, dtype=torch.int64)
    for i in range(batch):
        full[i, :prefix] = pre
        full[i, prefix:prefix + int(tl[i])] = tails[i, :int(tl[i])]
    return pre.to(DEV), tails.to(DEV), tl.int().to(DEV), full.to(DEV), (tl + prefix).int().to(DEV)


def _spy_last_logits(model, fn):
    """Run ``fn`` and return the last ``logits_rows`` output(s) of the model's forward, as fp32 CPU rows."""
    grabbed = []
    orig = model.forward

    def spy(*a, **k):
        out = orig(*a, **k)
        if k.get("logits_rows") is not None:
            grabbed.append(out.view(-1, out.shape[-1]).float().cpu())
        return out

    model.forward = spy
    try:
        res = fn()
    finally:
        model.forward = orig
    return res, grabbed


def _teacher_forced(model, full, lens, toks):
    """Every row and every step: the unshared engine's one-step prefill of prompt + toks[:, :k] ranks toks[:, k] first, or
    within 2e-2 of the top logit."""
    b = full.shape[0]
    for k in range(toks.shape[1]):
        ids = torch.zeros(b, full.shape[1] + k, dtype=torch.int64, device=DEV)
        for i in range(b):
            n = int(lens[i])
            ids[i, :n] = full[i, :n]
            ids[i, n:n + k] = toks[i, :k]
        eng = DecodeEngine(model, max_batch=b, max_seq_len=MAX_SEQ)
        _, grabbed = _spy_last_logits(model, lambda: eng.prefill(ids, (lens + k).int()))
        lg = grabbed[-1]
        mine = toks[:, k].cpu()
        top = lg.max(-1).values
        chosen = lg.gather(1, mine.view(b, 1)).squeeze(1)
        assert torch.all(top - chosen <= 2e-2), (k, top - chosen)


def _shared_run(model, pre, tails, tl, steps=STEPS, use_graph=False, chunk=None, eng=None):
    b = tails.shape[0]
    eng = eng or DecodeEngine(model, max_batch=b, max_seq_len=MAX_SEQ)
    first = eng.prefill(tails, tl, chunk_size=chunk, shared_prefix_ids=pre)
    rest = eng.decode(first, steps - 1, use_graph=use_graph)
    return torch.cat([first.view(b, 1), rest], dim=1), eng


def _models():
    return [("random", _random_model)] + [(f, lambda f=f: _fixture_model(f)) for f in FAMILIES]


@pytest.mark.parametrize("name,make", _models(), ids=[m[0] for m in _models()])
@pytest.mark.parametrize("prefix,batch", [(96, 3), (200, 8)])
def test_shared_prefill_state_logits_and_tokens(name, make, prefix, batch, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)      # the tiny models exercise the new kernel
    m = make()
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, prefix, batch, seed=prefix + batch)
    eng = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ)
    first, grabbed = _spy_last_logits(m, lambda: eng.prefill(tails, tl, shared_prefix_ids=pre))
    info = eng.info
    # pool and table: the prefix once, then one tail grid
    assert eng.pool.used == prefix + batch * 40
    table = info.b_req_tokens_table.cpu()
    for i in range(batch):
        assert torch.equal(table[i, :prefix], table[0, :prefix])
    assert len(set(table[0, :prefix].tolist())) == prefix
    # the documented post-prefill state
    assert info.shared_prefix_len == prefix and info.shared_prefix_req == 0
    assert info.b_ctx_len is None and info.max_ctx_len == 0 and info.max_actual_seq_len == prefix + 40
    assert torch.equal(info.b_seq_len.cpu(), lens.cpu()) and info.b_seq_len.dtype == torch.int32
    assert torch.equal(info.b_req_idx.cpu(), torch.arange(batch, dtype=torch.int32))
    assert torch.equal(eng._positions.cpu().view(-1), lens.cpu().long()) and eng._batch == batch
    # last-token logits against the unshared one-step prefill
    ref = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ)
    ref_first, ref_grabbed = _spy_last_logits(m, lambda: ref.prefill(full, lens))
    assert ref.pool.used == batch * (prefix + 40) and ref.info.shared_prefix_len == 0
    torch.testing.assert_close(grabbed[-1], ref_grabbed[-1], rtol=3e-2, atol=3e-2)
    # greedy decode on the shared route, teacher-forced against the unshared engine
    rest = eng.decode(first, STEPS - 1, use_graph=False)
    toks = torch.cat([first.view(batch, 1), rest], dim=1)
    _teacher_forced(m, full, lens, toks)


def test_new_kernel_is_reached_and_old_route_reads_the_aliased_table(monkeypatch):
    m = _random_model()
    prefix, batch = 200, 8
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, prefix, batch, seed=9)
    calls = []
    import lite_llama_amd.model as M

    real = M.shared_prefix_decode_attention

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(M, "shared_prefix_decode_attention", counted)
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    toks_new, _ = _shared_run(m, pre, tails, tl)
    assert len(calls) == (STEPS - 1) * m.geo.num_layers and all(calls)
    # threshold above the prefix: rows and prefill stay shared, the decode launch stays on the old route
    calls.clear()
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", prefix + 1)
    toks_old, eng = _shared_run(m, pre, tails, tl)
    assert not calls and eng.info.shared_prefix_len == prefix
    _teacher_forced(m, full, lens, toks_old)
    _teacher_forced(m, full, lens, toks_new)


@pytest.mark.parametrize("name,make", _models()[:3], ids=[m[0] for m in _models()[:3]])
def test_graph_equals_eager_and_no_state_leaks(name, make, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    m = make()
    vocab = m.geo.vocab_size
    a = _prompts(vocab, 200, 3, seed=1)
    b = _prompts(vocab, 96, 3, seed=2)
    eager, _ = _shared_run(m, a[0], a[1], a[2], use_graph=False)
    graph, eng = _shared_run(m, a[0], a[1], a[2], use_graph=True)
    assert torch.equal(eager, graph)
    # the same engine: another prefix length, then no prefix at all -- each as a fresh engine gives it
    again, _ = _shared_run(m, b[0], b[1], b[2], use_graph=True, eng=eng)
    fresh, _ = _shared_run(m, b[0], b[1], b[2], use_graph=True)
    assert torch.equal(again, fresh)
    first = eng.prefill(a[3], a[4])
    assert eng.info.shared_prefix_len == 0
    plain = torch.cat([first.view(3, 1), eng.decode(first, STEPS - 1, use_graph=True)], dim=1)
    e2 = DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ)
    f2 = e2.prefill(a[3], a[4])
    assert torch.equal(plain, torch.cat([f2.view(3, 1), e2.decode(f2, STEPS - 1, use_graph=True)], dim=1))


def test_chunk_size_with_shared_prefix_gives_the_same_first_tokens(monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    m = _random_model(seed=5)
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, 96, 8, seed=3)
    firsts = {}
    for chunk in (None, 16, 7):
        eng = DecodeEngine(m, max_batch=8, max_seq_len=MAX_SEQ)
        firsts[chunk] = eng.prefill(tails, tl, chunk_size=chunk, shared_prefix_ids=pre).cpu()
        assert eng.pool.used == 96 + 8 * 40 and eng.info.shared_prefix_len == 96
        assert torch.equal(eng.info.b_seq_len.cpu(), lens.cpu())
    assert torch.equal(firsts[16], firsts[None]) and torch.equal(firsts[7], firsts[None])


def test_refusals():
    m = _random_model()
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, 96, 3, seed=4)
    with pytest.raises(ValueError, match="bump pool"):
        DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ, kv_block_size=16).prefill(tails, tl, shared_prefix_ids=pre)
    eng = DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ)
    bad = tl.clone()
    bad[1] = 0
    with pytest.raises(ValueError, match="at least one token"):
        eng.prefill(tails, bad, shared_prefix_ids=pre)
    with pytest.raises(ValueError, match="at least one token"):
        eng.prefill(tails[:, :0], None, shared_prefix_ids=pre)
