"""DecodeEngine(kv_block_size=, kv_share_blocks=True): a shared prompt prefix and n samples per prompt on the paged pool
(PagedKVPool.fork: full blocks shared by count, the partial last block copied).  Block accounting derived from the
design; bit-equality with the bump-pool shared-prefix engine where the prefix is whole blocks (the same launches, other
row numbers); otherwise the teacher-forced rule and margins of tests/test_shared_prefix_engine_gpu.py against the
unshared bump engine; the shared-prefix decode kernel is reached; captured graph equals eager; no state leaks between
prefills; siblings never write shared rows; the refusals."""

import functools
import types

import pytest
import torch

import lite_llama_amd.kernels.attention as A
from lite_llama_amd.executor import DecodeEngine
from tests.test_shared_prefix_engine_gpu import (DEV, FAMILIES, MAX_SEQ, STEPS, _fixture_model, _prompts, _random_model,
                                                 _teacher_forced)

pytestmark = pytest.mark.gpu
MODELS = ["random"] + FAMILIES
BIT_REPRODUCIBLE = ("random", "llama", "qwen2")     # the models the graph-equals-eager test of that file trusts


@functools.lru_cache(maxsize=None)
def _model(name):
    return _random_model() if name == "random" else _fixture_model(name)


def _prefill(eng, *a, **k):
    """``eng.prefill`` -> (first tokens, the last-token logits ``[rows, vocab]`` it sampled them from, fp32 on the host)."""
    grabbed = []
    orig = eng._first_tokens

    def spy(last, sampling):
        grabbed.append(last.float().cpu())
        return orig(last, sampling)

    eng._first_tokens = spy
    try:
        first = eng.prefill(*a, **k)
    finally:
        del eng._first_tokens
    return first, grabbed[0]


def _ceil(a, b):
    return -(-a // b)


def _in_use(eng):
    return eng.pool.num_blocks - 1 - eng.pool.free_blocks


def _count_kernel_calls(monkeypatch):
    import lite_llama_amd.model as M

    calls = []
    real = M.shared_prefix_decode_attention

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out

    monkeypatch.setattr(M, "shared_prefix_decode_attention", counted)
    return calls


# ------------------------------------------------------------------ shared prefix ----- #
@pytest.mark.parametrize("chunk", [None, 16], ids=["onestep", "chunk16"])
@pytest.mark.parametrize("prefix,batch", [(p, b) for p in (192, 200, 96) for b in (3, 8)])
@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("name", MODELS)
def test_shared_prefix_on_the_paged_pool(name, bs, prefix, batch, chunk, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    m = _model(name)
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, prefix, batch, seed=prefix + batch)
    eng = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=True)
    first, logits = _prefill(eng, tails, tl, chunk_size=chunk, shared_prefix_ids=pre)
    info, pool = eng.info, eng.pool
    # accounting: every row holds the blocks of its own length; the prefix's full blocks exist once
    shared = prefix // bs * bs
    want = [_ceil(int(n), bs) for n in lens.tolist()]
    assert pool.req_blocks.cpu().tolist()[:batch] == want
    assert _in_use(eng) == sum(want) - (batch - 1) * (prefix // bs)
    assert pool.free_blocks == pool.num_blocks - 1 - _in_use(eng) and pool.error == 0
    assert info.shared_prefix_len == shared and info.shared_prefix_req == 0
    table = info.b_req_tokens_table.cpu()
    own = []
    for i in range(batch):
        assert torch.equal(table[i, :shared], table[0, :shared])
        own.append(set(table[i, shared:int(lens[i])].tolist()))
        assert len(own[-1]) == int(lens[i]) - shared
    for i in range(batch):
        for j in range(i):
            assert not own[i] & own[j], (i, j)
        assert not own[i] & set(table[0, :shared].tolist())
    share = pool.block_share.cpu()
    assert int((share > 0).sum()) == prefix // bs and (share[share > 0] == batch - 1).all()
    # the documented post-prefill state
    assert info.b_ctx_len is None and info.max_ctx_len == 0 and info.max_actual_seq_len == prefix + 40
    assert torch.equal(info.b_seq_len.cpu(), lens.cpu()) and info.b_seq_len.dtype == torch.int32
    assert torch.equal(info.b_req_idx.cpu(), torch.arange(batch, dtype=torch.int32))
    assert torch.equal(eng._positions.cpu().view(-1), lens.cpu().long()) and eng._batch == batch
    # last-token logits against the unshared one-step prefill of the concatenated prompts
    ref = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ)
    _, ref_logits = _prefill(ref, full, lens)
    torch.testing.assert_close(logits, ref_logits, rtol=3e-2, atol=3e-2)
    rest = eng.decode(first, STEPS - 1, use_graph=False)
    assert pool.error == 0
    toks = torch.cat([first.view(batch, 1), rest], dim=1)
    if prefix % bs == 0 and name in BIT_REPRODUCIBLE:
        # whole blocks: the launches of the bump-pool shared-prefix engine with other row numbers
        bump = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ)
        b_first, b_logits = _prefill(bump, tails, tl, chunk_size=chunk, shared_prefix_ids=pre)
        assert bump.info.shared_prefix_len == prefix == shared
        assert torch.equal(first, b_first) and torch.equal(logits, b_logits)
        assert torch.equal(rest, bump.decode(b_first, STEPS - 1, use_graph=False))
    _teacher_forced(m, full, lens, toks)


@pytest.mark.parametrize("bs", [16, 64])
def test_shared_prefix_kernel_is_reached_graph_equals_eager_and_no_state_leaks(bs, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    m = _model("random")
    calls = _count_kernel_calls(monkeypatch)
    a = _prompts(m.geo.vocab_size, 200, 3, seed=1)
    b = _prompts(m.geo.vocab_size, 96, 3, seed=2)

    def run(p, use_graph, eng=None):
        eng = eng or DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=True)
        first = eng.prefill(p[1], p[2], shared_prefix_ids=p[0])
        return torch.cat([first.view(3, 1), eng.decode(first, STEPS - 1, use_graph=use_graph)], dim=1), eng

    eager, _ = run(a, False)
    assert len(calls) == (STEPS - 1) * m.geo.num_layers and all(calls)
    graph, eng = run(a, True)
    assert torch.equal(eager, graph) and eng.pool.error == 0
    # the same engine: another prefix, then a plain prefill -- each as a fresh engine gives it
    again, _ = run(b, True, eng=eng)
    fresh, _ = run(b, True)
    assert torch.equal(again, fresh)
    assert eng.info.shared_prefix_len == 96 // bs * bs
    first = eng.prefill(a[3], a[4])
    assert eng.info.shared_prefix_len == 0 and not eng.pool.block_share.any().item()
    plain = torch.cat([first.view(3, 1), eng.decode(first, STEPS - 1, use_graph=True)], dim=1)
    e2 = DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ, kv_block_size=bs)
    f2 = e2.prefill(a[3], a[4])
    assert torch.equal(plain, torch.cat([f2.view(3, 1), e2.decode(f2, STEPS - 1, use_graph=True)], dim=1))


# ------------------------------------------------------------------ n samples per prompt ----- #
def _ragged_prompts(vocab, batch, bs, seed, rot=0):
    """Lengths on and off a block boundary, each at least 64 + bs: 5 * bs + 5, 6 * bs, 6 * bs - 1, rotated by ``rot``."""
    g = torch.Generator().manual_seed(seed)
    lens = [5 * bs + 5, 6 * bs, 6 * bs - 1]
    lens = (lens[rot:] + lens[:rot])[:batch]
    ids = torch.randint(0, vocab, (batch, max(lens)), generator=g)
    for i, n in enumerate(lens):
        ids[i, n:] = 0
    return ids.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("chunk", [None, 24], ids=["onestep", "chunk24"])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("batch,rot", [(1, 0), (1, 1), (3, 0)], ids=["b1_off", "b1_on", "b3"])
@pytest.mark.parametrize("name,bs", [("random", 16), ("random", 32), ("qwen2", 16)])
def test_n_samples_per_prompt(name, bs, batch, rot, n, chunk, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)
    m = _model(name)
    calls = _count_kernel_calls(monkeypatch)
    ids, lens = _ragged_prompts(m.geo.vocab_size, batch, bs, seed=batch * 10 + n, rot=rot)
    rep_ids, rep_lens = ids.repeat_interleave(n, dim=0), lens.repeat_interleave(n)
    lens_l = lens.tolist()
    runs = []
    for use_graph in (False, True):
        eng = DecodeEngine(m, max_batch=batch * n, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=True)
        first = eng.prefill(ids, lens, chunk_size=chunk, num_samples=n)
        info, pool = eng.info, eng.pool
        assert first.shape == (batch * n,) and pool.error == 0
        assert _in_use(eng) == sum(_ceil(v, bs) + (n - 1) * (1 if v % bs else 0) for v in lens_l)
        # the state a one-step prefill of the repeated prompts leaves
        assert torch.equal(info.b_req_idx.cpu(), torch.arange(batch * n, dtype=torch.int32))
        assert torch.equal(info.b_seq_len.cpu(), rep_lens.cpu()) and info.b_seq_len.dtype == torch.int32
        assert torch.equal(info.b_start_loc.cpu(), torch.arange(batch * n, dtype=torch.int32) * ids.shape[1])
        assert torch.equal(eng._positions.cpu().view(-1), rep_lens.cpu().long()) and eng._batch == batch * n
        assert info.max_actual_seq_len == ids.shape[1] and info.b_ctx_len is None
        assert info.shared_prefix_len == (lens_l[0] // bs * bs if batch == 1 and n > 1 else 0)
        table = info.b_req_tokens_table.cpu()
        for i, v in enumerate(lens_l):
            for s in range(1, n):
                full = v // bs * bs
                assert torch.equal(table[i * n + s, :full], table[i * n, :full])
                assert not set(table[i * n + s, full:v].tolist()) & set(table[i * n, :v].tolist())
        # siblings never write shared rows: the shared blocks after the decode are what the prefill left
        shared_blocks = torch.nonzero(pool.block_share > 0).view(-1)
        assert shared_blocks.numel() == (sum(v // bs for v in lens_l) if n > 1 else 0)
        rows = (shared_blocks.view(-1, 1) * bs + torch.arange(bs, device=DEV).view(1, -1)).view(-1)
        before = [kv[rows].clone() for kv in pool.kv_buffer]
        share_before = pool.block_share.clone()
        calls.clear()
        rest = eng.decode(first, STEPS - 1, use_graph=use_graph)
        assert pool.error == 0 and torch.equal(pool.block_share, share_before)
        for kv, was in zip(pool.kv_buffer, before):
            assert torch.equal(kv[rows].view(torch.uint8), was.view(torch.uint8))
        if batch == 1 and n > 1:                                # a prompt of >= 64 + bs tokens: the route is taken,
            if name == "random":                                # and on the head-size-128 model the kernel is reached
                assert lens_l[0] >= 64 + bs and all(calls)
                # eager: one call per layer and step; captured: the warm-up step and the capture (replays run no Python)
                assert len(calls) == (2 if use_graph else STEPS - 1) * m.geo.num_layers
        else:
            assert not calls                                    # several prompts, or nothing shared: the ordinary route
        toks = torch.cat([first.view(-1, 1), rest], dim=1)
        runs.append(toks)
        _teacher_forced(m, rep_ids, rep_lens, toks)
        if n == 1:
            e1 = DecodeEngine(m, max_batch=batch, max_seq_len=MAX_SEQ, kv_block_size=bs, kv_share_blocks=True)
            f1 = e1.prefill(ids, lens, chunk_size=chunk)
            assert torch.equal(toks, torch.cat([f1.view(-1, 1), e1.decode(f1, STEPS - 1, use_graph=use_graph)], dim=1))
    if name in BIT_REPRODUCIBLE:
        assert torch.equal(runs[0], runs[1])                    # captured equals eager


def test_samples_of_one_prompt_differ_under_sampling(monkeypatch):
    """Temperature 1, top-p 1: the uniforms are per row, so 8 samples of one prompt over 8 steps are not all one row.  The
    seed is fixed: the run is deterministic."""
    m = _model("random")
    ids, lens = _ragged_prompts(m.geo.vocab_size, 1, 16, seed=5)
    sp = types.SimpleNamespace(temperature=1.0, top_p=1.0, repetition_penalty=1.0)
    torch.manual_seed(1234)
    eng = DecodeEngine(m, max_batch=8, max_seq_len=MAX_SEQ, kv_block_size=16, kv_share_blocks=True)
    first = eng.prefill(ids, lens, sampling=sp, num_samples=8)
    rest = eng.decode(first, STEPS - 1, use_graph=True, sampling=sp)
    toks = torch.cat([first.view(8, 1), rest], dim=1).cpu()
    assert eng.pool.error == 0 and toks.shape == (8, STEPS)
    assert len({tuple(r.tolist()) for r in toks}) > 1, toks
    # every sample still holds the prompt's full blocks by count, and its own blocks after them
    # decode names the row of the NEXT token after every forward (as tests/test_paged_kv_gpu.py counts: prompt + generated
    # + 1), so after the prefill and STEPS - 1 steps every sample has blocks for n0 + STEPS positions
    n0 = lens.tolist()[0]
    assert torch.equal(eng.info.b_seq_len.cpu(), torch.full((8,), n0 + STEPS, dtype=torch.int32))
    assert _in_use(eng) == n0 // 16 + 8 * _ceil(n0 + STEPS - n0 // 16 * 16, 16)


# ------------------------------------------------------------------ refusals ----- #
def test_refusals():
    m = _model("random")
    pre, tails, tl, full, lens = _prompts(m.geo.vocab_size, 96, 3, seed=4)
    with pytest.raises(ValueError, match="kv_share_blocks needs kv_block_size"):
        DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ, kv_share_blocks=True)
    plain = DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ, kv_block_size=16)
    with pytest.raises(ValueError, match="bump pool"):
        plain.prefill(tails, tl, shared_prefix_ids=pre)
    with pytest.raises(ValueError, match="num_samples needs kv_share_blocks"):
        plain.prefill(full, lens, num_samples=1)
    with pytest.raises(ValueError, match="num_samples needs kv_share_blocks"):
        DecodeEngine(m, max_batch=3, max_seq_len=MAX_SEQ).prefill(full, lens, num_samples=1)
    eng = DecodeEngine(m, max_batch=8, max_seq_len=MAX_SEQ, kv_block_size=16, kv_share_blocks=True)
    with pytest.raises(ValueError, match="max_batch"):
        eng.prefill(full, lens, num_samples=3)                  # 9 rows > 8
    with pytest.raises(ValueError, match="cannot be combined with shared_prefix_ids"):
        eng.prefill(tails, tl, shared_prefix_ids=pre, num_samples=2)
    with pytest.raises(ValueError, match="at least one token"):
        eng.prefill(tails[:, :0], None, shared_prefix_ids=pre)
    # the engine is usable after the refusals, and a pool error names bit 4
    first = eng.prefill(full, lens, num_samples=2)
    assert first.shape == (6,) and eng.pool.error == 0
    eng.pool.state[1] = 4
    with pytest.raises(RuntimeError, match="4: a fork"):
        eng._check_device_errors()
    eng.pool.state[1] = 0
