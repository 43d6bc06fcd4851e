"""Log-probabilities from the engine: DecodeEngine.decode / prefill (logprobs=k) and DecodeEngine.score on the golden
model-step fixtures (llama / qwen2 / qwen3 / qwen3_moe), bump and paged pool, eager and captured.

Tolerances.  Against the oracle (teacher-forced on the engine's tokens exactly as
tests/test_chunked_prefill_gpu.py::_oracle_ranks_engine_tokens does): 6e-2, twice the 3e-2 logits tolerance this project uses
between routes -- the log-sum-exp moves by at most the largest logit error, the token's own logit by as much again.  Between
two runs of the same kernels on the same logits: the kernel tolerance of tests/_logprobs_ref.py."""

import types

import pytest
import torch

from lite_llama_amd.executor import DecodeEngine
from tests import _logprobs_ref as R
from tests.test_chunked_prefill_gpu import FAMILIES, _load, _random_model
from tests.test_model_step import _hip_model, _info, _oracle_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 12
ORACLE_TOL = 6e-2


def _fixture(family):
    d, params = _load(family)
    ids = torch.from_numpy(d["prompt_ids"]).to(DEV)
    lens = torch.from_numpy(d["lens"]).int().to(DEV)
    return d, params, _hip_model(params, None, family), ids, lens


def _oracle_logits(d, params, family, first, toks):
    """The oracle's fp64 log-softmax teacher-forced on the engine's tokens: ``(prefill [B, LP, V], first-token [B, V],
    per decode step [B, steps, V])``."""
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
    prefill = torch.log_softmax(logits.double(), -1)
    last = torch.stack([prefill[i, n - 1] for i, n in enumerate(lens_l)])
    steps = []
    if toks is not None:
        tok = first.cpu()
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
            lg = om.forward(tok.view(B, 1), (seq - 1).view(B, 1).long(), info)[:, -1]
            steps.append(torch.log_softmax(lg.double(), -1))
            tok = toks[:, step].cpu()
    return prefill, last, (torch.stack(steps, 1) if steps else None)


def _greedy_identities(lp, tokens, k):
    """Under greedy decoding: chosen == top_logprobs[..., 0] and top_ids[..., 0] == token, exactly; top_logprobs
    non-increasing along k."""
    rows, t = tokens.shape
    assert lp.chosen.shape == (rows, t) and lp.top_logprobs.shape == (rows, t, k) and lp.top_ids.shape == (rows, t, k)
    assert torch.equal(lp.chosen, lp.top_logprobs[..., 0])
    assert torch.equal(lp.top_ids[..., 0], tokens)
    assert torch.all(lp.top_logprobs[..., 1:] <= lp.top_logprobs[..., :-1])
    assert torch.all(torch.isfinite(lp.top_logprobs)) and torch.all(lp.chosen <= 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kv_block_size", [None, 4])
def test_decode_and_prefill_logprobs(family, kv_block_size):
    d, params, m, ids, lens = _fixture(family)
    got = {}
    for use_graph in (False, True):
        plain = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
        first0 = plain.prefill(ids, lens)
        toks0 = plain.decode(first0, STEPS, use_graph=use_graph)
        assert plain.first_logprobs is None and plain.last_logprobs is None
        eng = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
        first = eng.prefill(ids, lens, logprobs=5)
        toks = eng.decode(first, STEPS, use_graph=use_graph, logprobs=5)
        # nothing else moved
        assert torch.equal(first, first0) and torch.equal(toks, toks0), (family, use_graph)
        _greedy_identities(eng.first_logprobs, first.view(-1, 1), 5)
        _greedy_identities(eng.last_logprobs, toks, 5)
        got[use_graph] = (first.cpu(), toks.cpu(), eng.first_logprobs.chosen.cpu(), eng.last_logprobs.chosen.cpu())
        # k = 20 of the fixtures' 512 tokens: the probabilities of distinct tokens add up to at most 1
        wide = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=kv_block_size)
        f20 = wide.prefill(ids, lens, logprobs=20)
        t20 = wide.decode(f20, STEPS, use_graph=use_graph, logprobs=20)
        assert torch.equal(t20, toks0)
        _greedy_identities(wide.last_logprobs, t20, 20)
        for lp in (wide.first_logprobs, wide.last_logprobs):
            assert torch.all(torch.exp(lp.top_logprobs.double()).sum(-1) <= 1 + 1e-4)
            ids_sorted = lp.top_ids.sort(-1).values
            assert torch.all(ids_sorted[..., 1:] != ids_sorted[..., :-1])
        # a decode without logprobs after one with: nothing is left behind
        again = eng.decode(eng.prefill(ids, lens), 3, use_graph=use_graph)
        assert eng.last_logprobs is None and eng.first_logprobs is None and torch.equal(again, toks0[:, :3])
    assert torch.equal(got[False][0], got[True][0]) and torch.equal(got[False][1], got[True][1])  # graph == eager, as today
    first, toks, first_lp, last_lp = got[True]
    _, o_first, o_steps = _oracle_logits(d, params, family, first, toks)
    for which, g in got.items():
        err_first = (g[2][:, 0].double() - o_first.gather(1, first.view(-1, 1)).squeeze(1)).abs().max().item()
        err_steps = (g[3].double() - o_steps.gather(2, toks.unsqueeze(-1)).squeeze(-1)).abs().max().item()
        print(f"{family} bs={kv_block_size} graph={which}: |chosen - oracle| first {err_first:.3e}, steps {err_steps:.3e}")
        assert err_first <= ORACLE_TOL and err_steps <= ORACLE_TOL, (family, which, err_first, err_steps)


@pytest.mark.parametrize("family", FAMILIES)
def test_steps_per_graph_gives_the_same_logprobs(family):
    d, params, m, ids, lens = _fixture(family)
    out = {}
    for group in (1, 4):
        eng = DecodeEngine(m, max_batch=2, max_seq_len=64)
        first = eng.prefill(ids, lens)
        toks = eng.decode(first, 10, use_graph=True, steps_per_graph=group, logprobs=5)  # 4 + 4, then two single steps
        out[group] = (toks.cpu(), eng.last_logprobs)
    assert torch.equal(out[1][0], out[4][0])
    a, b = out[1][1], out[4][1]
    assert torch.equal(a.top_ids, b.top_ids)
    print(f"{family}: steps_per_graph 4 vs 1 bit-equal: chosen {torch.equal(a.chosen, b.chosen)}, "
          f"top {torch.equal(a.top_logprobs, b.top_logprobs)}")
    R.assert_close_logprobs(b.chosen, a.chosen.cpu().double(), "steps_per_graph chosen")
    R.assert_close_logprobs(b.top_logprobs, a.top_logprobs.cpu().double(), "steps_per_graph top")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_logprobs_under_sampling_describe_the_raw_distribution(family, use_graph):
    d, params, m, ids, lens = _fixture(family)
    sp = types.SimpleNamespace(temperature=0.8, top_p=0.9, repetition_penalty=1.1)
    k = 5
    eng = DecodeEngine(m, max_batch=2, max_seq_len=64)
    torch.manual_seed(3)
    first = eng.prefill(ids, lens, sampling=sp, logprobs=k)
    toks = eng.decode(first, STEPS, use_graph=use_graph, sampling=sp, logprobs=k)
    for lp, tk in ((eng.first_logprobs, first.view(-1, 1)), (eng.last_logprobs, toks)):
        assert lp.chosen.shape == tk.shape
        assert torch.all(torch.isfinite(lp.chosen))
        assert torch.all(lp.chosen <= lp.top_logprobs[..., 0])
        hit = lp.top_ids == tk.unsqueeze(-1)                       # the sampled token among the k
        assert torch.all(hit.sum(-1) <= 1)
        where = hit.any(-1)
        assert torch.equal(lp.chosen[where], lp.top_logprobs[hit])
        assert torch.all(lp.top_logprobs[..., 1:] <= lp.top_logprobs[..., :-1])
    # the same seed without logprobs draws the same tokens
    eng2 = DecodeEngine(m, max_batch=2, max_seq_len=64)
    torch.manual_seed(3)
    first2 = eng2.prefill(ids, lens, sampling=sp)
    toks2 = eng2.decode(first2, STEPS, use_graph=use_graph, sampling=sp)
    assert torch.equal(first2, first) and torch.equal(toks2, toks)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("chunk", [None, 2])
def test_n_samples_share_their_prompts_distribution(family, chunk):
    d, params, m, ids, lens = _fixture(family)
    b, n, k = ids.shape[0], 4, 3
    sp = types.SimpleNamespace(temperature=1.0, top_p=1.0, repetition_penalty=1.0)
    eng = DecodeEngine(m, max_batch=b * n, max_seq_len=64, kv_block_size=4, kv_share_blocks=True)
    first = eng.prefill(ids, lens, sampling=sp, chunk_size=chunk, num_samples=n, logprobs=k)
    lp = eng.first_logprobs
    assert first.shape == (b * n,) and lp.chosen.shape == (b * n, 1) and lp.top_ids.shape == (b * n, 1, k)
    for i in range(b):
        for s in range(1, n):
            assert torch.equal(lp.top_ids[i * n + s], lp.top_ids[i * n])
            assert torch.equal(lp.top_logprobs[i * n + s], lp.top_logprobs[i * n])
    # every row scores its own token in that distribution
    _, o_first, _ = _oracle_logits(d, params, family, None, None)
    want = o_first.repeat_interleave(n, 0).gather(1, first.cpu().view(-1, 1)).squeeze(1)
    assert (lp.chosen[:, 0].cpu().double() - want).abs().max().item() <= ORACLE_TOL
    toks = eng.decode(first, 6, use_graph=True, sampling=sp, logprobs=k)
    assert eng.last_logprobs.chosen.shape == (b * n, 6) and torch.all(torch.isfinite(eng.last_logprobs.chosen))
    ranked = eng.last_logprobs.cumulative() + lp.cumulative()      # best-of-n: one number per sample
    assert ranked.shape == (b * n,) and torch.all(ranked < 0)


@pytest.mark.parametrize("family", FAMILIES)
def test_score_follows_the_oracle_prefill(family):
    d, params, m, ids, lens = _fixture(family)
    lens_l = d["lens"].tolist()
    b, l = ids.shape
    prefill, _, _ = _oracle_logits(d, params, family, None, None)
    want = prefill[:, :-1].gather(2, ids.cpu()[:, 1:].unsqueeze(-1)).squeeze(-1)          # [B, L - 1]
    valid = torch.arange(1, l).unsqueeze(0) < torch.tensor(lens_l).view(b, 1)
    assert valid.sum() < valid.numel(), "the fixture pads a prompt: the padding rule is exercised"
    got = {}
    for bs in (None, 4):
        for chunk in (None, 2):
            eng = DecodeEngine(m, max_batch=2, max_seq_len=64, kv_block_size=bs)
            lp = eng.score(ids, lens, chunk_size=chunk, top_k=4)
            assert lp.chosen.shape == (b, l - 1) and lp.top_ids.shape == (b, l - 1, 4)
            c = lp.chosen.cpu()
            err = (c.double() - want)[valid].abs().max().item()
            print(f"{family} bs={bs} chunk={chunk}: |score - oracle| {err:.3e}")
            assert err <= ORACLE_TOL, (family, bs, chunk, err)
            assert torch.all(c[~valid] == 0.0) and torch.all(lp.top_ids.cpu()[~valid] == -1)
            assert torch.all(lp.top_logprobs.cpu()[~valid] == 0.0)
            assert torch.all(lp.top_ids.cpu()[valid] >= 0)
            hit = lp.top_ids == ids[:, 1:].unsqueeze(-1)
            assert torch.equal(lp.chosen[hit.any(-1)], lp.top_logprobs[hit])
            # the sequence log-likelihood and the per-token negative log-likelihood
            total = lp.cumulative().cpu().double()
            assert torch.allclose(total, torch.where(valid, want, torch.zeros_like(want)).sum(1), atol=ORACLE_TOL * l)
            nll = -lp.cumulative() / (lens - 1)
            assert torch.all(nll > 0)
            got[(bs, chunk)] = lp
            # the engine still serves a prefill and a decode afterwards
            first = eng.prefill(ids, lens)
            assert torch.equal(first.cpu(), torch.from_numpy(d["first_tokens"]))
            assert eng.decode(first, 4, use_graph=True).shape == (b, 4)
    for chunk in (None, 2):   # both pools: the same kernels through the same token table
        R.assert_close_logprobs(got[(4, chunk)].chosen, got[(None, chunk)].chosen.cpu().double(), f"pools chunk={chunk}")
        assert torch.equal(got[(4, chunk)].top_ids, got[(None, chunk)].top_ids)
    # chunked prefill attends through another kernel: the two agree to the route tolerance
    assert (got[(None, 2)].chosen - got[(None, None)].chosen).abs().max().item() <= ORACLE_TOL


@pytest.mark.parametrize("kv_block_size", [None, 16])
def test_score_long_prompt_in_small_logits_chunks(kv_block_size):
    m = _random_model()
    gen = torch.Generator().manual_seed(4)
    lens = torch.tensor([600, 431], dtype=torch.int32)
    ids = torch.randint(0, m.geo.vocab_size, (2, 600), generator=gen).to(DEV)
    eng = DecodeEngine(m, max_batch=2, max_seq_len=1024, kv_block_size=kv_block_size)
    one = eng.score(ids, lens.to(DEV), top_k=5)                    # 1029 rows: one chunk of logits
    small = eng.score(ids, lens.to(DEV), top_k=5, logits_rows=256)  # five chunks
    assert one.chosen.shape == (2, 599)
    valid = torch.arange(1, 600).unsqueeze(0) < lens.view(2, 1)
    assert torch.all(one.chosen.cpu()[~valid] == 0.0) and torch.all(one.chosen.cpu()[valid] < 0)
    assert torch.equal(small.top_ids, one.top_ids)
    R.assert_close_logprobs(small.chosen, one.chosen.cpu().double(), "small chunks chosen")
    R.assert_close_logprobs(small.top_logprobs, one.top_logprobs.cpu().double(), "small chunks top")
    first = eng.prefill(ids, lens.to(DEV))
    assert first.shape == (2,) and eng.decode(first, 4, use_graph=True).shape == (2, 4)
