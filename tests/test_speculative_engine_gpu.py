"""``DecodeEngine.decode(speculate=...)`` end to end on the tiny models: drafts never change the output (exact), the output
passes the teacher-forced oracle criterion, the acceptance statistics equal the reference simulator's
(tests/_spec_ref.py), eager equals captured, ``stop`` works inside accepted runs, and every refused combination raises."""

import math

import pytest
import torch

from lite_llama_amd.executor import DecodeEngine, Speculation, StopCriteria
from lite_llama_amd.quantization import QuantConfig
from tests import _spec_ref as R
from tests.test_chunked_prefill_gpu import _load, _oracle_ranks_engine_tokens, _random_model
from tests.test_model_step import _hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
DENSE = ["llama", "qwen2", "qwen3"]
_models = {}


def _setup(name):
    """(model, prompt ids, lens, max_seq_len, block size, new tokens) -- built once per module."""
    if name not in _models:
        if name in ("geom128", "geom128_w4"):
            m = _random_model(seed=3)
            if name.endswith("w4"):
                m.quantize_(QuantConfig.int4_groupwise(128))
            gen = torch.Generator().manual_seed(11)
            lens = torch.tensor([61, 130], dtype=torch.int32)
            ids = torch.randint(0, m.geo.vocab_size, (2, 130), generator=gen)
            _models[name] = (m, ids.to(DEV), lens.to(DEV), 256, 16, 40)
        else:
            d, params = _load(name)
            m = _hip_model(params, None, name)
            _models[name] = (m, torch.from_numpy(d["prompt_ids"]).to(DEV), torch.from_numpy(d["lens"]).int().to(DEV), 64, 4, 24)
    return _models[name]


def _decode(name, spec, use_graph=False, stop=None, eng=None, n=None, **engine_kw):
    m, ids, lens, s, bs, n_default = _setup(name)
    n = n_default if n is None else n
    if eng is None:
        eng = DecodeEngine(m, max_batch=ids.shape[0], max_seq_len=s, kv_block_size=bs, **engine_kw)
    first = eng.prefill(ids, lens)
    toks = eng.decode(first, n, use_graph=use_graph, speculate=spec, stop=stop)
    torch.cuda.synchronize()
    return toks.cpu(), eng, first.cpu()


def _stats(eng):
    sp = eng.last_speculation
    return (sp.verify_steps.cpu().tolist(), sp.drafted.cpu().tolist(), sp.accepted.cpu().tolist(),
            sp.accepted_per_step.cpu().tolist(), sp.steps_run)


@pytest.mark.parametrize("k", [1, 3, 4, 7])
@pytest.mark.parametrize("name", DENSE + ["geom128", "geom128_w4"])
def test_drafts_never_change_the_output(name, k):
    """The grid width fixes every GEMM route, every row's arithmetic is independent of its neighbours and masked keys
    contribute exact zeros: whatever is drafted, the tokens are those of the same ``k`` with empty drafts -- exactly."""
    vocab = _setup(name)[0].geo.vocab_size
    base, eng, _ = _decode(name, Speculation(num_draft_tokens=k, ngram=False))
    assert _stats(eng)[1] == [0] * base.shape[0] and eng.last_speculation.steps_run == base.shape[1]
    third = base.clone()
    third[:, 2::3] = (third[:, 2::3] + 1) % vocab
    sources = {
        "ngram": Speculation(num_draft_tokens=k),
        "true": Speculation(num_draft_tokens=k, ngram=False, predicted_ids=base),
        "third": Speculation(num_draft_tokens=k, predicted_ids=third),
        "wrong": Speculation(num_draft_tokens=k, ngram=False, predicted_ids=(base + 1) % vocab),
    }
    for src, spec in sources.items():
        toks, eng, _ = _decode(name, spec)
        assert torch.equal(toks, base), (name, k, src, (toks != base).nonzero()[:4].tolist())
        _, drafted, accepted, _, steps = _stats(eng)
        if src == "true":
            # the drafts did something: every step after the first takes k + 1 tokens
            assert sum(accepted) > 0 and steps < base.shape[1], (name, k, drafted, accepted, steps)
        assert eng.pool.error == 0


@pytest.mark.parametrize("name", DENSE + ["qwen3_moe"])
def test_output_passes_the_oracle_criterion(name):
    d, params = _load(name)
    plain, eng, _ = _decode(name, None, use_graph=True)
    for spec in (Speculation(num_draft_tokens=4), Speculation(num_draft_tokens=3, predicted_ids=plain)):
        toks, eng, _ = _decode(name, spec, use_graph=True)
        assert eng.info.b_ctx_len is None and eng.info.max_ctx_len == 0
        _oracle_ranks_engine_tokens(d, params, name, toks)


def _replayed(name, toks, first, k, lengths=None, **rule):
    _, ids, lens, s, _, n = _setup(name)
    prompts = [ids[i, :int(lens[i])].cpu().tolist() for i in range(ids.shape[0])]
    rec = [toks[i, :n if lengths is None else lengths[i]].tolist() for i in range(toks.shape[0])]
    return R.replay(rec, first.tolist(), prompts, toks.shape[1], k, s, **rule)


@pytest.mark.parametrize("name", DENSE)
def test_acceptance_accounting(name):
    k, c = 3, 2
    base, _, _ = _decode(name, Speculation(num_draft_tokens=k, ngram=False))
    n = base.shape[1]
    for rule, kw in (("ngram", {}), ("true", dict(predicted=base.tolist()))):
        spec = Speculation(num_draft_tokens=k, check_every=c, predicted_ids=base if rule == "true" else None)
        toks, eng, first = _decode(name, spec, use_graph=True)
        rows, s = _replayed(name, toks, first, k, **kw)
        if rule == "true":
            assert s <= n // 2, (s, n)                       # on the simulator alone: the prediction at least halves the steps
        verify, drafted, accepted, per_step, steps_run = _stats(eng)
        assert s <= steps_run <= min(n, (math.ceil(s / c) + 1) * c), (s, steps_run)
        for i, r in enumerate(rows):
            assert (verify[i], drafted[i], accepted[i]) == (r.verify_steps, r.drafted, r.accepted), (rule, i)
            want = r.accepted_per_step + [-1] * (steps_run - len(r.accepted_per_step))
            assert per_step[i] == want, (rule, i, per_step[i], want)
            assert r.out == toks[i].tolist()


@pytest.mark.parametrize("name", ["qwen2", "geom128_w4"])
def test_eager_equals_captured_and_the_engine_is_reusable(name):
    k = 4
    _, ids, lens, s, bs, n = _setup(name)
    spec = Speculation(num_draft_tokens=k)
    eager, eng_e, _ = _decode(name, spec, use_graph=False)
    captured, eng, _ = _decode(name, spec, use_graph=True)
    assert torch.equal(eager, captured)
    assert _stats(eng_e) == _stats(eng)
    stats = _stats(eng)
    again, _, _ = _decode(name, spec, use_graph=True, eng=eng)           # a second prefill + decode on the same engine
    assert torch.equal(again, captured) and _stats(eng) == stats
    assert eng.pool.error == 0
    held = eng.pool.req_blocks.cpu().tolist()
    for i in range(ids.shape[0]):
        final_len = int(lens[i]) + n
        assert held[i] <= math.ceil((final_len + k) / bs), (i, held[i], final_len)
    # a pool that shares blocks is allowed: writes land at or beyond the row's own length
    shared, eng_s, _ = _decode(name, spec, use_graph=True, kv_share_blocks=True)
    assert torch.equal(shared, captured) and eng_s.pool.error == 0


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_stop_inside_accepted_runs(name):
    k, pad = 3, 1
    base, eng, first = _decode(name, Speculation(num_draft_tokens=k, ngram=False))
    base_steps = eng.last_steps_run
    n = base.shape[1]
    # a stop id from the output itself, so that it hits -- inside row 0's run, and not a token prefill returned where
    # there is a choice (a row whose prefill token is a stop id starts finished: length 0, reason 1)
    stop_id = next((t for t in base[0, 4:].tolist() if t not in first.tolist()), int(base[0, 7]))
    max_tokens = [100, 5]
    stop = StopCriteria(stop_token_ids=[stop_id], max_tokens=max_tokens, pad_token_id=pad, check_every=1)
    spec = Speculation(num_draft_tokens=k, ngram=False, predicted_ids=base, check_every=1)
    for use_graph in (False, True):
        toks, eng, first = _decode(name, spec, use_graph=use_graph, stop=stop)
        lengths, reasons = eng.last_lengths.cpu().tolist(), eng.last_finish_reasons.cpu().tolist()
        for i in range(base.shape[0]):
            hits = (base[i] == stop_id).nonzero().view(-1).tolist()
            at = 0 if int(first[i]) == stop_id else hits[0] + 1 if hits else n + 1
            want_len = min(at, max_tokens[i], n)
            want_reason = 1 if at <= min(max_tokens[i], n) else 3 if max_tokens[i] <= n else 0
            assert (lengths[i], reasons[i]) == (want_len, want_reason), (i, lengths, reasons)
            assert torch.equal(toks[i, :want_len], base[i, :want_len])
            assert torch.all(toks[i, want_len:] == pad)
        assert eng.last_steps_run < base_steps and eng.last_speculation.steps_run == eng.last_steps_run
        rows, s = _replayed(name, toks, first, k, lengths=lengths, predicted=base.tolist(), ngram=False,
                            stop_ids=(stop_id,), max_tokens=max_tokens)
        assert [r.accepted for r in rows] == eng.last_speculation.accepted.cpu().tolist()
        assert [r.length for r in rows] == lengths


def test_refused_combinations_and_the_untouched_plain_route():
    m, ids, lens, s, bs, n = _setup("qwen2")
    spec = Speculation(num_draft_tokens=2)

    def engine(**kw):
        kw.setdefault("kv_block_size", bs)
        eng = DecodeEngine(m, max_batch=4, max_seq_len=kw.pop("max_seq_len", s), **kw)
        return eng, eng.prefill(ids, lens)

    eng, first = engine(kv_block_size=None)
    with pytest.raises(ValueError, match="paged pool"):
        eng.decode(first, 4, speculate=spec)
    eng, first = engine(kv_dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="e4m3"):
        eng.decode(first, 4, speculate=spec)
    eng, first = engine()
    sampling = type("S", (), dict(temperature=0.7, top_p=0.9, repetition_penalty=1.0))()
    for kw, what in ((dict(sampling=sampling), "sampling"), (dict(logprobs=0), "logprobs"), (dict(constraint=object()), "constraint"),
                     (dict(steps_per_graph=2), "steps_per_graph"),
                     (dict(stop=StopCriteria(stop_sequences=[[1, 2]])), "stop_sequences")):
        with pytest.raises(ValueError, match=what):
            eng.decode(first, 4, speculate=spec, **kw)
    with pytest.raises(ValueError, match="Speculation"):
        eng.decode(first, 4, speculate=2)
    with pytest.raises(ValueError, match="predicted_ids"):
        eng.decode(first, 4, speculate=Speculation(num_draft_tokens=2, predicted_ids=torch.zeros(3, 4, dtype=torch.long)))
    # the refusals left the prefill usable
    want = eng.decode(first, 6, speculate=Speculation(num_draft_tokens=2, ngram=False))
    with pytest.raises(ValueError, match="already continued"):
        eng.decode(first, 4, speculate=spec)
    small, first = engine(max_seq_len=16)
    with pytest.raises(ValueError, match="does not fit"):
        small.decode(first, 4, speculate=Speculation(num_draft_tokens=15))
    shared = DecodeEngine(m, max_batch=4, max_seq_len=s, kv_block_size=bs, kv_share_blocks=True)
    first = shared.prefill(ids[:, 2:], lens - 2, shared_prefix_ids=ids[0, :2])
    with pytest.raises(ValueError, match="shared_prefix_ids"):
        shared.decode(first, 4, speculate=spec)
    first = shared.prefill(ids, lens, num_samples=2)
    with pytest.raises(ValueError, match="num_samples"):
        shared.decode(first, 4, speculate=spec)
    # speculate=None is the decode there was: same tokens, and no speculative state is made
    eng, first = engine()
    plain = eng.decode(first, 6, speculate=None)
    assert eng.last_speculation is None
    eng2, first2 = engine()
    assert torch.equal(plain, eng2.decode(first2, 6)) and torch.equal(first, first2)
    assert plain.shape == want.shape
