"""One DecodeEngine, one prefill route after another: every route must leave the engine as a fresh engine's, whatever ran
before it -- shared-prefix fields, chunk metadata, log-probability buffers, stop state and the pools' bookkeeping are all
per-run state on a long-lived object.  Each run on the reused engine is compared, bit for bit, with the same run on an engine
that has done nothing else."""

import functools

import pytest
import torch

from lite_llama_amd.executor import StopCriteria
from lite_llama_amd.kernels import attention as A
from tests.test_stop_engine_gpu import DEV, _engine, _model, _prompts

pytestmark = pytest.mark.gpu
STEPS = 6


def _prefix():
    g = torch.Generator().manual_seed(23)
    return torch.randint(0, _model().geo.vocab_size, (72,), generator=g).to(DEV)       # off the block boundaries of 16


@functools.lru_cache(maxsize=None)
def _stops():
    """Stops that certainly occur in the chunked run: a stop id (row 0), a 2-token sequence (row 3), a max_tokens (row 4)."""
    ids, lens = _prompts()
    eng = _engine()
    t = eng.decode(eng.prefill(ids, lens, chunk_size=16), STEPS).tolist()
    limits = [1000] * 8
    limits[4] = 3
    return StopCriteria(stop_token_ids=[t[0][2]], stop_sequences=[[t[3][1], t[3][2]]], max_tokens=limits, pad_token_id=1,
                        check_every=2)


def _decoded(eng, first, **kw):
    toks = eng.decode(first, STEPS, **kw)
    lp = eng.last_logprobs
    return {"first": first, "tokens": toks, "lengths": eng.last_lengths, "reasons": eng.last_finish_reasons,
            "steps_run": eng.last_steps_run, "seq_len": eng.info.b_seq_len, "shared": eng.info.shared_prefix_len,
            **({} if lp is None else {"chosen": lp.chosen, "top_logprobs": lp.top_logprobs, "top_ids": lp.top_ids})}


def _with_first_logprobs(eng, out):
    lp = eng.first_logprobs
    return {**out, "first_chosen": lp.chosen, "first_top_logprobs": lp.top_logprobs, "first_top_ids": lp.top_ids}


def _run_shared(eng):
    ids, lens = _prompts()
    return _decoded(eng, eng.prefill(ids, lens, shared_prefix_ids=_prefix()))


def _run_samples(eng):
    ids, lens = _prompts()
    first = eng.prefill(ids[:4].contiguous(), lens[:4].contiguous(), num_samples=2)
    assert first.shape == (8,)
    return _decoded(eng, first)


def _run_chunked_stop(eng):
    ids, lens = _prompts()
    first = eng.prefill(ids, lens, chunk_size=16, logprobs=2)
    out = _with_first_logprobs(eng, _decoded(eng, first, stop=_stops(), logprobs=2, steps_per_graph=3))
    assert any(out["reasons"].tolist()) and not all(out["reasons"].tolist())
    return out


def _run_score(eng):
    ids, lens = _prompts()
    lp = eng.score(ids, lens, top_k=2)
    return {"chosen": lp.chosen, "top_logprobs": lp.top_logprobs, "top_ids": lp.top_ids}


def _run_synthetic(eng):
    return _decoded(eng, eng.synthetic_context(8, 32, seed=3))


def _run_plain(eng):
    ids, lens = _prompts()
    out = _decoded(eng, eng.prefill(ids, lens))
    assert eng.first_logprobs is None and out["lengths"] is None and out["shared"] == 0 and "chosen" not in out
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("bs,share", [(None, False), (16, True)], ids=["bump", "paged16-shared"])
def test_every_route_on_a_used_engine_equals_the_route_alone(bs, share, monkeypatch):
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 64)         # the shared run's decode steps take the shared-prefix route
    runs = [_run_shared] + ([_run_samples] if share else []) + [_run_chunked_stop, _run_score, _run_synthetic, _run_plain]
    reused = _engine(bs, share)
    for run in runs:
        got = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in run(reused).items()}
        want = run(_engine(bs, share))
        assert got.keys() == want.keys(), run.__name__
        for key in want:
            assert _same(got[key], want[key]), (run.__name__, key, got[key], want[key])
    if bs is not None:
        assert reused.pool.error == 0
