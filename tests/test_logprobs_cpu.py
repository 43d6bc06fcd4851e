"""CPU tier of the token log-probability feature: the C ABI (header, ctypes table, host-side scratch query), wrapper
validation before any launch, the test reference itself against hand-computed rows, TokenLogprobs.cumulative and the
split of CausalLM.forward into its two halves."""

import math
import os
import re

import pytest
import torch

from tests import _logprobs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_token_logprobs():
    from lite_llama_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lite_llama_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(ll_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in ("ll_token_logprobs", "ll_token_logprobs_scratch_bytes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["ll_token_logprobs"]) == 18
    q = lib.ll_token_logprobs_scratch_bytes
    assert q(64, 152064, 20) > 0 and q(64, 152064, 0) > 0
    # grows with rows: never shrinks (rows x chunks is held near one grid size while rows are split into chunks), and
    # grows strictly from regime to regime and once every row is one chunk
    sizes = [q(r, 152064, 20) for r in (1, 3, 64, 128, 257, 2048, 4096, 8192)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[2] > sizes[0] and sizes[5] > sizes[2] and sizes[7] == 2 * sizes[6] > sizes[5], sizes
    assert q(64, 152064, 20) > q(64, 152064, 5)
    assert q(64, 152064, 20) % 4 == 0
    # error codes without a device: LL_ERR_SHAPE (-2) for no rows / no vocabulary, LL_ERR_ARG (-3) for a bad top_k
    assert q(0, 152064, 5) == -2 and q(-1, 152064, 5) == -2 and q(4, 0, 0) == -2
    assert q(4, 152064, 21) == -3 and q(4, 152064, -1) == -3 and q(4, 10, 11) == -3


def test_wrapper_validates_before_launch():
    from lite_llama_amd.sampling import TokenLogprobs, token_logprobs

    logits = torch.zeros(4, 32)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        token_logprobs(logits, ids, 3)
    with pytest.raises(ValueError, match="top_k"):
        token_logprobs(logits, ids, 21)
    with pytest.raises(ValueError, match="top_k"):
        token_logprobs(logits, ids, -1)
    with pytest.raises(ValueError, match="top_k"):
        token_logprobs(logits, ids, 33)  # beyond 20 and beyond the vocabulary
    with pytest.raises(ValueError, match="exceeds the vocabulary"):
        token_logprobs(torch.zeros(4, 8), ids, 9)
    with pytest.raises(ValueError, match="one id per row"):
        token_logprobs(logits, torch.zeros(5, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="int64"):
        token_logprobs(logits, ids.int(), 3)
    with pytest.raises(ValueError, match="rows, vocab"):
        token_logprobs(torch.zeros(2, 4, 32), ids, 3)
    with pytest.raises(ValueError, match="nothing to compute"):
        token_logprobs(logits, None, 0)
    with pytest.raises(ValueError, match="column"):
        token_logprobs(logits, ids, 0, column=torch.zeros(1, dtype=torch.int64))
    bad = TokenLogprobs(torch.zeros(4, 3), torch.zeros(4, 3, 2), torch.zeros(4, 3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="top_k"):
        token_logprobs(logits, ids, 3, out=bad)
    with pytest.raises(ValueError, match="chosen"):
        token_logprobs(logits, ids, 2, out=TokenLogprobs(torch.zeros(5, 3), bad.top_logprobs, bad.top_ids))


def test_engine_rejects_bad_logprobs_argument():
    from lite_llama_amd.executor import _check_logprobs

    assert _check_logprobs(None) is None and _check_logprobs(0) == 0 and _check_logprobs(20) == 20
    for bad in (-1, 21):
        with pytest.raises(ValueError, match="logprobs"):
            _check_logprobs(bad)


def test_reference_all_equal_row():
    v, k = 1000, 7
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        z = torch.full((2, v), 1.5, dtype=dtype)
        chosen, top_lp, top_ids = R.ref_logprobs(z, torch.tensor([0, v - 1]), k)
        assert torch.allclose(chosen, torch.full((2,), -math.log(v), dtype=torch.float64), atol=1e-12)
        assert torch.allclose(top_lp, torch.full((2, k), -math.log(v), dtype=torch.float64), atol=1e-12)
        assert torch.equal(top_ids, torch.arange(k).expand(2, k))


def test_reference_tie_run_straddles_k():
    # values: one 5.0 at index 9, then a run of four 3.0 at indices 2, 4, 6, 11, the rest 0.0; k = 3 cuts the run after 4
    z = torch.zeros(1, 16, dtype=torch.float16)
    z[0, 9] = 5.0
    z[0, [2, 4, 6, 11]] = 3.0
    _, top_lp, top_ids = R.ref_logprobs(z, None, 3)
    assert top_ids.tolist() == [[9, 2, 4]]
    lse = math.log(math.exp(5.0) + 4 * math.exp(3.0) + 11)
    assert torch.allclose(top_lp, torch.tensor([[5.0 - lse, 3.0 - lse, 3.0 - lse]], dtype=torch.float64), atol=1e-12)
    _, _, ids6 = R.ref_logprobs(z, None, 6)
    assert ids6.tolist() == [[9, 2, 4, 6, 11, 0]]
    chosen, _, _ = R.ref_logprobs(z, torch.tensor([16]), 0)
    assert torch.isnan(chosen).all()


def test_reference_prefiltered_order_equals_plain_sort():
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(6, 5000, generator=g) * 4).half().double()  # fp16 values: full of exact ties
    z[5] = 2.0
    for k in (1, 5, 20):
        assert torch.equal(R.ref_top_ids(z, k, plain=True), R.ref_top_ids(z, k, plain=False))


def test_cumulative():
    from lite_llama_amd.sampling import TokenLogprobs

    chosen = torch.tensor([[-1.0, -2.0, -4.0], [-0.5, -0.25, -8.0]])
    lp = TokenLogprobs(chosen, torch.zeros(2, 3, 0), torch.zeros(2, 3, 0, dtype=torch.int64))
    assert torch.equal(lp.cumulative(), torch.tensor([-7.0, -8.75]))
    assert torch.equal(lp.cumulative(torch.tensor([2, 0])), torch.tensor([-3.0, 0.0]))
    assert torch.equal(lp.cumulative(torch.tensor([3, 1], dtype=torch.int32)), torch.tensor([-7.0, -0.5]))
    with pytest.raises(ValueError):
        TokenLogprobs(None, lp.top_logprobs, lp.top_ids).cumulative()


def test_forward_is_the_composition_of_its_halves(monkeypatch):
    """On the CPU the norm kernel is not available: a tiny model without decoder layers, with the final norm replaced by
    the same function on both sides, exercises exactly the code that was split."""
    from lite_llama_amd import model as M

    def rms(x, residual, weight, eps):
        assert residual is None
        v = x.float()
        return (v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * weight, None

    monkeypatch.setattr(M, "add_norm", rms)
    geo = M.tiny_geometry(num_layers=0, hidden_size=64, vocab_size=96, num_heads=2, num_kv_heads=1, head_dim=32,
                          intermediate_size=128)
    m = M.CausalLM(geo)
    g = torch.Generator().manual_seed(1)
    m.embed_tokens.weight.copy_(torch.randn(96, 64, generator=g).half())
    if m.lm_head_weight is not m.embed_tokens.weight:
        m.lm_head_weight.copy_(torch.randn(96, 64, generator=g).half())
    m.norm_weight.copy_((1 + 0.1 * torch.randn(64, generator=g)).half())
    ids = torch.randint(0, 96, (2, 5), generator=g)
    pos = torch.arange(5).unsqueeze(0).expand(2, 5)
    full = m(ids, pos, None)
    h = m.final_hidden_states(ids, pos, None)
    assert h.shape == (2, 5, 64) and full.shape == (2, 5, 96)
    assert torch.equal(full, m.logits_from_hidden(h))
    rows = torch.tensor([4, 7])
    assert torch.equal(m(ids, pos, None, logits_rows=rows), m.logits_from_hidden(h.view(-1, 64)[rows]))
    assert torch.equal(m(ids, pos, None, logits_rows=rows), full.view(-1, 96)[rows])
