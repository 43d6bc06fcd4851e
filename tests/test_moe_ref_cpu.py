"""CPU checks of the fused-MoE test reference (tests/_moe_ref.py): the float64 reference against the oracle on the golden
fixtures and on one seeded case per format, the signal condition on the old and the new input scaling, and the refined
tensor-parallel scale grids against the 128 x 128 grid they re-express.

The oracle rounds ``gate_up``, ``act`` and the per-slot rows to fp16; its distance from the float64 reference, max error over
the rms of the reference row, is the yardstick every GPU comparison scales (4 x): 1.6e-3 - 3.7e-3 on the cases below (the
largest: int8 per channel at hidden 256 / intermediate 128), asserted here to stay under 5e-3."""

import pytest
import torch

from oracle import oracle as O
from tests import _golden as G
from tests import _moe_ref as R

ORACLE_ERR_MAX = 5e-3  # fp16 roundings of gate_up, act and the slot rows: a few 2^-11 steps of a row's largest values


@pytest.mark.parametrize("name", G.names("fused_moe_"))
def test_moe_ref64_agrees_with_the_oracle_on_the_golden_fixtures(name):
    d = G.load(name)
    kw = {k: d[k] for k in ("w1_scale", "w2_scale", "group_n", "group_k") if k in d}
    ref = O.fused_moe(d["x"], d["w1"], d["w2"], d["topk_weights"], d["topk_ids"], **kw)
    ref64 = R.moe_ref64(d["x"], d["w1"], d["w2"], d["topk_weights"], d["topk_ids"], **R.groups_of(kw))
    err = R.moe_error(ref, ref64)
    print(f"{name}: oracle vs fp64 {err:.2e}; fixture vs fp64 {R.moe_error(d['out'], ref64):.2e}")
    assert err <= ORACLE_ERR_MAX


@pytest.mark.parametrize("fmt,tokens,experts,top_k,hidden,inter", [
    ("f16", 37, 8, 2, 256, 128),
    ("fp8_block", 37, 8, 2, 256, 128),
    ("int8_channel", 37, 8, 2, 256, 128),
    ("fp8_channel", 37, 8, 2, 256, 128),
    ("f16", 4, 8, 4, 2048, 768),
    ("fp8_block", 4, 8, 4, 2048, 768),
])
def test_moe_ref64_agrees_with_the_oracle_on_seeded_inputs(fmt, tokens, experts, top_k, hidden, inter):
    x, w1, w2, wts, ids, kw = R.moe_case(fmt, tokens, experts, top_k, hidden, inter, seed=11)
    ref = O.fused_moe(x, w1, w2, wts, ids, **kw)
    ref64 = R.moe_ref64(x, w1, w2, wts, ids, **R.groups_of(kw))
    R.assert_has_signal(ref64, 2e-2)
    err = R.moe_error(ref, ref64)
    print(f"{fmt} H {hidden} I {inter}: oracle vs fp64 {err:.2e}, zero passes {100 * R.zero_pass_share(ref64, 2e-2):.1f} %")
    assert err <= ORACLE_ERR_MAX
    # an all-zero output, or one wrong row, cannot meet a bound of that size
    assert R.moe_error(torch.zeros_like(ref), ref64) > 1.0
    wrong = ref.clone()
    wrong[tokens // 2] = ref[(tokens // 2 + 1) % tokens]
    with pytest.raises(AssertionError):
        R.assert_moe_close(wrong, ref64, 4 * err)


def test_moe_ref64_interleaved_rows_and_per_matrix_grids_describe_the_same_block():
    x, w1, w2, wts, ids, kw = R.moe_case("fp8_block", 5, 4, 2, 256, 128, seed=3)
    ref64 = R.moe_ref64(x, w1, w2, wts, ids, **R.groups_of(kw))
    inter = w1.shape[1] // 2
    pair = R.interleave_rows
    rows = kw["w1_scale"].repeat_interleave(128, dim=1)[:, : 2 * inter]
    got = R.moe_ref64(x, pair(w1), w2, wts, ids, w1_scale=pair(rows), w2_scale=kw["w2_scale"], w1_group=(1, 128),
                      w2_group=(128, 128), w1_interleaved=True)
    assert torch.equal(got, ref64)


def test_assert_has_signal_rejects_the_old_scaling_and_accepts_the_new_one():
    g = torch.Generator().manual_seed(0)
    tokens, experts, top_k, hidden, inter = 37, 8, 2, 256, 128
    x = (torch.randn(tokens, hidden, generator=g) / hidden**0.5).half()  # the scaling these tests used to have
    w1 = (torch.randn(experts, 2 * inter, hidden, generator=g) / hidden**0.5).half()
    w2 = (torch.randn(experts, hidden, inter, generator=g) / inter**0.5).half()
    ids = torch.randint(0, experts, (tokens, top_k), generator=g)
    wts = torch.softmax(torch.randn(tokens, top_k, generator=g), dim=-1).half()
    old = R.moe_ref64(x, w1, w2, wts, ids)
    assert R.zero_pass_share(old, 2e-2) == 1.0
    with pytest.raises(AssertionError):
        R.assert_has_signal(old, 2e-2)
    torch.testing.assert_close(torch.zeros_like(old), old, rtol=2e-2, atol=2e-2)  # what made those tests vacuous
    for fmt in ("f16", "fp8_block", "int8_channel"):
        x, w1, w2, wts, ids, kw = R.moe_case(fmt, tokens, experts, top_k, hidden, inter, seed=1)
        new = R.moe_ref64(x, w1, w2, wts, ids, **R.groups_of(kw))
        assert R.assert_has_signal(new, 2e-2) <= 0.10
        with pytest.raises(AssertionError):
            torch.testing.assert_close(torch.zeros_like(new), new, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("cut", [64, 32])
def test_refined_scale_grids_dequantise_to_the_128_block_weights(cut):
    """A tensor-parallel shard that cuts the 128 x 128 blocks stores its scales on gcd(128, shard) channels (gate|up along N,
    down along K, weights.expand_scale_grid): the same dequantised weights, and a shard's block is the matching slice."""
    from lite_llama_amd.weights import expand_scale_grid

    g = torch.Generator().manual_seed(cut)
    experts, hidden, inter = 3, 256, 384
    w1, s1 = R.fp8_block_experts(experts, 2 * inter, hidden, g)
    w2, s2 = R.fp8_block_experts(experts, hidden, inter, g)
    s1f, s2f = expand_scale_grid(s1, 1, 128, cut), expand_scale_grid(s2, 2, 128, cut)
    assert s1f.shape[1] == 2 * inter // cut and s2f.shape[2] == inter // cut
    assert torch.equal(R.dequant64(w1, s1f, (cut, 128)), R.dequant64(w1, s1, (128, 128)))
    assert torch.equal(R.dequant64(w2, s2f, (128, cut)), R.dequant64(w2, s2, (128, 128)))
    # one shard of 3 * cut channels (not a multiple of 128): rows / columns [lo, hi) of the whole
    lo, hi = cut, 4 * cut
    w1s = torch.cat([w1[:, lo:hi], w1[:, inter + lo:inter + hi]], dim=1)
    s1s = torch.cat([s1f[:, lo // cut:hi // cut], s1f[:, (inter + lo) // cut:(inter + hi) // cut]], dim=1)
    whole1 = R.dequant64(w1, s1, (128, 128))
    assert torch.equal(R.dequant64(w1s, s1s, (cut, 128)), torch.cat([whole1[:, lo:hi], whole1[:, inter + lo:inter + hi]], dim=1))
    assert torch.equal(R.dequant64(w2[:, :, lo:hi], s2f[:, :, lo // cut:hi // cut], (128, cut)),
                       R.dequant64(w2, s2, (128, 128))[:, :, lo:hi])
    # and the shards partition the block: their float64 outputs add up to the whole
    x, _, _, wts, ids, _ = R.moe_case("fp8_block", 6, experts, 2, hidden, 128, seed=5)
    whole = R.moe_ref64(x, w1, w2, wts, ids, w1_scale=s1, w2_scale=s2, w1_group=(128, 128), w2_group=(128, 128))
    parts = torch.zeros_like(whole)
    for lo in range(0, inter, 3 * cut):
        hi = lo + 3 * cut
        w1s = torch.cat([w1[:, lo:hi], w1[:, inter + lo:inter + hi]], dim=1)
        s1s = torch.cat([s1f[:, lo // cut:hi // cut], s1f[:, (inter + lo) // cut:(inter + hi) // cut]], dim=1)
        parts += R.moe_ref64(x, w1s, w2[:, :, lo:hi], wts, ids, w1_scale=s1s, w2_scale=s2f[:, :, lo // cut:hi // cut],
                             w1_group=(cut, 128), w2_group=(128, cut))
    torch.testing.assert_close(parts, whole, rtol=1e-12, atol=1e-12)


def test_moe_gemm_ref64_is_the_block_reference_taken_apart():
    x, w1, w2, wts, ids, kw = R.moe_case("int8_channel", 9, 4, 2, 128, 64, seed=2)
    top_k, inter = ids.shape[1], w1.shape[1] // 2
    gu = R.moe_gemm_ref64(x, w1, ids, top_k, scale=kw["w1_scale"], group=(1, 128))
    g, u = gu[:, :inter], gu[:, inter:]
    rows = R.moe_gemm_ref64(g * torch.sigmoid(g) * u, w2, ids, 1, scale=kw["w2_scale"], group=(1, 128), slot_weights=wts)
    torch.testing.assert_close(rows.view(9, top_k, -1).sum(1), R.moe_ref64(x, w1, w2, wts, ids, **R.groups_of(kw)),
                               rtol=1e-12, atol=1e-12)
