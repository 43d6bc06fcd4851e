"""Attention kernels against float64 references on inputs where the softmax weights matter (tests/_attn_ref.py):
wide scores, spotlit keys swept over the partition edges, per-head spotlights inside a GQA group, rising and falling
ramps, offset V, and poisoned pool rows past each row's length.  The bound is the rounding model of
``_attn_ref.bound``; tests/test_attention_regimes_cpu.py shows it rejects broken versions of the algorithm.

Every decode case first asserts the form its shape reaches (single partition, the one-workgroup LDS merge, the walking
waves, the counter merge, the two-launch form), from the library's own dispatch queries and the device's CU count.
"""

import pytest
import torch

import lite_llama_amd._lib as L
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
BIG = 3000   # contexts above this run the cheaper regime subset


def K():
    import lite_llama_amd.kernels as k

    return k


def _cus():
    return torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count


def decode_form(max_len, batch, hq, hkv, two_launch=False):
    """The decode form ``flash_decoding`` takes (host dispatch of csrc/flash_decoding.hip::launch_fd)."""
    lib = L.lib()
    nparts = lib.ll_flash_decoding_num_partitions(max_len)
    hgroups = (hq // hkv + 15) // 16
    waves = lib.ll_flash_decoding_group_waves(max_len, batch * hkv * hgroups)
    if two_launch:
        return "two_launch"
    if nparts <= 1:
        return "single"
    if waves >= 2:
        return "lds" if nparts <= R.FD_GROUP_MAX else "walk"
    return "counter"


def _batch(form, hq, hkv):
    """Batch that reaches ``form``: the walking waves (and the counter merge past 256 partitions) need batch x KV heads
    x head groups to fill half the chip; the small-batch counter merge needs it below that."""
    hgroups = (hq // hkv + 15) // 16
    if form in ("walk", "counter_big"):
        return -(-(_cus() // 2) // (hkv * hgroups))
    return 2 if form == "counter" else 4


def _lens(ctx, batch, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(1, ctx // 2), ctx + 1, (batch,), generator=g).tolist()
    lens[0] = ctx
    if batch > 1:
        lens[1] = max(1, ctx - 1)
    if batch > 2:
        lens[2] = R.FD_PART * ((ctx - 1) // R.FD_PART) + 1    # one token into the last partition
    if batch > 3:
        lens[3] = min(ctx, R.FD_PART + 1)
    return lens


def _regimes(ctx):
    return R.DECODE_REGIMES if ctx <= BIG else ("spotlight", "split", "wide", "poison")


def _check_decode(name, out, inp, pool, dtype):
    hkv = inp["hkv"]
    ref, vmax, z, n = R.decode_ref(inp["q"], pool[:, :hkv], pool[:, hkv:], inp["scale"], inp["table"], inp["req"],
                                   inp["seq"])
    return R.assert_within(out, ref, R.bound(ref, vmax, z, n, dtype), name)


# (form, context, hq, hkv, head dim, dtype): every form; GQA buckets 4 (8/2), 8 (28/4), 16 (14/1) and 32/1 (two head
# groups); head dims 64 / 128; bf16 on the LDS-merge, walking and counter-merge forms
DECODE_CASES = [
    ("single", 128, 8, 2, 64, F16),
    ("single", 128, 28, 4, 128, F16),
    ("single", 128, 32, 1, 64, BF16),
    ("lds", 1000, 8, 2, 64, F16),
    ("lds", 1000, 28, 4, 128, F16),
    ("lds", 1000, 14, 1, 128, F16),
    ("lds", 1000, 32, 1, 64, F16),
    ("lds", 1000, 28, 4, 128, BF16),
    ("lds", 600, 32, 1, 128, BF16),
    ("walk", 1025, 28, 4, 128, F16),
    ("walk", 1025, 32, 1, 64, F16),
    ("walk", 8200, 28, 4, 128, F16),
    ("walk", 32768, 8, 2, 128, F16),
    ("walk", 2000, 14, 1, 64, BF16),
    ("walk", 8200, 28, 4, 128, BF16),
    ("counter", 3000, 28, 4, 128, F16),
    ("counter", 2000, 8, 2, 64, F16),
    ("counter", 3000, 32, 1, 128, F16),
    ("counter", 2000, 14, 1, 64, BF16),
    ("counter_big", 32769, 28, 4, 128, F16),
    ("two_launch", 3000, 28, 4, 128, F16),
    ("two_launch", 600, 8, 2, 64, BF16),
    ("two_launch", 2000, 32, 1, 128, F16),
]


@pytest.mark.parametrize("form,ctx,hq,hkv,d,dtype", DECODE_CASES,
                         ids=[f"{f}-{c}-{a}x{b}-d{d}-{str(t)[6:]}" for f, c, a, b, d, t in DECODE_CASES])
def test_flash_decoding_regimes_match_fp64(form, ctx, hq, hkv, d, dtype, monkeypatch):
    import lite_llama_amd.kernels.attention as A

    batch = _batch(form, hq, hkv)
    two = form == "two_launch"
    assert decode_form(ctx, batch, hq, hkv, two) == ("counter" if form == "counter_big" else form)
    if form == "counter_big":
        assert L.lib().ll_flash_decoding_num_partitions(ctx) > 256       # one step past the walking form's last lap
    if two:
        monkeypatch.setattr(A, "_merge_counters", lambda device, entries: None)
    lens = _lens(ctx, batch, ctx + hq)
    for regime in _regimes(ctx):
        inp = R.decode_inputs(regime, lens, hq, hkv, d, dtype, seed=ctx * 31 + hq, device=DEV)
        pool = inp["pool"]

        def run(p):
            return K().flash_decoding(inp["q"], p[:, :hkv], p[:, hkv:], inp["scale"], inp["table"], inp["req"],
                                      inp["seq"], ctx)

        out = run(pool)
        name = f"decode {form} {str(dtype)[6:]} d{d} {hq}/{hkv} ctx{ctx} {regime}"
        _check_decode(name, out, inp, pool, dtype)
        if regime == "poison":
            clean = R.clean_pool(inp)
            assert torch.equal(run(clean).view(torch.int16), out.view(torch.int16)), name + ": poison leaked"


# fp8 (OCP e4m3) pool: grouped (LDS merge) and counter-merged, head dims 64 / 128
FP8_CASES = [("lds", 1000, 28, 4, 128), ("lds", 700, 8, 2, 64), ("counter", 3000, 28, 4, 128), ("counter", 2000, 8, 2, 64)]


@pytest.mark.parametrize("form,ctx,hq,hkv,d", FP8_CASES, ids=[f"{f}-{c}-{a}x{b}-d{d}" for f, c, a, b, d in FP8_CASES])
def test_flash_decoding_fp8kv_regimes_match_fp64_on_the_widened_pool(form, ctx, hq, hkv, d):
    batch = _batch(form, hq, hkv)
    assert decode_form(ctx, batch, hq, hkv) == form
    ks, vs = 0.5, 2.0
    for regime in ("spotlight", "wide"):
        inp = R.decode_inputs(regime, _lens(ctx, batch, ctx), hq, hkv, d, F16, seed=ctx + d, device=DEV)
        codes, wide = R.fp8_pool(inp["pool"], ks, vs, hkv)
        out = K().flash_decoding_fp8kv(inp["q"], codes[:, :hkv], codes[:, hkv:], inp["scale"], inp["table"],
                                       inp["req"], inp["seq"], ctx, ks, vs)
        _check_decode(f"decode-fp8kv {form} d{d} {hq}/{hkv} ctx{ctx} {regime}", out, inp, wide, F16)


def _rope_tables(n, d, dtype):
    inv = 1.0 / (1e6 ** (torch.arange(0, d, 2, device=DEV, dtype=torch.float32) / d))
    fr = torch.arange(n, device=DEV, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _new_token_inputs(ctx, batch, hq, hkv, d, dtype, seed):
    """A spotlight pool plus this step's q | k_new | v_new whose NEW token leads every head by about 15: a stale pool
    row in its place costs O(vmax)."""
    inp = R.decode_inputs("spotlight", _lens(ctx, batch, seed), hq, hkv, d, dtype, seed=seed, device=DEV)
    g = hq // hkv
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    qd = inp["q"].double().view(batch, hkv, g, d)
    lead = torch.stack([torch.full((hkv, g), R._spot_offset(int(n), 0.5) + 3.0, dtype=torch.float64, device=DEV)
                        for n in inp["seq"].tolist()])
    k_new = R._aim(qd, lead, d)                                                         # [B, Hkv, D]
    v_new = 3.0 * torch.sign(torch.randn(batch, hkv, d, generator=gen, device=DEV, dtype=torch.float64))
    return inp, k_new, v_new


ONE_LAUNCH_CASES = [("lds", 600, 28, 4, 128, F16, False), ("counter", 3000, 8, 2, 64, BF16, False),
                    ("lds", 1000, 28, 4, 128, BF16, True), ("counter", 2000, 14, 2, 128, F16, True)]


@pytest.mark.parametrize("form,ctx,hq,hkv,d,dtype,norm", ONE_LAUNCH_CASES,
                         ids=[f"{f}-{c}-{a}x{b}-d{d}-{str(t)[6:]}-{'norm' if n else 'rope'}"
                              for f, c, a, b, d, t, n in ONE_LAUNCH_CASES])
def test_decode_attention_one_launch_matches_fp64(form, ctx, hq, hkv, d, dtype, norm):
    """rope (+ the q / k head norm) + KV write + attention in one launch, against fp64 on the pool the launch wrote and
    the two-call form's rotated q, with the spotlight on the new token the launch itself writes."""
    from lite_llama_amd.kernels.attention import decode_attention
    from lite_llama_amd.kernels.norm_act import rope_and_cache

    batch = _batch(form, hq, hkv)
    assert decode_form(ctx, batch, hq, hkv) == form
    inp, k_new, v_new = _new_token_inputs(ctx, batch, hq, hkv, d, dtype, seed=ctx + hq)
    q = inp["q"]
    kv = torch.cat([k_new, v_new], dim=1).to(dtype).contiguous()
    seq, req, table = inp["seq"].long(), inp["req"], inp["table"]
    sel = table[req, seq - 1].contiguous()
    pos = (seq - 1).contiguous()
    cos, sin = _rope_tables(ctx + 8, d, dtype)
    eps = 1e-6
    gen = torch.Generator(device=DEV).manual_seed(7)
    qk_norm = None
    q2, kv2 = q.clone(), kv.clone()
    if norm:
        qw = (1.0 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
        kw = (1.0 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
        qk_norm = (qw, kw, eps)
        q2, _ = K().skip_rmsnorm(q.contiguous(), None, qw, eps)
        kn, _ = K().skip_rmsnorm(kv[:, :hkv].contiguous(), None, kw, eps)
        kv2 = torch.cat([kn, kv[:, hkv:]], dim=1).contiguous()
    pool_one, pool_two = inp["pool"].clone(), inp["pool"].clone()
    got = decode_attention(q, kv, cos, sin, pos, sel, pool_one, inp["scale"], table, req, inp["seq"], ctx,
                           qk_norm=qk_norm)
    assert got is not None
    rope_and_cache(q2, kv2, cos, sin, batch, 1, sel, pool_two, positions=pos)
    assert torch.equal(pool_one.view(torch.int16), pool_two.view(torch.int16))
    ref_inp = dict(inp, q=q2)
    _check_decode(f"decode_attention {form} {str(dtype)[6:]} d{d} {hq}/{hkv} ctx{ctx} {'norm' if norm else 'rope'}",
                  got, ref_inp, pool_one, dtype)


@pytest.mark.parametrize("ctx,batch", [(600, 4), (1025, 0)])
def test_decode_attention_partials_attends_the_new_token_it_writes(ctx, batch):
    """The q|k|v-partials one-launch form writes the new token's K / V row and must attend THAT row: with the new token
    holding most of the weight, a read of the stale pool row costs O(vmax) against the fp64 reference."""
    from lite_llama_amd.kernels.attention import decode_attention_partials
    from lite_llama_amd.kernels.norm_act import PartialSums, rope_and_cache

    hq, hkv, d, dtype = 28, 4, 128, F16
    batch = batch or _batch("walk", hq, hkv)
    assert decode_form(ctx, batch, hq, hkv) == ("lds" if ctx <= 1024 else "walk")
    inp, k_new, v_new = _new_token_inputs(ctx, batch, hq, hkv, d, dtype, seed=ctx)
    x = torch.cat([inp["q"].double().reshape(batch, -1), k_new.reshape(batch, -1), v_new.reshape(batch, -1)], 1).float()
    gen = torch.Generator(device=DEV).manual_seed(3)
    r = torch.randn(x.shape, generator=gen, device=DEV)
    planes = torch.stack([x - r, r]).contiguous()
    row_w = x.shape[1]
    proj = (planes[0] + planes[1]).to(dtype)      # the value the projection would have stored (plane order)
    q2, kv2 = proj[:, : hq * d].reshape(batch, hq, d).clone(), proj[:, hq * d:].reshape(batch, 2 * hkv, d).clone()
    seq, req, table = inp["seq"].long(), inp["req"], inp["table"]
    sel = table[req, seq - 1].contiguous()
    pos = (seq - 1).contiguous()
    cos, sin = _rope_tables(ctx + 8, d, dtype)
    pool_one, pool_two = inp["pool"].clone(), inp["pool"].clone()
    stale = pool_one[sel.long()].clone()
    got = decode_attention_partials(PartialSums(planes, (batch, row_w), dtype), None, hq, hkv, d, cos, sin, pos, sel,
                                    pool_one, inp["scale"], table, req, inp["seq"], ctx)
    assert got is not None
    rope_and_cache(q2, kv2, cos, sin, batch, 1, sel, pool_two, positions=pos)
    assert torch.equal(pool_one.view(torch.int16), pool_two.view(torch.int16))
    assert not torch.equal(stale.view(torch.int16), pool_one[sel.long()].view(torch.int16))
    _check_decode(f"decode_attention_partials ctx{ctx} B{batch} 28/4 d128 new-token spotlight", got,
                  dict(inp, q=q2), pool_one, dtype)


def prefill_form(d, max_len):
    """The prefill form ``flash_attention2_no_pad`` takes (csrc/prefill_attn.hip::launch_fa)."""
    if d in (64, 128):
        return "fa_prefill2_qb2" if max_len > 64 else "fa_prefill2_qb1"
    return "fa_prefill"


SHORT = [64, 128, 129, 65, 1, 127, 63]
QB1 = [64, 33, 1, 17, 63]
LONG = [2048, 4097]
PREFILL_CASES = ([(d, t, SHORT) for d in (32, 64, 128, 256) for t in (F16, BF16)]
                 + [(d, t, QB1) for d in (64, 128) for t in (F16, BF16)]
                 + [(32, F16, LONG), (64, BF16, LONG), (128, F16, LONG), (256, BF16, LONG)])


@pytest.mark.parametrize("d,dtype,lens", PREFILL_CASES,
                         ids=[f"d{d}-{str(t)[6:]}-max{max(ls)}" for d, t, ls in PREFILL_CASES])
def test_flash_attention2_no_pad_regimes_match_fp64(d, dtype, lens):
    hq, hkv = 8, 2
    form = prefill_form(d, max(lens))
    assert form == ("fa_prefill" if d in (32, 256) else "fa_prefill2_qb1" if lens is QB1 else "fa_prefill2_qb2")
    for regime in R.PREFILL_REGIMES:
        inp = R.prefill_inputs(regime, lens, hq, hkv, d, dtype, seed=d + max(lens), device=DEV)

        def run(q, k, v):
            return K().flash_attention2_no_pad(q, k, v, inp["sm_scale"], inp["start"], inp["seq"], max(lens))

        out = run(inp["q"], inp["k"], inp["v"])
        ref, vmax, z, n, idx = R.prefill_ref(inp["q"], inp["k"], inp["v"], inp["sm_scale"], inp["start"], inp["seq"])
        R.assert_within(out[idx], ref, R.bound(ref, vmax, z, n, dtype),
                        f"prefill {form} {str(dtype)[6:]} d{d} {hq}/{hkv} max{max(lens)} {regime}")
        if regime == "poison":
            q, k, v = inp["q"].clone(), inp["k"].clone(), inp["v"].clone()
            for t in (q, k, v):
                t[inp["poisoned"]] = 0
            clean = run(q, k, v)
            assert torch.equal(clean[idx].view(torch.int16), out[idx].view(torch.int16)), "poison leaked"
