"""kernels.shared_prefix_decode_attention against the float64 decode reference over the same aliased table
(tests/_attn_ref.py: ``decode_ref`` and the derived ``bound``): every decode regime, prefix lengths on the tile and split
boundaries, ragged tails (an empty one, a one-token one, one that crosses a suffix partition), GQA groups 1 .. 16, a
tensor-parallel shard geometry, int64 index vectors, refusals and graph capture."""

import pytest
import torch

import lite_llama_amd._lib as L
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16


def K():
    import lite_llama_amd.kernels as k

    return k


def _lens(prefix, batch, seed):
    """Ragged tails of 1 .. 300 tokens: row 0 (the prefix row) has an empty tail, row 1 one token, row 2 crosses a
    128-token suffix partition, the last row has the longest tail."""
    g = torch.Generator().manual_seed(seed)
    lens = (prefix + torch.randint(1, 301, (batch,), generator=g)).tolist()
    if batch == 1:
        return [prefix + 150]
    lens[0] = prefix
    lens[1] = prefix + 1
    if batch > 2:
        lens[2] = prefix + 200
    if batch > 3:
        lens[-1] = prefix + 300
    return lens


def _inputs(regime, prefix, batch, hq, hkv, d, dtype, seed, prefix_row=0):
    """``decode_inputs`` with every table row's first ``prefix`` entries aliased to those of batch row ``prefix_row``."""
    inp = R.decode_inputs(regime, _lens(prefix, batch, seed), hq, hkv, d, dtype, seed, device=DEV)
    pr = int(inp["req"][prefix_row])
    inp["table"][:, :prefix] = inp["table"][pr, :prefix].clone()
    inp["prefix_req"] = pr
    return inp


def _run(inp, pool, prefix, **kw):
    hkv = inp["hkv"]
    max_len = kw.pop("max_len", None)
    if max_len is None:
        max_len = int(inp["seq"].max())
    return K().shared_prefix_decode_attention(inp["q"], pool[:, :hkv], pool[:, hkv:], inp["scale"], inp["table"],
                                              kw.pop("req", inp["req"]), kw.pop("seq", inp["seq"]), max_len, prefix,
                                              inp["prefix_req"], **kw)


def _check(name, out, inp, pool, dtype):
    hkv = inp["hkv"]
    ref, vmax, z, n = R.decode_ref(inp["q"], pool[:, :hkv], pool[:, hkv:], inp["scale"], inp["table"], inp["req"],
                                   inp["seq"])
    return R.assert_within(out, ref, R.bound(ref, vmax, z, n, dtype), name)


# (hq, hkv, head dim, dtype, batch, prefix): GQA groups 1, 4, 7, 8, 16; both head sizes and dtypes; batch 1, 3 (does not
# fill a 64-row tile), 64 and 100 (groups 7 / 4 / 16: tiles straddle batch rows inside a KV head's group); hq 7 / hkv 1 is a
# tensor-parallel shard of the headline geometry; prefix 4100 takes several splits at every batch
CASES = [
    (28, 4, 128, F16, 64, 200),
    (28, 4, 128, F16, 64, 1000),
    (28, 4, 128, F16, 16, 4100),
    (7, 1, 128, F16, 64, 128),
    (7, 1, 128, BF16, 64, 65),
    (8, 8, 64, F16, 3, 64),
    (8, 8, 64, BF16, 3, 127),
    (8, 2, 64, BF16, 100, 200),
    (8, 1, 128, BF16, 3, 1000),
    (16, 1, 64, F16, 1, 4100),
    (16, 1, 128, F16, 100, 65),
    (4, 4, 128, F16, 100, 127),
    (8, 2, 64, F16, 64, 1000),
    (16, 1, 64, BF16, 3, 128),
    (7, 1, 64, BF16, 100, 64),
]


@pytest.mark.parametrize("regime", R.DECODE_REGIMES)
@pytest.mark.parametrize("hq,hkv,d,dtype,batch,prefix", CASES,
                         ids=[f"h{c[0]}kv{c[1]}d{c[2]}-{'f16' if c[3] == F16 else 'bf16'}-b{c[4]}-p{c[5]}" for c in CASES])
def test_shared_prefix_decode_against_fp64(regime, hq, hkv, d, dtype, batch, prefix):
    inp = _inputs(regime, prefix, batch, hq, hkv, d, dtype, seed=prefix + batch)
    splits = L.lib().ll_shared_prefix_num_splits(batch, hq, hkv, d, prefix, int(inp["seq"].max()))
    assert splits >= 1 and (prefix < 4100 or splits > 1)
    out = _run(inp, inp["pool"], prefix)
    assert out is not None
    clean = R.clean_pool(inp)
    if regime == "poison":
        # rows the table does not name for a sequence -- the prefix row's own positions >= prefix included -- never
        # reach the output
        assert torch.equal(out, _run(inp, clean, prefix))
    _check(f"shared_prefix {regime} {hq}/{hkv} d{d} b{batch} p{prefix} splits{splits}", out, inp, clean, dtype)


@pytest.mark.parametrize("regime", ["wide", "spotlight", "ramp"])
@pytest.mark.parametrize("prefix", [200, 1000])
def test_agrees_with_flash_decoding_within_the_bound(regime, prefix):
    hq, hkv, d = 28, 4, 128
    inp = _inputs(regime, prefix, 9, hq, hkv, d, F16, seed=11)
    pool = R.clean_pool(inp)
    out = _run(inp, pool, prefix)
    old = K().flash_decoding(inp["q"], pool[:, :hkv], pool[:, hkv:], inp["scale"], inp["table"], inp["req"], inp["seq"],
                             int(inp["seq"].max()))
    _check(f"shared {regime} p{prefix}", out, inp, pool, F16)
    _check(f"flash_decoding {regime} p{prefix}", old, inp, pool, F16)


def test_int64_indices_other_prefix_row_and_larger_max_len():
    hq, hkv, d, prefix = 8, 2, 128, 200
    inp = _inputs("wide", prefix, 5, hq, hkv, d, F16, seed=5, prefix_row=3)
    if inp["prefix_req"] == 0:   # the prefix must not sit in table row 0 here
        inp = _inputs("wide", prefix, 5, hq, hkv, d, F16, seed=5, prefix_row=2)
    assert inp["prefix_req"] != 0
    row = inp["table"][inp["prefix_req"], :prefix]
    assert not bool((row[1:] > row[:-1]).all())          # a scattered (non-monotone) prefix table row
    pool = R.clean_pool(inp)
    base = _run(inp, pool, prefix)
    _check("prefix_req != 0", base, inp, pool, F16)
    wide = _run(inp, pool, prefix, req=inp["req"].long(), seq=inp["seq"].long())
    assert torch.equal(wide, base)
    # a bucketed max_len (the engine's graph capture): more suffix partitions launched, the same values
    bucket = (int(inp["seq"].max()) + 127) // 128 * 128 + 256
    assert torch.equal(_run(inp, pool, prefix, max_len=bucket), base)


def test_strided_pool_view_and_preallocated_out():
    hq, hkv, d, prefix = 7, 1, 64, 130
    inp = _inputs("offset", prefix, 10, hq, hkv, d, BF16, seed=8)
    pool = R.clean_pool(inp)
    big = torch.zeros(pool.shape[0], 2 * hkv + 3, d, dtype=pool.dtype, device=DEV)
    big[:, 1:1 + 2 * hkv] = pool
    view = big[:, 1:1 + 2 * hkv]
    assert not view.is_contiguous()
    out = torch.full_like(inp["q"], 7.0)
    got = _run(inp, view, prefix, out=out)
    assert got is out
    _check("strided pool", out, inp, pool, BF16)
    assert torch.equal(out, _run(inp, pool, prefix))


def test_refusals_leave_out_untouched():
    hq, hkv, d, prefix = 8, 2, 128, 100
    inp = _inputs("wide", prefix, 4, hq, hkv, d, F16, seed=2)
    pool = R.clean_pool(inp)
    sentinel = 123.0
    out = torch.full_like(inp["q"], sentinel)
    # e4m3 pool
    codes, _ = R.fp8_pool(pool, 1.0, 1.0, hkv)
    assert _run(inp, codes, prefix, out=out) is None
    # prefix below one key tile, max_len below the prefix
    assert _run(inp, pool, 63, out=out) is None
    assert _run(inp, pool, prefix, max_len=prefix - 1, out=out) is None
    # head size 32
    inp32 = _inputs("wide", prefix, 4, 8, 2, 32, F16, seed=2)
    out32 = torch.full_like(inp32["q"], sentinel)
    assert _run(inp32, R.clean_pool(inp32), prefix, out=out32) is None
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((out32 == sentinel).all())
    # the C entry itself: LL_ERR_SHAPE (-2), nothing written
    lib = L.lib()
    k, v = pool[:, :hkv], pool[:, hkv:]
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)

    def entry(q, k, v, p, max_len, dt, dd):
        return lib.ll_shared_prefix_decode_attention(
            out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), inp["table"].data_ptr(), inp["req"].data_ptr(),
            inp["seq"].data_ptr(), inp["prefix_req"], p, ws.data_ptr(), 4, hq, hkv, dd, max_len, inp["scale"], q.stride(0),
            q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
            inp["table"].stride(0), dt, L.LL_I32, L.LL_I32, L.stream_ptr())

    top = int(inp["seq"].max())
    assert entry(inp["q"], k, v, 63, top, L.LL_F16, d) == -2
    assert entry(inp["q"], k, v, prefix, prefix - 1, L.LL_F16, d) == -2
    assert entry(inp["q"], k, v, prefix, top, L.LL_FP8E4M3, d) == -2
    assert entry(inp["q"], k, v, prefix, top, L.LL_F16, 32) == -2
    assert lib.ll_shared_prefix_workspace_floats(4, hq, hkv, d, 63, top) == 0
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


def test_capture_replays_bit_identical():
    hq, hkv, d, prefix = 28, 4, 128, 1000
    inp = _inputs("wide", prefix, 16, hq, hkv, d, F16, seed=4)
    pool = R.clean_pool(inp)
    top = int(inp["seq"].max())          # read here: nothing on the host may touch the lengths inside the capture
    eager = _run(inp, pool, prefix, max_len=top).clone()
    out = torch.zeros_like(inp["q"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(inp, pool, prefix, out=out, max_len=top)   # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(inp, pool, prefix, out=out, max_len=top)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check("captured", out, inp, pool, F16)
