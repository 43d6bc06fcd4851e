"""Causal prefill attention over the paged KV pool (csrc/prefill_paged_attn.hip) against a float64 reference: cached
context x chunk length, head geometries, head sizes, fp16 / bf16 / e4m3 pools, contiguous / permuted / shared-prefix
tables, poisoned unnamed rows, the causal future, the ctx = 0 anchor against flash_attention2_no_pad, and refusals."""

import pytest
import torch

from lite_llama_amd import _lib as L
from lite_llama_amd.kernels import flash_attention2_no_pad, prefill_paged_attention
from tests._attn_ref import assert_within, bound, fp8_pool
from tests._paged_ref import paged_inputs, paged_prefill_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(inp, pool=None, kv_scales=(1.0, 1.0), q=None, out=None):
    pool = inp["pool"] if pool is None else pool
    return prefill_paged_attention(inp["q"] if q is None else q, pool, inp["sm_scale"], inp["table"], inp["req"],
                                   inp["start"], inp["q_len"], inp["ctx"], inp["max_q"], inp["max_ctx"], kv_scales,
                                   out=out)


def _check(inp, got, what, wide=None, dtype=None):
    hkv = inp["pool"].shape[1] // 2
    pool = inp["pool"] if wide is None else wide
    ref, vmax, z, n, idx = paged_prefill_ref(inp["q"], pool[:, :hkv], pool[:, hkv:], inp["sm_scale"], inp["table"],
                                             inp["req"], inp["start"], inp["q_len"], inp["ctx"])
    assert_within(got[idx], ref, bound(ref, vmax, z, n, dtype or inp["q"].dtype), what)


def _written(inp):
    """Rows of q / out the kernel writes: each sequence's new tokens."""
    return torch.cat([torch.arange(int(s), int(s) + int(n), device=DEV) for s, n in zip(inp["start"], inp["q_len"])])


def _seqs(ctx, chunk):
    # ragged: a full chunk, a shorter one over a shorter context, and a sequence with nothing new
    return [(ctx, chunk), (ctx // 3, max(chunk // 2, 1)), (ctx, 0)]


@pytest.mark.parametrize("ctx", [0, 1, 63, 64, 65, 128, 1000, 4097])
@pytest.mark.parametrize("chunk", [1, 16, 17, 64, 65, 129, 300])
def test_paged_prefill_ctx_by_chunk(ctx, chunk):
    inp = paged_inputs(_seqs(ctx, chunk), 28, 4, 128, torch.float16, seed=ctx * 1000 + chunk, table_kind="permuted",
                       device=DEV)
    _check(inp, _run(inp), f"ctx {ctx} chunk {chunk}")


@pytest.mark.parametrize("hq,hkv", [(8, 2), (28, 4), (32, 8), (16, 16)])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_paged_prefill_geometry(hq, hkv, d, dtype):
    inp = paged_inputs([(65, 129), (0, 17), (200, 1), (7, 0)], hq, hkv, d, dtype, seed=hq * 7 + d, device=DEV)
    _check(inp, _run(inp), f"{hq}/{hkv} d{d} {dtype}")


@pytest.mark.parametrize("kind", ["contiguous", "permuted", "shared"])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_prefill_tables(kind, d):
    inp = paged_inputs([(300, 70), (300, 70), (150, 33)], 16, 4, d, torch.bfloat16, seed=3, table_kind=kind,
                       device=DEV)
    _check(inp, _run(inp), f"{kind} table d{d}")


def test_shared_prefix_identical_queries_bit_identical():
    inp = paged_inputs([(257, 90), (257, 90)], 28, 4, 128, torch.float16, seed=5, table_kind="shared", device=DEV)
    # sequence 1's new tokens: the same queries and the same K / V contents (in its own rows) as sequence 0's
    t, hkv = inp["table"], 4
    inp["pool"][t[1, 257:347].long()] = inp["pool"][t[0, 257:347].long()]
    s0, s1 = (int(v) for v in inp["start"])
    inp["q"][s1:s1 + 90] = inp["q"][s0:s0 + 90]
    got = _run(inp)
    assert torch.equal(got[s0:s0 + 90], got[s1:s1 + 90])
    _check(inp, got, "shared prefix")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", [32, 128])
def test_unnamed_rows_never_reach_the_output(dtype, d):
    inp = paged_inputs([(130, 65), (0, 40), (1000, 3)], 8, 2, d, dtype, seed=11, table_kind="permuted", device=DEV)
    poisoned = _run(inp)
    clean = inp["pool"].clone()
    clean[inp["unnamed"]] = 0
    w = _written(inp)
    assert torch.equal(poisoned[w], _run(inp, pool=clean)[w])
    _check(inp, poisoned, "poisoned pool")


def test_causal_future_does_not_change_a_query():
    inp = paged_inputs([(100, 129)], 28, 4, 128, torch.float16, seed=13, device=DEV)
    before = _run(inp)
    j0 = 50  # rewrite every row named after position ctx + j0
    pool = inp["pool"].clone()
    future = inp["table"][0, 100 + j0 + 1:100 + 129].long()
    pool[future] = torch.randn_like(pool[future].float()).to(pool.dtype) * 3
    after = _run(inp, pool=pool)
    assert torch.equal(before[: j0 + 1], after[: j0 + 1])
    assert not torch.equal(before[j0 + 1:129], after[j0 + 1:129])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_ctx0_identity_table_matches_flash_attention_nopad(dtype, d):
    hq, hkv = 16, 4
    inp = paged_inputs([(0, 300), (0, 65), (0, 1)], hq, hkv, d, dtype, seed=17, table_kind="contiguous", device=DEV)
    # an identity layout: the sequences' rows of q and of the pool coincide (start = first pool row of the sequence)
    starts = [int(v) for v in inp["table"][:, 0]]
    pool = inp["pool"]
    q = torch.full((pool.shape[0], hq, d), float("nan"), dtype=dtype, device=DEV)
    for b, n in enumerate(inp["q_len"].tolist()):
        s = int(inp["start"][b])
        q[starts[b]:starts[b] + n] = inp["q"][s:s + n]
    inp = dict(inp, q=q, start=torch.tensor(starts, dtype=torch.int32, device=DEV))
    got = _run(inp)
    fa = flash_attention2_no_pad(q, pool[:, :hkv], pool[:, hkv:], inp["sm_scale"], inp["start"], inp["q_len"], 300)
    ref, vmax, z, n, idx = paged_prefill_ref(q, pool[:, :hkv], pool[:, hkv:], inp["sm_scale"], inp["table"],
                                             inp["req"], inp["start"], inp["q_len"], inp["ctx"])
    tol = bound(ref, vmax, z, n, dtype)
    assert_within(got[idx], fa[idx].double(), tol, f"ctx 0 vs flash_attention2_no_pad d{d}")
    assert_within(got[idx], ref, tol, f"ctx 0 vs reference d{d}")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("ctx,chunk", [(0, 64), (65, 17), (1000, 300), (4097, 1)])
def test_fp8_pool_on_widened_values(d, ctx, chunk):
    ks, vs = 0.02, 0.01
    inp = paged_inputs(_seqs(ctx, chunk), 32, 8, d, torch.float16, seed=ctx + d, table_kind="permuted", device=DEV)
    codes, wide = fp8_pool(inp["pool"], ks, vs, 8)
    got = _run(inp, pool=codes, kv_scales=(ks, vs))
    _check(inp, got, f"e4m3 pool d{d} ctx {ctx} chunk {chunk}", wide=wide, dtype=torch.float16)
    # uint8 views of the same codes give the same bits
    w = _written(inp)
    assert torch.equal(got[w], _run(inp, pool=codes.view(torch.uint8), kv_scales=(ks, vs))[w])


def test_int64_index_vectors():
    inp = paged_inputs([(70, 65), (3, 5)], 8, 2, 64, torch.float16, seed=19, device=DEV)
    got32 = _run(inp)
    inp64 = dict(inp, **{k: inp[k].long() for k in ("req", "start", "q_len", "ctx")})
    assert torch.equal(got32[inp["start"][0]:inp["start"][0] + 65], _run(inp64)[inp["start"][0]:inp["start"][0] + 65])


def test_rows_past_the_chunk_are_not_written():
    inp = paged_inputs([(40, 20), (10, 0)], 8, 2, 128, torch.float16, seed=23, device=DEV)
    out = torch.full_like(inp["q"], 7.0)
    _run(inp, out=out)
    s = int(inp["start"][0])
    written = torch.zeros(out.shape[0], dtype=torch.bool, device=DEV)
    written[s:s + 20] = True
    assert bool((out[~written] == 7.0).all())
    assert bool(torch.isfinite(out[written]).all())


def _raw(inp, out, q, pool, d, dtype_code, kv_code, q_st=None, kv_scales=(1.0, 1.0)):
    hkv = pool.shape[1] // 2
    k, v = pool[:, :hkv], pool[:, hkv:]
    return L.lib().ll_prefill_paged_attention(
        out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), inp["table"].data_ptr(), inp["req"].data_ptr(),
        inp["start"].data_ptr(), inp["q_len"].data_ptr(), inp["ctx"].data_ptr(), 2, q.shape[1], hkv, d, inp["max_q"],
        inp["max_ctx"], inp["sm_scale"], kv_scales[0], kv_scales[1], q.stride(0) if q_st is None else q_st, q.stride(1),
        k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1), inp["table"].stride(0),
        dtype_code, kv_code, 0, 0, 0, 0, L.stream_ptr())


def test_refusals_return_errors_and_never_write():
    inp = paged_inputs([(40, 20), (10, 5)], 8, 2, 64, torch.float16, seed=29, device=DEV)
    q, pool = inp["q"], inp["pool"]
    out = torch.full_like(q, 7.0)
    cases = [
        (dict(dtype_code=L.LL_F32, kv_code=L.LL_F32), -1),                     # fp32 queries
        (dict(dtype_code=L.LL_F16, kv_code=L.LL_BF16), -1),                    # pool dtype != query dtype
        (dict(dtype_code=L.LL_BF16, kv_code=L.LL_FP8E4M3), -1),                # e4m3 pool needs fp16 queries
        (dict(dtype_code=L.LL_F16, kv_code=L.LL_F16, q_st=q.stride(0) + 4), -3),  # misaligned row stride
        (dict(dtype_code=L.LL_F16, kv_code=L.LL_FP8E4M3, kv_scales=(0.0, 1.0)), -3),  # non-positive scale
    ]
    for kw, code in cases:
        assert _raw(inp, out, q, pool, 64, **kw) == code, kw
    # head sizes not served: 96 (16-bit), 32 and 256 (e4m3)
    q96 = torch.zeros(q.shape[0], 8, 96, dtype=torch.float16, device=DEV)
    p96 = torch.zeros(pool.shape[0], 4, 96, dtype=torch.float16, device=DEV)
    out96 = torch.full_like(q96, 7.0)
    assert _raw(inp, out96, q96, p96, 96, L.LL_F16, L.LL_F16) == -2
    p32 = torch.zeros(pool.shape[0], 4, 32, dtype=torch.uint8, device=DEV)
    q32 = torch.zeros(q.shape[0], 8, 32, dtype=torch.float16, device=DEV)
    out32 = torch.full_like(q32, 7.0)
    assert _raw(inp, out32, q32, p32, 32, L.LL_F16, L.LL_FP8E4M3) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out96 == 7.0).all()) and bool((out32 == 7.0).all())
    with pytest.raises(L.KernelError):
        prefill_paged_attention(q.float(), pool.float(), inp["sm_scale"], inp["table"], inp["req"], inp["start"],
                                inp["q_len"], inp["ctx"], inp["max_q"], inp["max_ctx"])
