"""Host side of the shared-prefix decode route (no GPU): the split / workspace arithmetic of the C planner (host code,
called through ctypes like ll_flash_decoding_num_partitions; without a device it plans for 256 CUs), the wrapper's
argument validation, the routing predicate and the AttentionMetadata defaults."""

import inspect
import types

import pytest
import torch

from lite_llama_amd import _lib, build


def _lib_handle():
    build.build(verbose=False)
    return _lib.lib()


def _plan(batch, hq, hkv, prefix, cus=256):
    """Restatement of csrc/shared_prefix_attn.hip::sp_plan: (splits, keys per split)."""
    qtiles = -(-batch * (hq // hkv) // 64)
    tiles = -(-prefix // 64)
    want = max(1, min(-(-cus // (hkv * qtiles)), tiles, 64))
    per = -(-tiles // want)
    return -(-tiles // per), per * 64


@pytest.mark.parametrize("batch,hq,hkv,d", [(64, 28, 4, 128), (16, 28, 4, 128), (1, 16, 1, 64), (100, 7, 1, 128), (3, 8, 8, 64),
                                            (1, 1, 1, 64), (256, 32, 2, 128)])
@pytest.mark.parametrize("prefix", [64, 65, 127, 128, 200, 1000, 2048, 4100, 100000])
def test_split_and_workspace_arithmetic(batch, hq, hkv, d, prefix):
    lib = _lib_handle()
    max_len = prefix + 300
    splits = lib.ll_shared_prefix_num_splits(batch, hq, hkv, d, prefix, max_len)
    want, keys = _plan(batch, hq, hkv, prefix)
    assert splits == want
    assert 1 <= splits <= 64 and keys % 64 == 0 and keys >= 64            # never below one 64-key tile
    assert (splits - 1) * keys < prefix <= splits * keys                   # every split holds keys, together all of them
    # the launch fills the CUs where the prefix allows: fewer splits only when the query tiles alone fill them, the prefix
    # has no more key tiles, or regrouping the tiles evenly needs fewer
    base = hkv * -(-batch * (hq // hkv) // 64)
    assert splits <= max(1, -(-256 // base)) and (splits > 1 or base >= 256 or prefix <= 64 or -(-256 // base) == 1)
    # workspace: prefix records, suffix records (partitions of max_len - prefix), the suffix lengths; 4-float aligned parts
    rows, nparts = batch * hq, -(-(max_len - prefix) // 128)
    al = lambda n: -(-n // 4) * 4  # noqa: E731
    floats = rows * splits * d + al(rows * splits) + rows * nparts * d + al(rows * nparts) + al(batch)
    assert lib.ll_shared_prefix_workspace_floats(batch, hq, hkv, d, prefix, max_len) == floats
    assert lib.ll_shared_prefix_workspace_floats(batch, hq, hkv, d, prefix, prefix) == \
        rows * splits * d + al(rows * splits) + al(batch)                 # no tail partitions at all


def test_headline_plan():
    lib = _lib_handle()
    # batch 64 x 7 heads per KV head = 448 query rows = 7 tiles, x 4 KV heads = 28 workgroups per split
    assert lib.ll_shared_prefix_num_splits(64, 28, 4, 128, 2048, 2176) == 8      # 32 key tiles in splits of 4: 224 workgroups
    assert lib.ll_shared_prefix_num_splits(64, 28, 4, 128, 128, 256) == 2
    assert lib.ll_shared_prefix_num_splits(1, 1, 1, 64, 4100, 4200) == 33        # 65 key tiles, two per split


@pytest.mark.parametrize("args", [
    (4, 8, 2, 32, 100, 200),      # head size
    (4, 8, 2, 256, 100, 200),
    (4, 8, 2, 128, 63, 200),      # below one key tile
    (4, 8, 2, 128, 100, 99),      # max_len below the prefix
    (4, 34, 2, 128, 100, 200),    # 17 query heads per KV head
    (4, 7, 2, 128, 100, 200),     # ragged groups
])
def test_unserved_shapes_size_to_zero(args):
    lib = _lib_handle()
    assert lib.ll_shared_prefix_num_splits(*args) == 0
    assert lib.ll_shared_prefix_workspace_floats(*args) == 0


def _cpu_args(b=2, hq=4, hkv=2, d=64, rows=300, width=256):
    q = torch.zeros(b, hq, d, dtype=torch.float16)
    pool = torch.zeros(rows, 2 * hkv, d, dtype=torch.float16)
    table = torch.zeros(b, width, dtype=torch.int32)
    idx = torch.arange(b, dtype=torch.int32)
    seq = torch.full((b,), 200, dtype=torch.int32)
    return q, pool[:, :hkv], pool[:, hkv:], 0.125, table, idx, seq, 200


def test_wrapper_validates_before_anything_launches():
    from lite_llama_amd.kernels import shared_prefix_decode_attention as f

    q, k, v, sc, table, idx, seq, top = _cpu_args()
    with pytest.raises(ValueError, match="int32"):
        f(q, k, v, sc, table.long(), idx, seq, top, 100)
    with pytest.raises(ValueError, match="one entry per row"):
        f(q, k, v, sc, table, idx[:1], seq, top, 100)
    with pytest.raises(ValueError, match="not a row of the token table"):
        f(q, k, v, sc, table, idx, seq, top, 100, prefix_req=2)
    with pytest.raises(ValueError, match="exceeds the table row"):
        f(q, k, v, sc, table, idx, seq, 400, 300)
    with pytest.raises(ValueError, match="views of one pool"):
        f(q, k, v[:, :, :32], sc, table, idx, seq, top, 100)
    with pytest.raises(ValueError, match="multiple of the KV heads"):
        f(q[:, :3], k, v, sc, table, idx, seq, top, 100)
    with pytest.raises(ValueError, match=r"q \[B, Hq, D\]"):
        f(q[0], k, v, sc, table, idx, seq, top, 100)
    # well-formed arguments on the CPU: the product path fails loudly, there is no fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        f(q, k, v, sc, table, idx, seq, top, 100)


def test_supported_predicate_and_threshold_constant():
    from lite_llama_amd.kernels import attention as A

    ok = A.shared_prefix_supported
    f16, bf16 = torch.float16, torch.bfloat16
    assert ok(f16, f16, 28, 4, 128, 2048, 2176) and ok(bf16, bf16, 7, 1, 64, 64, 64) and ok(f16, f16, 16, 1, 128, 64, 65)
    assert not ok(f16, torch.float8_e4m3fn, 28, 4, 128, 2048, 2176)       # e4m3 pool
    assert not ok(f16, bf16, 28, 4, 128, 2048, 2176)
    assert not ok(torch.float32, torch.float32, 28, 4, 128, 2048, 2176)
    assert not ok(f16, f16, 28, 4, 32, 2048, 2176) and not ok(f16, f16, 28, 4, 256, 2048, 2176)
    assert not ok(f16, f16, 34, 2, 128, 2048, 2176)
    assert not ok(f16, f16, 28, 4, 128, 63, 2176) and not ok(f16, f16, 28, 4, 128, 2048, 2047)
    assert isinstance(A.SHARED_PREFIX_MIN_LEN, int) and A.SHARED_PREFIX_MIN_LEN >= 64


def test_metadata_defaults_and_routing_predicate(monkeypatch):
    from lite_llama_amd.executor import AttentionMetadata, DecodeEngine
    from lite_llama_amd.kernels import attention as A
    from lite_llama_amd.model import shared_prefix_route

    info = AttentionMetadata()
    assert info.shared_prefix_len == 0 and info.shared_prefix_req == 0 and info.b_ctx_len is None
    assert "shared_prefix_ids" in inspect.signature(DecodeEngine.prefill).parameters
    assert inspect.signature(DecodeEngine.prefill).parameters["shared_prefix_ids"].default is None
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 512)
    assert not shared_prefix_route(info, False)                          # unset: nothing changes
    legacy = types.SimpleNamespace(max_actual_seq_len=4096)             # metadata objects without the new fields
    assert not shared_prefix_route(legacy, False)
    info.shared_prefix_len, info.max_actual_seq_len = 512, 600
    assert shared_prefix_route(info, False)
    assert not shared_prefix_route(info, True)                           # prefill steps are untouched
    info.b_ctx_len = torch.zeros(1, dtype=torch.int32)
    assert not shared_prefix_route(info, False)                          # chunk steps are untouched
    info.b_ctx_len = None
    info.shared_prefix_len = 511
    assert not shared_prefix_route(info, False)                          # below the threshold: the old route
    monkeypatch.setattr(A, "SHARED_PREFIX_MIN_LEN", 1)
    info.shared_prefix_len = 63
    assert not shared_prefix_route(info, False)                          # never below one key tile
