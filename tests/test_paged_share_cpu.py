"""CPU tier of the shared paged pool: the header declares and the library exports ll_kv_paged_fork and
ll_kv_paged_release_shared; the reference model (tests/_paged_share_ref.py) keeps its invariants over a random
admit / fork / append / release sequence and reduces to oracle.kv_paged.PagedPoolModel when nothing is forked; the
argument refusals that are raised before any device call."""

import os
import re

import numpy as np
import pytest
import torch

from oracle.kv_paged import PagedPoolModel
from tests._paged_share_ref import RandomOps, SharedPagedPoolModel, check_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries():
    from lite_llama_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lite_llama_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(ll_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in ("ll_kv_paged_fork", "ll_kv_paged_release_shared"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the argument lists of the declarations, counted: the ctypes table passes as many
    for name in ("ll_kv_paged_fork", "ll_kv_paged_release_shared"):
        args = re.search(name + r"\s*\(([^;]*)\)\s*;", header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name]), name
    # shape errors are answered on the host, before any launch: too many forks, pool rows that are not 16-byte words
    def fork(n, row_bytes):
        return lib.ll_kv_paged_fork(None, None, None, 4, None, None, None, None, None, None, n, 16, None, 8, None, 1, row_bytes,
                                    4, None)

    assert fork(1025, 64) == -2 and fork(1, 24) == -2
    assert fork(1, 64) == -3                                                                # null pointers
    assert fork(0, 64) == 0
    assert lib.ll_kv_paged_release_shared(None, None, None, 4, None, None, None, None, 1025, 4, None) == -2
    assert lib.ll_kv_paged_release_shared(None, None, None, 4, None, None, None, None, 0, 4, None) == 0


@pytest.mark.parametrize("bs,seed", [(1, 0), (8, 1), (64, 2)])
def test_model_keeps_its_invariants_over_a_random_sequence(bs, seed):
    max_req, max_len, nb = 16, 5 * bs + 3, 70
    m = SharedPagedPoolModel(nb, bs, max_req, max_len)
    ops = RandomOps(seed, bs, max_req, max_len)
    seen = {"fork": 0, "release": 0, "shared_release": 0, "chain": 0}
    children = set()
    for _ in range(400):
        op, a = ops.next()
        if op == "admit":
            m.extend(a[0], a[1], a[2], 0)
            ops.admitted(a[0], a[1], m.req_blocks)
        elif op == "fork":
            err = m.err
            if m.fork(*a):
                ops.forked(a[1], a[2])
                seen["fork"] += 1
                seen["chain"] += any(s in children for s in a[0])
                children.update(a[1])
                for s, d, ln in zip(*a):       # the child's rows: the source's over full blocks, its own after them
                    full = ln // bs * bs
                    assert np.array_equal(m.token_table[d, :full], m.token_table[s, :full])
                    assert not set(m.token_table[d, full:ln].tolist()) & set(m.token_table[s, :ln].tolist())
                assert len(m.copies) == sum(1 for ln in a[2] if ln % bs)
            else:
                assert m.err != err or m.err & 1
        elif op == "append":
            m.extend(a[0], a[1], 1, 1)
            ops.appended(a[0], a[1], m.req_blocks)
            for r, n in zip(*a):               # the block an append writes has no other holder
                if int(m.req_blocks[r]) * bs >= n:
                    assert m.share[m.block_table[r, (n - 1) // bs]] == 0
        elif op == "release":
            seen["shared_release"] += int(sum(m.share[m.block_table[r, j]] > 0 for r in a[0] for j in range(m.req_blocks[r])))
            m.release(a[0])
            ops.released(a[0])
            children.difference_update(a[0])
            seen["release"] += 1
        check_model(m)
    assert seen["fork"] >= 10 and seen["release"] >= 10 and seen["shared_release"] >= 5 and seen["chain"] >= 1, seen


def test_model_without_forks_is_the_plain_pool_model():
    bs, max_req, max_len, nb = 8, 12, 70, 60
    a, b = SharedPagedPoolModel(nb, bs, max_req, max_len), PagedPoolModel(nb, bs, max_req, max_len)
    rng = np.random.default_rng(3)
    live, lens = set(), np.zeros(max_req, dtype=np.int64)
    for _ in range(200):
        op = rng.integers(0, 10)
        idle = [r for r in range(max_req) if r not in live]
        if op < 3 and idle:
            reqs = [int(r) for r in rng.choice(idle, int(rng.integers(1, min(4, len(idle)) + 1)), replace=False)]
            ln = [int(rng.integers(1, 30)) for _ in reqs]
            assert np.array_equal(a.extend(reqs, ln, max(ln), 0), b.extend(reqs, ln, max(ln), 0))
            for r, n in zip(reqs, ln):
                if b.req_blocks[r] * bs >= n:
                    live.add(r)
                    lens[r] = n
        elif op < 8 and live:
            reqs = [r for r in sorted(live) if lens[r] + 1 <= max_len]
            new = [int(lens[r] + 1) for r in reqs]
            assert np.array_equal(a.extend(reqs, new, 1, 1), b.extend(reqs, new, 1, 1))
            for r, n in zip(reqs, new):
                if b.req_blocks[r] * bs >= n:
                    lens[r] = n
        elif live:
            reqs = [int(r) for r in rng.choice(sorted(live), int(rng.integers(1, min(3, len(live)) + 1)), replace=False)]
            a.release(reqs)
            b.release(reqs)
            for r in reqs:
                live.discard(r)
        assert a.free == b.free and a.err == b.err and a.stack[: a.free] == b.stack[: b.free]
        assert np.array_equal(a.req_blocks, b.req_blocks) and np.array_equal(a.token_table, b.token_table)
        assert not a.share.any()


def test_model_fork_refusals_change_nothing():
    m = SharedPagedPoolModel(6, 4, 6, 24)           # 5 usable blocks
    m.extend([0], [10], 10, 0)                      # 3 blocks, 2 free
    before = (m.free, list(m.stack), m.req_blocks.copy(), m.block_table.copy(), m.share.copy(), m.token_table.copy())

    def unchanged():
        return (m.free == before[0] and m.stack == before[1] and np.array_equal(m.req_blocks, before[2])
                and np.array_equal(m.block_table, before[3]) and np.array_equal(m.share, before[4])
                and np.array_equal(m.token_table, before[5]))

    assert not m.fork([0, 0, 0], [1, 2, 3], [10, 9, 7]) and m.err == 1 and unchanged()     # three partial blocks, two free
    m.err = 0
    assert not m.fork([0], [1], [13]) and m.err == 4 and unchanged()                        # beyond the source's blocks
    m.err = 0
    assert not m.fork([0, 0], [1, 0], [8, 8]) and m.err == 4 and unchanged()                # a child that holds blocks
    m.err = 0
    assert not m.fork([0], [1], [0]) and m.err == 4 and unchanged()
    m.err = 0
    assert not m.fork([0, 0], [1, 1], [8, 8]) and m.err == 4 and unchanged()                # a child listed twice
    m.err = 0
    assert not m.fork([0, 1], [1, 2], [8, 8]) and m.err == 4 and unchanged()                # a child that is a source
    m.err = 0
    assert m.fork([0, 0], [1, 2], [10, 8]) and m.err == 0 and m.free == 1
    assert m.share.tolist() == [2, 2, 0, 0, 0, 0] and m.copies == [(2, 3, 2)]
    m.release([0, 1, 2])                             # all holders in one call: the last one pushes, at its place
    assert m.free == 5 and m.stack[:5] == [4, 2, 3, 0, 1] and not m.share.any()
    check_model(m)


def _bare_engine(paged, share, max_batch=4):
    """A DecodeEngine with only the attributes prefill's argument checks read: they are raised before any device call."""
    from lite_llama_amd.executor import DecodeEngine

    eng = object.__new__(DecodeEngine)
    eng.paged, eng.share_blocks, eng.max_batch, eng.device = paged, share, max_batch, "cpu"
    return eng


def test_engine_refusals_before_any_device_call():
    from lite_llama_amd.executor import DecodeEngine
    from lite_llama_amd.executor.paged_kv import PagedKVPool

    with pytest.raises(ValueError, match="kv_share_blocks needs kv_block_size"):
        DecodeEngine(None, max_batch=2, max_seq_len=32, kv_share_blocks=True)
    ids = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_samples needs kv_share_blocks"):
        _bare_engine(True, False).prefill(ids, num_samples=2)
    with pytest.raises(ValueError, match="num_samples needs kv_share_blocks"):
        _bare_engine(False, False).prefill(ids, num_samples=2)
    with pytest.raises(ValueError, match="max_batch"):
        _bare_engine(True, True, max_batch=5).prefill(ids, num_samples=3)
    with pytest.raises(ValueError, match="max_batch"):
        _bare_engine(True, True).prefill(ids, num_samples=0)
    with pytest.raises(ValueError, match="cannot be combined with shared_prefix_ids"):
        _bare_engine(True, True).prefill(ids, num_samples=2, shared_prefix_ids=torch.zeros(4, dtype=torch.int64))
    eng = _bare_engine(True, False)
    eng.info = type("Info", (), {})()
    with pytest.raises(ValueError, match="bump pool"):
        eng.prefill(ids, shared_prefix_ids=torch.zeros(4, dtype=torch.int64))
    # a pool without share counts has no fork
    pool = object.__new__(PagedKVPool)
    pool.share_blocks = False
    with pytest.raises(ValueError, match="share_blocks=True"):
        pool.fork(None, None, None, None)
