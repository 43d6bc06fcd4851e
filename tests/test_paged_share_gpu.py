"""PagedKVPool(share_blocks=True): per-block share counts on the device, fork and the reference-counted release
(ll_kv_paged_fork / ll_kv_paged_release_shared), held to the sequential model of tests/_paged_share_ref.py exactly --
state, req_blocks, held block-table prefixes, free stack in order, token table and share counts after every operation
of random admit / fork / append / release sequences -- plus the pool contents after a fork (the child's rows are bit-equal
to the parent's, every other row is untouched), the all-or-nothing refusals, and agreement with the plain pool when
nothing is ever forked."""

from collections import Counter

import numpy as np
import pytest
import torch

from lite_llama_amd.executor.paged_kv import PagedKVPool
from tests._paged_share_ref import RandomOps, SharedPagedPoolModel, check_invariants, check_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _same(pool, table, model):
    st = pool.state.cpu().numpy()
    assert int(st[0]) == model.free and int(st[1]) == model.err, (st, model.free, model.err)
    assert np.array_equal(pool.req_blocks.cpu().numpy(), model.req_blocks)
    got_bt = pool.block_table.cpu().numpy()
    for r in range(len(model.req_blocks)):  # only the held prefix of a row is defined
        n = int(model.req_blocks[r])
        assert np.array_equal(got_bt[r, :n], model.block_table[r, :n]), r
    stack = pool.free_stack.cpu().numpy()
    assert np.array_equal(stack[: model.free], np.array(model.stack[: model.free], dtype=np.int32))
    assert np.array_equal(table.cpu().numpy(), model.token_table)
    share = pool.block_share.cpu().numpy()
    assert np.array_equal(share, model.share)
    assert not pool.share_scratch.cpu().numpy().any()          # zero at rest
    check_invariants(model.nb, int(st[0]), stack, pool.req_blocks.cpu().numpy(), got_bt, share)
    check_model(model)


@pytest.mark.parametrize("bs,seed", [(1, 0), (8, 1), (64, 2), (8, 5)])
def test_random_sequences_match_the_model(bs, seed):
    max_req, max_len, nb = 16, 5 * bs + 3, 70
    pool = PagedKVPool(2, nb, bs, 1, 16, DEV, max_req, max_len, share_blocks=True)
    model = SharedPagedPoolModel(nb, bs, max_req, max_len)
    table = torch.zeros(max_req, max_len, dtype=torch.int32, device=DEV)
    ops = RandomOps(seed, bs, max_req, max_len)
    seen = {"fork": 0, "release": 0, "shared_release": 0, "joint_release": 0, "all_holders_in_one_call": 0}
    for step in range(160):
        op, a = ops.next()
        if op == "admit":
            sel = pool.admit(_i32(a[0]), _i32(a[1]), a[2], table)
            assert np.array_equal(sel.cpu().numpy(), model.extend(a[0], a[1], a[2], 0)), step
            ops.admitted(a[0], a[1], model.req_blocks)
        elif op == "fork":
            pool.fork(_i32(a[0]), _i32(a[1]), _i32(a[2]), table)
            if model.fork(*a):
                ops.forked(a[1], a[2])
                seen["fork"] += 1
        elif op == "append":
            sel = pool.append(_i32(a[0]), _i32(a[1]), table)
            assert np.array_equal(sel.cpu().numpy(), model.extend(a[0], a[1], 1, 1)), step
            ops.appended(a[0], a[1], model.req_blocks)
            share = pool.block_share.cpu().numpy()
            for r, n in zip(*a):               # the block an append writes has no other holder
                if int(model.req_blocks[r]) * bs >= n:
                    assert share[model.block_table[r, (n - 1) // bs]] == 0
        elif op == "release":
            blocks = [int(model.block_table[r, j]) for r in a[0] for j in range(model.req_blocks[r])]
            seen["shared_release"] += sum(model.share[b] > 0 for b in blocks)
            seen["joint_release"] += len(blocks) - len(set(blocks))
            seen["all_holders_in_one_call"] += sum(k > 1 and k == model.share[b] + 1 for b, k in Counter(blocks).items())
            pool.release(_i32(a[0]))
            model.release(a[0])
            ops.released(a[0])
            seen["release"] += 1
        _same(pool, table, model)
    assert seen["fork"] >= 5 and seen["release"] >= 5 and seen["shared_release"] >= 3, seen
    assert seen["joint_release"] >= 1 and seen["all_holders_in_one_call"] >= 1, seen


@pytest.mark.parametrize("bs", [1, 8, 64])
def test_release_orders_and_all_holders_in_one_call(bs):
    """Parent before children, children before parent, and every holder of a block in one call (then the last holder in
    call order pushes it, at its place in the scan)."""
    max_req, max_len, nb = 8, 4 * bs + 3, 40
    for order in ([[0], [1, 2, 3]], [[3, 1], [2], [0]], [[2, 0, 3, 1]], [[1, 0], [3, 2]]):
        pool = PagedKVPool(1, nb, bs, 1, 16, DEV, max_req, max_len, share_blocks=True)
        model = SharedPagedPoolModel(nb, bs, max_req, max_len)
        table = torch.zeros(max_req, max_len, dtype=torch.int32, device=DEV)
        ln = 3 * bs + 2 if bs > 2 else 3 * bs
        pool.admit(_i32([0]), _i32([ln]), ln, table)
        model.extend([0], [ln], ln, 0)
        f = ([0, 0], [1, 2], [ln, 2 * bs])                                  # two children of the parent
        pool.fork(*(_i32(v) for v in f), table)
        assert model.fork(*f)
        f = ([1], [3], [2 * bs + 1 if bs > 1 else 2])                       # a chain: the child of a child
        pool.fork(*(_i32(v) for v in f), table)
        assert model.fork(*f)
        _same(pool, table, model)
        assert model.share[model.block_table[0, 0]] == 3
        for reqs in order:
            pool.release(_i32(reqs))
            model.release(reqs)
            _same(pool, table, model)
        assert pool.free_blocks == nb - 1 and pool.error == 0 and not pool.block_share.any().item()


def _filled_pool(dtype, bs, layers=3, nb=24, max_req=8, heads=2, dim=16):
    pool = PagedKVPool(layers, nb, bs, heads, dim, DEV, max_req, 6 * bs, dtype=dtype, share_blocks=True)
    g = torch.Generator(device=DEV).manual_seed(7)
    for kv in pool.kv_buffer:                                               # seeded random BYTES: every row is distinct
        kv.view(torch.uint8).copy_(torch.randint(0, 256, kv.view(torch.uint8).shape, dtype=torch.uint8, device=DEV, generator=g))
    return pool


def _bytes(pool):
    return [kv.view(torch.uint8).reshape(kv.shape[0], -1).clone() for kv in pool.kv_buffer]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float8_e4m3fn], ids=["fp16", "bf16", "e4m3"])
@pytest.mark.parametrize("bs", [8, 64])
def test_fork_copies_the_partial_block_in_every_layer_and_touches_nothing_else(dtype, bs):
    pool = _filled_pool(dtype, bs)
    nb = pool.num_blocks
    table = torch.zeros(8, 6 * bs, dtype=torch.int32, device=DEV)
    lens = [2 * bs + 5, bs + bs - 1]
    pool.admit(_i32([0, 1]), _i32(lens), max(lens), table)
    before = _bytes(pool)
    src, dst, ln = [0, 0, 1, 0], [2, 3, 4, 5], [2 * bs + 5, 2 * bs + 1, 2 * bs - 1, 2 * bs]
    pool.fork(_i32(src), _i32(dst), _i32(ln), table)
    assert pool.error == 0
    t = table.cpu().long()
    after = _bytes(pool)
    written = torch.zeros(nb * bs, dtype=torch.bool)
    for s, d, n in zip(src, dst, ln):
        full = n // bs * bs
        assert torch.equal(t[d, :full], t[s, :full]) and not set(t[d, full:n].tolist()) & set(t[s].tolist())
        written[t[d, full:n]] = True
        for layer in range(len(after)):                                    # the child reads what the parent reads
            assert torch.equal(after[layer][t[d, :n].to(DEV)], after[layer][t[s, :n].to(DEV)]), (d, layer)
    assert int(written.sum()) == 5 + 1 + (bs - 1)
    keep = (~written).to(DEV)
    keep[(nb - 1) * bs:] = False                                            # the junk block aside
    for layer in range(len(after)):
        assert torch.equal(after[layer][keep], before[layer][keep]), layer


def test_refusals_are_all_or_nothing():
    bs, nb = 4, 7                                                           # 6 usable blocks
    pool = _filled_pool(torch.float16, bs, nb=nb, max_req=6)
    model = SharedPagedPoolModel(nb, bs, 6, 6 * bs)
    table = torch.zeros(6, 6 * bs, dtype=torch.int32, device=DEV)
    pool.admit(_i32([0, 4]), _i32([10, 3]), 10, table)                      # 3 + 1 blocks, 2 free
    model.extend([0, 4], [10, 3], 10, 0)
    _same(pool, table, model)
    before = _bytes(pool)

    def refused(f, bit):
        pool.state[1] = 0
        model.err = 0
        pool.fork(*(_i32(v) for v in f), table)
        assert not model.fork(*f)
        assert pool.error == bit == model.err
        _same(pool, table, model)
        for a, b in zip(_bytes(pool), before):
            assert torch.equal(a, b)

    refused(([0, 0, 0], [1, 2, 3], [10, 9, 7]), 1)                          # three partial blocks, two free
    refused(([0], [1], [13]), 4)                                            # beyond the source's blocks
    refused(([0, 0], [1, 4], [8, 8]), 4)                                    # a child that already holds blocks
    refused(([0, 0], [1, 2], [8, 0]), 4)                                    # an empty fork
    refused(([0, 0], [1, 1], [8, 8]), 4)                                    # a child listed twice
    refused(([0, 0, 0], [2, 1, 2], [10, 8, 4]), 4)
    refused(([0, 1], [1, 2], [8, 8]), 4)                                    # a child that is a source of the same call
    refused(([1, 0], [2, 1], [8, 8]), 4)
    pool.state[1] = 0
    model.err = 0
    f = ([0, 0], [1, 2], [10, 8])
    pool.fork(*(_i32(v) for v in f), table)
    assert model.fork(*f) and pool.error == 0
    _same(pool, table, model)
    # a pool without share counts has no fork, and its release is the plain one
    plain = PagedKVPool(1, 8, 4, 1, 16, DEV, 4, 16)
    with pytest.raises(ValueError, match="share_blocks=True"):
        plain.fork(_i32([0]), _i32([1]), _i32([1]), table)
    assert not hasattr(plain, "block_share")


def test_without_forks_the_shared_pool_is_the_plain_pool():
    rng = np.random.default_rng(4)
    bs, max_req, max_len, nb = 8, 12, 70, 60
    a = PagedKVPool(1, nb, bs, 1, 32, DEV, max_req, max_len, share_blocks=True)
    b = PagedKVPool(1, nb, bs, 1, 32, DEV, max_req, max_len)
    ta, tb = (torch.zeros(max_req, max_len, dtype=torch.int32, device=DEV) for _ in range(2))
    lens = np.zeros(max_req, dtype=np.int64)
    live = set()
    for step in range(120):
        op = rng.integers(0, 10)
        idle = [r for r in range(max_req) if r not in live]
        if op < 3 and idle:
            reqs = [int(r) for r in rng.choice(idle, int(rng.integers(1, min(4, len(idle)) + 1)), replace=False)]
            ln = [int(rng.integers(1, 30)) for _ in reqs]
            sa, sb = (p.admit(_i32(reqs), _i32(ln), max(ln) + 1, t) for p, t in ((a, ta), (b, tb)))
            assert torch.equal(sa, sb)
            held = b.req_blocks.cpu().numpy()
            for r, n in zip(reqs, ln):
                if held[r] * bs >= n:
                    live.add(r)
                    lens[r] = n
        elif op < 8 and live:
            reqs = [r for r in sorted(live) if lens[r] + 1 <= max_len and rng.integers(0, 2)]
            if not reqs:
                continue
            new = [int(lens[r] + 1) for r in reqs]
            sa, sb = (p.append(_i32(reqs), _i32(new), t) for p, t in ((a, ta), (b, tb)))
            assert torch.equal(sa, sb)
            held = b.req_blocks.cpu().numpy()
            for r, n in zip(reqs, new):
                if held[r] * bs >= n:
                    lens[r] = n
        elif live:
            reqs = [int(r) for r in rng.choice(sorted(live), int(rng.integers(1, min(3, len(live)) + 1)), replace=False)]
            a.release(_i32(reqs))
            b.release(_i32(reqs))
            for r in reqs:
                live.discard(r)
                lens[r] = 0
        assert torch.equal(a.state, b.state) and torch.equal(a.req_blocks, b.req_blocks) and torch.equal(ta, tb), step
        free = int(b.state[0].item())
        assert torch.equal(a.free_stack[:free], b.free_stack[:free]), step
        held = b.req_blocks.cpu().tolist()
        for r, n in enumerate(held):
            assert torch.equal(a.block_table[r, :n], b.block_table[r, :n])
        assert not a.block_share.any().item() and not a.share_scratch.any().item()
    # reset clears the counts
    a.reset()
    a.admit(_i32([0]), _i32([20]), 20, ta)
    a.fork(_i32([0, 0]), _i32([1, 2]), _i32([20, 16]), ta)
    assert a.block_share[:3].tolist() == [2, 2, 0] and a.free_blocks == nb - 1 - 4 and a.error == 0
    a.reset()
    assert not a.block_share.any().item() and a.free_blocks == nb - 1 and a.error == 0
