"""Host side of chunked prefill (no GPU): the chunk planner's metadata, the float64 paged reference against
_attn_ref.prefill_ref at ctx = 0, a restatement of the paged allocator's extend_at mode, and the continuation grid of
SlotBatch.begin_prefill(cached_lens=...)."""

import types

import pytest
import torch

from lite_llama_amd.executor.chunking import plan_prefill_chunks
from tests._attn_ref import prefill_inputs, prefill_ref
from tests._paged_ref import paged_prefill_ref


@pytest.mark.parametrize("lens,grid", [([5, 2, 7], 7), ([1], 1), ([13, 13], 13), ([9, 1, 4, 6], 9)])
@pytest.mark.parametrize("chunk", [1, 3, 64])
def test_chunk_plan(lens, grid, chunk):
    plans = plan_prefill_chunks(lens, grid, chunk)
    b = len(lens)
    assert [p.col0 for p in plans] == list(range(0, grid, chunk))
    assert sum(p.width for p in plans) == grid and all(1 <= p.width <= chunk for p in plans)
    seen_end = []
    cached = [0] * b
    cells = set()
    for p in plans:
        assert p.b_start_loc.tolist() == [i * p.width for i in range(b)]
        assert p.b_ctx_len.tolist() == cached                      # each chunk starts where the earlier ones stopped
        for i in range(b):
            n = int(p.b_q_len[i])
            assert n == max(0, min(p.width, lens[i] - p.col0))
            assert p.positions[i, :n].tolist() == list(range(cached[i], cached[i] + n))
            assert int(p.positions[i].max()) < grid                # pads stay inside the prompt grid
            cached[i] += n
        assert p.max_q_len == int(p.b_q_len.max()) and p.max_ctx_len == int(p.b_ctx_len.max())
        for i, r in zip(p.ends.tolist(), p.logits_rows.tolist()):
            assert r == i * p.width + lens[i] - 1 - p.col0 and 0 <= lens[i] - 1 - p.col0 < p.width
            seen_end.append(i)
        for r, c, f in zip(p.valid_rows.tolist(), p.valid_cols.tolist(), p.valid_flat.tolist()):
            j = f - r * p.width
            assert 0 <= j < int(p.b_q_len[r]) and c == int(p.b_ctx_len[r]) + j
            assert (r, c) not in cells
            cells.add((r, c))
    assert cached == list(lens)
    assert sorted(seen_end) == list(range(b))                      # every sequence's last token: exactly one chunk
    assert cells == {(i, j) for i in range(b) for j in range(lens[i])}


def test_chunk_plan_rejects():
    with pytest.raises(ValueError):
        plan_prefill_chunks([3], 3, 0)
    with pytest.raises(ValueError):
        plan_prefill_chunks([4], 3, 2)
    with pytest.raises(ValueError):
        plan_prefill_chunks([0, 3], 3, 2)


@pytest.mark.parametrize("d", [32, 128])
def test_paged_reference_is_prefill_ref_at_ctx0(d):
    inp = prefill_inputs("wide", [37, 5, 64], 8, 2, d, torch.float16, seed=1)
    ref, vmax, z, n, idx = prefill_ref(inp["q"], inp["k"], inp["v"], inp["sm_scale"], inp["start"], inp["seq"])
    # identity table: position p of sequence b is packed row start[b] + p
    rows = inp["k"].shape[0]
    table = torch.stack([torch.arange(rows) - 0 + int(s) for s in inp["start"]]).clamp(max=rows - 1).to(torch.int32)
    b = len(inp["seq"])
    got, gv, gz, gn, gidx = paged_prefill_ref(inp["q"], inp["k"], inp["v"], inp["sm_scale"], table, torch.arange(b),
                                              inp["start"], inp["seq"], torch.zeros(b, dtype=torch.int32))
    assert torch.equal(gidx, idx) and torch.equal(gn, n)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gz, z, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gv, vmax, rtol=0, atol=0)


def _extend_at(state, block_table, req_blocks, free_stack, req_idx, ctx, chunk, grid_len, block_size, num_blocks,
               token_table):
    """Restatement of ll_kv_paged_extend_at (csrc/kv_paged.hip): reserve up to ctx + n, then the rows of positions
    ctx + g (g < grid_len) -- valid for g < n, junk-block rows for pads."""
    need = []
    for i, r in enumerate(req_idx):
        want = -(-(ctx[i] + chunk[i]) // block_size)
        need.append(max(0, want - req_blocks[r]))
    if sum(need) > state[0]:
        state[1] |= 1
    else:
        top = state[0]
        for i, r in enumerate(req_idx):
            for j in range(need[i]):
                top -= 1
                block_table[r][req_blocks[r] + j] = free_stack[top]
            req_blocks[r] += need[i]
        state[0] = top
    out = []
    for i, r in enumerate(req_idx):
        for g in range(grid_len):
            p = ctx[i] + g
            row = (num_blocks - 1) * block_size + p % block_size
            if p < ctx[i] + chunk[i] and p // block_size < req_blocks[r]:
                row = block_table[r][p // block_size] * block_size + p % block_size
                token_table[r][p] = row
            out.append(row)
    return out


@pytest.mark.parametrize("block_size", [1, 4, 16])
def test_extend_at_never_maps_pads_to_prefix_rows(block_size):
    num_blocks, max_len = 128, 96
    free_stack = list(range(num_blocks - 2, -1, -1))
    state = [num_blocks - 1, 0]
    block_table = [[-1] * (max_len // block_size + 1) for _ in range(3)]
    req_blocks = [0, 0, 0]
    table = [[-1] * max_len for _ in range(3)]
    lens = [40, 7, 23]
    chunk_size = 9
    for plan in plan_prefill_chunks(lens, max(lens), chunk_size):
        ctx, n = plan.b_ctx_len.tolist(), plan.b_q_len.tolist()
        before = [list(r) for r in table]
        rows = _extend_at(state, block_table, req_blocks, free_stack, [0, 1, 2], ctx, n, plan.width, block_size,
                          num_blocks, table)
        junk = set(range((num_blocks - 1) * block_size, num_blocks * block_size))
        for i in range(3):
            prefix = {table[i][p] for p in range(ctx[i])}
            assert table[i][:ctx[i]] == before[i][:ctx[i]]       # the cached prefix is never renamed
            for g in range(plan.width):
                row = rows[i * plan.width + g]
                if g < n[i]:
                    assert row == table[i][ctx[i] + g] and row not in junk
                else:
                    assert row in junk and row not in prefix      # a pad never names one of the request's rows
            # blocks only up to ctx + n
            assert req_blocks[i] == -(-(ctx[i] + n[i]) // block_size)
        assert state[1] == 0
    owned = [table[i][p] for i in range(3) for p in range(lens[i])]
    assert len(set(owned)) == len(owned)                        # every named row belongs to one position


@pytest.mark.parametrize("ctx0", [0, 9])
def test_bump_pool_extend_at_writes_the_cells_the_plan_lists(ctx0):
    """KVPool.extend_at against the plan's own ``valid_rows / valid_cols / valid_flat``: rows come off the cursor in grid
    order, the table cells of the valid positions name them, every other cell keeps its value."""
    from lite_llama_amd.executor import KVPool

    lens, width = [5, 17, 1, 12], 40 - ctx0
    req = torch.arange(4, dtype=torch.int32)
    table = torch.randint(1000, 2000, (6, 40), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    want, pool, used = table.clone(), KVPool(1, 4000, 1, 8, "cpu"), 0
    for plan in plan_prefill_chunks(lens, width, 6):
        select = pool.extend_at(req, plan.b_ctx_len + ctx0, plan.b_q_len, plan.width, table)
        rows = torch.arange(used, used + 4 * plan.width, dtype=torch.int32)
        used += 4 * plan.width
        want[plan.valid_rows, plan.valid_cols + ctx0] = rows[plan.valid_flat]
        assert torch.equal(select, rows) and select.dtype == torch.int32 and pool.used == used
        assert torch.equal(table, want), plan.col0
    # the padded grid of a one-step prefill is the chunk at context 0
    one = table.clone()
    assert torch.equal(pool.admit(req, torch.tensor(lens, dtype=torch.int32), 17, one), torch.arange(used, used + 68, dtype=torch.int32))
    for i, n in enumerate(lens):
        assert one[i, :n].tolist() == list(range(used + 17 * i, used + 17 * i + n)) and torch.equal(one[i, n:], table[i, n:])
    assert torch.equal(one[4:], table[4:])
    # a grid wider than what is left of the table rows: the valid positions are named, nothing is indexed past the row
    end = pool.extend_at(req[:2], torch.tensor([35, 38], dtype=torch.int32), torch.tensor([5, 2], dtype=torch.int32), 8, one)
    assert one[0, 35:].tolist() == end[:5].tolist() and one[1, 38:].tolist() == end[8:10].tolist()


class _Runner:
    """The slice of SlotRunner that SlotBatch reads, on the CPU."""

    def __init__(self, slots, max_seq_len):
        self.device = "cpu"
        self.max_seq_len = max_seq_len
        self.atten_info = types.SimpleNamespace(b_req_tokens_table=torch.zeros(slots, max_seq_len, dtype=torch.int32),
                                                b_req_idx=None, b_seq_len=None, b_start_loc=None, cur_select_index=None,
                                                max_actual_seq_len=0, b_ctx_len=None, max_ctx_len=0)
        self.b_req_tokens_table = self.atten_info.b_req_tokens_table
        self.pool = types.SimpleNamespace(kv_buffer=[torch.zeros(slots * max_seq_len, 2, 8)], claim=lambda rows: None)

    def graph_batch_size(self, n):
        return n


def test_slot_continuation_grid_stays_inside_its_slot():
    from lite_llama_amd.executor.slots import SlotBatch

    L = 32
    r = _Runner(4, L)
    sb = SlotBatch(r)
    sb.begin_prefill([0, 2], [5, 3], cached_lens=[27, 4])
    info = r.atten_info
    sel = info.cur_select_index.view(2, 5)
    assert sel[0].tolist() == [0 * L + 27 + j for j in range(5)]        # rows 27..31 of slot 0: its last five
    assert sel[1, :3].tolist() == [2 * L + 4 + j for j in range(3)]
    assert all(3 * L <= v < 4 * L for v in sel[1, 3:].tolist())        # pads: the filler slot's rows
    assert info.b_ctx_len.tolist() == [27, 4] and info.b_seq_len.tolist() == [5, 3] and info.max_ctx_len == 27
    assert info.b_start_loc.tolist() == [0, 5] and info.max_actual_seq_len == 5
    with pytest.raises(ValueError):
        sb.begin_prefill([0], [6], cached_lens=[27])                      # 27 + 6 > max_seq_len
    sb.begin_prefill([1], [4])                                            # the plain form clears the chunk metadata
    assert info.b_ctx_len is None
