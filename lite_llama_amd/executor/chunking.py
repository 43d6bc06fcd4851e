"""Chunked prefill planning (extension): how a right-padded prompt grid ``[B, Lp]`` is cut into successive chunk grids
``[B, <= chunk_size]``, each attending to what the earlier chunks cached.  Pure host code (CPU tensors only), so the
CPU tier can pin the metadata every chunk step hands to the model."""

from __future__ import annotations

from collections.abc import Sequence
from dataclasses import dataclass

import torch


@dataclass
class ChunkPlan:
    """One chunk step over grid columns ``[col0, col0 + width)`` of the prompt grid.

    ``b_start_loc`` / ``b_q_len`` / ``b_ctx_len`` (int32 ``[B]``): sequence ``i``'s new tokens start at flat row
    ``i * width`` of the chunk grid, it has ``b_q_len[i]`` of them (0 once its prompt is done) after ``b_ctx_len[i]``
    cached ones.  ``positions`` (int64 ``[B, width]``): ``ctx + j`` for valid tokens, pads clamped into the prompt
    grid.  ``ends`` lists the sequences whose last prompt token lies in this chunk and ``logits_rows`` its flat row in
    the chunk grid (same order).  ``valid_rows`` / ``valid_cols`` name the table cells ``(i, ctx_i + j)`` the chunk
    writes and ``valid_flat`` their flat grid rows ``i * width + j``."""

    col0: int
    width: int
    b_start_loc: torch.Tensor
    b_q_len: torch.Tensor
    b_ctx_len: torch.Tensor
    positions: torch.Tensor
    ends: torch.Tensor
    logits_rows: torch.Tensor
    valid_rows: torch.Tensor
    valid_cols: torch.Tensor
    valid_flat: torch.Tensor

    @property
    def max_q_len(self) -> int:
        return int(self.b_q_len.max()) if self.b_q_len.numel() else 0

    @property
    def max_ctx_len(self) -> int:
        return int(self.b_ctx_len.max()) if self.b_ctx_len.numel() else 0


def plan_prefill_chunks(prompt_lens: Sequence[int], grid_len: int, chunk_size: int) -> list[ChunkPlan]:
    """Cut the ``[len(prompt_lens), grid_len]`` prompt grid into chunks of at most ``chunk_size`` columns.  Chunk ``k``
    covers columns ``[k C, k C + width_k)``; sequence ``i`` takes ``min(C, len_i - k C)`` new tokens from it (0 when its
    prompt ended earlier) after ``min(k C, len_i)`` cached ones.  Every sequence's last prompt token lands in exactly one
    chunk."""
    if chunk_size < 1:
        raise ValueError(f"chunk_size must be >= 1, got {chunk_size}")
    lens = torch.as_tensor(list(prompt_lens), dtype=torch.int64)
    b = lens.numel()
    if b == 0 or grid_len < 1:
        raise ValueError("plan_prefill_chunks needs at least one sequence and a non-empty grid")
    if int(lens.min()) < 1 or int(lens.max()) > grid_len:
        raise ValueError(f"prompt lengths must lie in 1 .. {grid_len}, got {lens.tolist()}")
    plans = []
    for col0 in range(0, grid_len, chunk_size):
        width = min(chunk_size, grid_len - col0)
        ctx = lens.clamp(max=col0)
        n = (lens - col0).clamp(min=0, max=width)
        j = torch.arange(width, dtype=torch.int64)
        positions = (ctx[:, None] + j[None, :]).clamp(max=grid_len - 1)
        valid = j[None, :] < n[:, None]
        rows = torch.arange(b, dtype=torch.int64)[:, None].expand(b, width)
        ends = torch.nonzero((lens > col0) & (lens <= col0 + width)).view(-1)
        plans.append(ChunkPlan(
            col0=col0, width=width,
            b_start_loc=(torch.arange(b, dtype=torch.int64) * width).to(torch.int32),
            b_q_len=n.to(torch.int32), b_ctx_len=ctx.to(torch.int32), positions=positions,
            ends=ends, logits_rows=ends * width + (lens[ends] - 1 - col0),
            valid_rows=rows[valid], valid_cols=(ctx[:, None] + j[None, :])[valid],
            valid_flat=(rows * width + j[None, :])[valid]))
    return plans
