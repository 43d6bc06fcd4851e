"""Block-granular KV pool on the device (extension -- the reference's pool is token-granular with the
paging TODO at executor/kv_cache_manager.py:211).  Same storage as :class:`KVPool` (one ``[rows, 2*Hkv, D]`` tensor per
layer, rows = blocks x block_size), handed out in blocks; the per-token table the kernels read
(``b_req_tokens_table``) is derived on the device by ``ll_kv_paged_extend``, so the attention / KV-write kernels and
their results are those of token attention.  Nothing is read back: admission, the per-step append and release are
stream-ordered launches (the append sits inside the captured decode step); the host looks at ``free_blocks`` /
``error`` only when it chooses to synchronise.

``share_blocks=True`` adds a per-block share count on the device (holders minus one) and :meth:`fork`: a new request
names another request's full blocks and gets a private copy of the partial last block, so no shared block is ever written
(every writer writes at or beyond its own length) and the entries above and the kernels stay as they are; ``release``
then frees a block only when its last holder lets go."""

from __future__ import annotations

import torch

from .. import _lib as L


class PagedKVPool:
    def __init__(self, num_layers: int, num_blocks: int, block_size: int, num_kv_heads: int, head_dim: int, device,
                 max_requests: int, max_seq_len: int, dtype=torch.float16, share_blocks: bool = False):
        if block_size < 1 or num_blocks < 2:
            raise ValueError("PagedKVPool needs block_size >= 1 and num_blocks >= 2 (one block is the junk block)")
        self.block_size, self.num_blocks, self.device = block_size, num_blocks, device
        self.max_requests, self.max_seq_len = max_requests, max_seq_len
        self.max_tokens = num_blocks * block_size
        self.kv_buffer = [torch.zeros(self.max_tokens, 2 * num_kv_heads, head_dim, dtype=dtype, device=device)
                          for _ in range(num_layers)]
        self.blocks_per_request = (max_seq_len + block_size - 1) // block_size
        self.free_stack = torch.empty(num_blocks - 1, dtype=torch.int32, device=device)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)          # [free blocks, error flags]
        self.block_table = torch.zeros(max_requests, self.blocks_per_request, dtype=torch.int32, device=device)
        self.req_blocks = torch.zeros(max_requests, dtype=torch.int32, device=device)
        self.share_blocks = bool(share_blocks)
        if self.share_blocks:
            self.row_bytes = 2 * num_kv_heads * head_dim * self.kv_buffer[0].element_size()
            if self.row_bytes % 16:
                raise ValueError(f"share_blocks needs pool rows of a multiple of 16 bytes (the fork copies 16-byte words), "
                                 f"got {self.row_bytes}")
            self.block_share = torch.zeros(num_blocks, dtype=torch.int32, device=device)    # holders - 1
            # zero at rest: per block the holders a release call lists and its last caller + 1, then the fork's two words
            self.share_scratch = torch.zeros(2 * num_blocks + 2, dtype=torch.int32, device=device)
            self.layer_base = torch.tensor([kv.data_ptr() for kv in self.kv_buffer], dtype=torch.int64, device=device)
        self.reset()

    def reset(self) -> None:
        L.check(L.lib().ll_kv_paged_reset(self.free_stack.data_ptr(), self.state.data_ptr(), self.req_blocks.data_ptr(),
                                          self.num_blocks, self.max_requests, L.stream_ptr()), "kv_paged_reset")
        if self.share_blocks:
            self.block_share.zero_()

    def _extend(self, req_idx, lens, len_bias, grid_len, from_end, token_table, out=None):
        n = req_idx.numel()
        L.require_cuda(req_idx, lens, token_table)
        if req_idx.dtype != torch.int32 or lens.dtype != torch.int32 or token_table.dtype != torch.int32:
            raise ValueError("PagedKVPool: request indices, lengths and the token table must be int32")
        if token_table.stride(1) != 1 or not req_idx.is_contiguous() or not lens.is_contiguous():
            raise ValueError("PagedKVPool: the token table must be row-major, indices and lengths contiguous")
        select = out if out is not None else torch.empty(n * grid_len, dtype=torch.int32, device=self.device)
        if select.dtype != torch.int32 or select.numel() != n * grid_len or not select.is_contiguous():
            raise ValueError("PagedKVPool: the row output must be a contiguous int32 tensor of n * grid_len entries")
        L.check(L.lib().ll_kv_paged_extend(
            self.free_stack.data_ptr(), self.state.data_ptr(), self.block_table.data_ptr(), self.block_table.stride(0),
            self.req_blocks.data_ptr(), req_idx.data_ptr(), lens.data_ptr(), len_bias, n, self.block_size, grid_len,
            from_end, token_table.data_ptr(), token_table.stride(0), select.data_ptr(), self.num_blocks, L.stream_ptr()),
            "kv_paged_extend")
        return select

    @torch.no_grad()
    def admit(self, req_idx: torch.Tensor, lens: torch.Tensor, grid_len: int, token_table: torch.Tensor) -> torch.Tensor:
        """Blocks for ``lens[i]`` tokens of every listed request + the rows of the padded prefill grid ``[n, grid_len]``
        (``cur_select_index``; pad positions name junk rows); fills ``token_table[req, :len]``."""
        return self._extend(req_idx, lens, 0, grid_len, 0, token_table)

    @torch.no_grad()
    def append(self, req_idx: torch.Tensor, seq_len: torch.Tensor, token_table: torch.Tensor, out=None) -> torch.Tensor:
        """The decode step's row: position ``seq_len[i] - 1`` of every listed request (a new block is popped when the
        position opens one); writes ``token_table[req, seq_len - 1]`` and returns / fills ``cur_select_index``."""
        return self._extend(req_idx, seq_len, 0, 1, 1, token_table, out=out)

    def reserve(self, n: int) -> None:
        """Nothing is reserved ahead: every step's :meth:`append` pops a block when a position opens one."""

    @torch.no_grad()
    def extend_at(self, req_idx: torch.Tensor, ctx_lens: torch.Tensor, chunk_lens: torch.Tensor, grid_len: int,
                  token_table: torch.Tensor, out=None) -> torch.Tensor:
        """A chunk step: request ``i``'s row of the ``[n, grid_len]`` grid holds positions ``ctx_lens[i] + g``, the first
        ``chunk_lens[i]`` of them valid.  Blocks are popped up to ``ctx_lens[i] + chunk_lens[i]`` only, valid positions
        get ``token_table[req, ctx + g]``, pads junk rows (never one of the request's own prefix rows).  Returns / fills
        ``cur_select_index``."""
        n = req_idx.numel()
        L.require_cuda(req_idx, ctx_lens, chunk_lens, token_table)
        for t in (req_idx, ctx_lens, chunk_lens, token_table):
            if t.dtype != torch.int32:
                raise ValueError("PagedKVPool: request indices, lengths and the token table must be int32")
        if (token_table.stride(1) != 1 or not req_idx.is_contiguous() or not ctx_lens.is_contiguous()
                or not chunk_lens.is_contiguous() or ctx_lens.numel() != n or chunk_lens.numel() != n):
            raise ValueError("PagedKVPool: the token table must be row-major, indices and lengths contiguous, one per request")
        select = out if out is not None else torch.empty(n * grid_len, dtype=torch.int32, device=self.device)
        if select.dtype != torch.int32 or select.numel() != n * grid_len or not select.is_contiguous():
            raise ValueError("PagedKVPool: the row output must be a contiguous int32 tensor of n * grid_len entries")
        L.check(L.lib().ll_kv_paged_extend_at(
            self.free_stack.data_ptr(), self.state.data_ptr(), self.block_table.data_ptr(), self.block_table.stride(0),
            self.req_blocks.data_ptr(), req_idx.data_ptr(), ctx_lens.data_ptr(), chunk_lens.data_ptr(), n,
            self.block_size, grid_len, token_table.data_ptr(), token_table.stride(0), select.data_ptr(), self.num_blocks,
            L.stream_ptr()), "kv_paged_extend_at")
        return select

    @torch.no_grad()
    def fork(self, src_req: torch.Tensor, dst_req: torch.Tensor, lens: torch.Tensor, token_table: torch.Tensor) -> None:
        """Request ``dst_req[i]`` (holding nothing) becomes a copy of the first ``lens[i]`` positions of ``src_req[i]``:
        it names the source's ``lens[i] // block_size`` full blocks (share count + 1 each) and gets a fresh block holding a
        copy, in every layer, of the ``lens[i] % block_size`` rows after them; ``token_table[dst, :lens[i]]`` is filled.
        The same source may be listed many times (n samples of a prompt) and a ``dst`` may be the source of a later call.
        All-or-nothing: ``error`` bit 4 if a ``dst`` holds blocks, is listed twice or is a source of the same call, or a
        length is < 1 or beyond the source's blocks; bit 1 if the free blocks do not suffice."""
        if not self.share_blocks:
            raise ValueError("PagedKVPool.fork needs a pool created with share_blocks=True (per-block share counts)")
        n = src_req.numel()
        L.require_cuda(src_req, dst_req, lens, token_table)
        for t in (src_req, dst_req, lens, token_table):
            if t.dtype != torch.int32:
                raise ValueError("PagedKVPool: request indices, lengths and the token table must be int32")
        if (token_table.stride(1) != 1 or not src_req.is_contiguous() or not dst_req.is_contiguous()
                or not lens.is_contiguous() or dst_req.numel() != n or lens.numel() != n):
            raise ValueError("PagedKVPool: the token table must be row-major, indices and lengths contiguous, one per fork")
        L.check(L.lib().ll_kv_paged_fork(
            self.free_stack.data_ptr(), self.state.data_ptr(), self.block_table.data_ptr(), self.block_table.stride(0),
            self.req_blocks.data_ptr(), self.block_share.data_ptr(), self.share_scratch.data_ptr(), src_req.data_ptr(),
            dst_req.data_ptr(), lens.data_ptr(), n, self.block_size, token_table.data_ptr(), token_table.stride(0),
            self.layer_base.data_ptr(), len(self.kv_buffer), self.row_bytes, self.num_blocks, L.stream_ptr()),
            "kv_paged_fork")

    @torch.no_grad()
    def release(self, req_idx: torch.Tensor) -> None:
        L.require_cuda(req_idx)
        if self.share_blocks:
            L.check(L.lib().ll_kv_paged_release_shared(
                self.free_stack.data_ptr(), self.state.data_ptr(), self.block_table.data_ptr(), self.block_table.stride(0),
                self.req_blocks.data_ptr(), self.block_share.data_ptr(), self.share_scratch.data_ptr(), req_idx.data_ptr(),
                req_idx.numel(), self.num_blocks, L.stream_ptr()), "kv_paged_release_shared")
            return
        L.check(L.lib().ll_kv_paged_release(self.free_stack.data_ptr(), self.state.data_ptr(), self.block_table.data_ptr(),
                                            self.block_table.stride(0), self.req_blocks.data_ptr(), req_idx.data_ptr(),
                                            req_idx.numel(), L.stream_ptr()), "kv_paged_release")

    # host-visible (synchronising) views
    @property
    def free_blocks(self) -> int:
        return int(self.state[0].item())

    @property
    def error(self) -> int:
        """0, or flags: 1 = a call found too few free blocks (it allocated nothing), 2 = a request outgrew max_seq_len,
        4 = a fork broke its contract (a child that holds blocks, is listed twice or is a source of the same call, a length
        < 1 or beyond the source's blocks; it changed nothing)."""
        return int(self.state[1].item())

    def snapshot(self):
        return self.state.clone(), self.req_blocks.clone(), self.block_table.clone()

    def restore(self, snap) -> None:
        """Undo appends made since ``snapshot`` (pops only move the stack top: the stack itself is intact)."""
        self.state.copy_(snap[0])
        self.req_blocks.copy_(snap[1])
        self.block_table.copy_(snap[2])
