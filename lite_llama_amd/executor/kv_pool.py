"""The reference's token-granular bump-allocated KV pool (lite_llama/executor/kv_cache_manager.py:197-216,286-292), behind
the prefill / decode interface of :class:`~.paged_kv.PagedKVPool`."""

import torch

from ..kernels import update_kv_index


class KVPool:
    """Token-granular KV pool: one ``[max_tokens, 2*Hkv, D]`` fp16 tensor per layer (K heads first),
    with the reference's contiguous bump allocator (kv_cache_manager.py:197-216,286-292)."""

    block_size = 1  # rows are handed out one by one: what two requests share, they share to the token
    error = 0       # nothing is decided on the device: an exhausted pool is raised by the call that meets it

    def __init__(self, num_layers: int, max_tokens: int, num_kv_heads: int, head_dim: int, device, dtype=torch.float16):
        self.max_tokens = max_tokens
        self.device = device
        self.kv_buffer = [torch.zeros(max_tokens, 2 * num_kv_heads, head_dim, dtype=dtype, device=device)
                          for _ in range(num_layers)]
        self._next = 0

    def _bump(self, n: int) -> int:
        if self._next + n > self.max_tokens:
            raise RuntimeError(f"KV pool exhausted: need {n} rows, {self.max_tokens - self._next} free")
        self._next += n
        return self._next - n

    def alloc(self, n: int) -> torch.Tensor:
        start = self._bump(n)
        return torch.arange(start, start + n, dtype=torch.int32, device=self.device)

    def reset(self) -> None:
        self._next = 0

    def claim(self, num_rows: int) -> None:
        """Hand the first ``num_rows`` rows to an external owner (the slot layout); the bump cursor
        resumes just past them (kv_cache_manager.py:336-353)."""
        if num_rows > self.max_tokens:
            raise ValueError(f"cannot claim {num_rows} rows: the pool holds {self.max_tokens}")
        self._next = max(self._next, num_rows)

    @property
    def used(self) -> int:
        return self._next

    # ---- shared with PagedKVPool: a step's rows (``cur_select_index``) are returned, the table cells of its valid positions written
    @torch.no_grad()
    def admit(self, req_idx: torch.Tensor, lens: torch.Tensor, grid_len: int, token_table: torch.Tensor) -> torch.Tensor:
        """The padded prefill grid ``[n, grid_len]`` (_init_req_tokens_table, model_runner.py:153-179): fresh rows for all of
        it; a sequence's pad rows hold junk K/V that attention never reads, and its own decode steps name fresh rows."""
        return self.extend_at(req_idx, torch.zeros_like(lens), lens, grid_len, token_table)

    @torch.no_grad()
    def extend_at(self, req_idx: torch.Tensor, ctx_lens: torch.Tensor, chunk_lens: torch.Tensor, grid_len: int,
                  token_table: torch.Tensor) -> torch.Tensor:
        """A chunk step: request ``i``'s row of the ``[n, grid_len]`` grid holds positions ``ctx_lens[i] + g``, the first
        ``chunk_lens[i]`` of them valid: ``token_table[req, ctx + g]`` names their rows, every other cell keeps its value."""
        n = req_idx.numel()
        select = self.alloc(n * grid_len)
        # seen from the table: cell (req_idx[i], c) is grid column c - ctx_lens[i] of row i, if that is a valid one -- a
        # gather over whole table rows, so no cell is written twice and no index leaves the table, whatever the lengths
        col = torch.arange(token_table.shape[1], device=self.device).unsqueeze(0) - ctx_lens.view(n, 1)
        rows = req_idx.long()
        token_table[rows] = torch.where((col >= 0) & (col < chunk_lens.view(n, 1)),
                                        select.view(n, grid_len).gather(1, col.clamp(0, grid_len - 1)), token_table[rows])
        return select

    @torch.no_grad()
    def append(self, req_idx: torch.Tensor, seq_len: torch.Tensor, token_table: torch.Tensor, out=None) -> torch.Tensor:
        """The decode step's row, position ``seq_len[i] - 1`` of every listed request: the next ``n`` rows off the cursor,
        or -- with ``out``, the previous step's rows -- the ``n`` after those, advanced in place on the device (what a
        captured step replays; :meth:`reserve` has set them aside).  Writes ``token_table[req, seq_len - 1]``."""
        if out is None:
            out = self.alloc(req_idx.numel())
        else:
            out += req_idx.numel()
        update_kv_index(token_table, req_idx, seq_len, out)
        return out

    def reserve(self, n: int) -> None:
        """Set the next ``n`` rows aside for the steps after an :meth:`append`: each takes the B rows after the last one's."""
        if n > 0:
            self._bump(n)

    def snapshot(self):
        return None  # the cursor is host state that no step moves

    def restore(self, snap) -> None:
        pass
