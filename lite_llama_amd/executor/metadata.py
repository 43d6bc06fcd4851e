"""The per-step metadata struct every attention kernel call reads (lite_llama/executor/attention_metadata.py:19-44)."""

from __future__ import annotations

from dataclasses import dataclass, field

import torch


@dataclass
class AttentionMetadata:
    """The struct every attention kernel call reads (same field names as the reference)."""

    kv_buffer: list = field(default_factory=list)        # per layer [max_tokens, 2*Hkv, D]
    cur_select_index: torch.Tensor | None = None          # rows written this step (int32)
    b_req_tokens_table: torch.Tensor | None = None        # [max_requests, max_seq_len] int32
    b_start_loc: torch.Tensor | None = None               # prefill only
    b_req_idx: torch.Tensor | None = None
    b_seq_len: torch.Tensor | None = None
    max_actual_seq_len: int = 0
    # chunk steps (extension): sequence b already holds b_ctx_len[b] tokens in the pool; b_seq_len / max_actual_seq_len
    # then count this step's new tokens only (the queries of prefill_paged_attention), max_ctx_len bounds b_ctx_len
    b_ctx_len: torch.Tensor | None = None
    max_ctx_len: int = 0
    kv_scales: tuple = (1.0, 1.0)                          # fp8 KV pool only (extension): stored value * scale = K / V
    # shared prompt prefix (extension): table[b_req_idx[b], :shared_prefix_len] == table[shared_prefix_req, :shared_prefix_len]
    # for every row of the batch; 0: no sharing.  Decode steps then read the prefix's K/V once per query tile
    # (kernels.shared_prefix_decode_attention) from kernels.attention.SHARED_PREFIX_MIN_LEN positions on
    shared_prefix_len: int = 0
    shared_prefix_req: int = 0
