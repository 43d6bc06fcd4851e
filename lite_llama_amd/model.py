"""The decode-step caller of the kernel boundary -- this build's counterpart of
lite_llama/models/base.py:50-489 (PagedAttention / Attention / FusedMLP / DecoderLayer /
CausalLM.forward), qwen3_moe.py:60-111 (sparse MoE block) and rotary_embedding.py:34-137.

It fixes the per-layer call ORDER and wiring the reference uses, calling the 16-name kernel
boundary unchanged:
  norm -> q_proj, kv_proj -> split -> [qk-norm] -> rope -> cat(k, v) -> KV scatter ->
  attention (prefill: flash_attention2_no_pad with scale*log2e; decode: flash_decoding) ->
  o_proj (+TP all-reduce) -> norm (residual threaded in place) -> gate, up -> swiglu ->
  down (+all-reduce) | router -> fused_moe (+all-reduce);  final norm -> fp16 lm_head.
Checkpoint loading / HF config parsing are out of scope: geometry comes
from the static table below and weights are synthetic (seeded).
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import torch
import torch.nn as nn
import torch.nn.functional as F

from .distributed.parallel_state import all_reduce_tp, divide, get_tp_rank, get_tp_world_size
from .distributed.partition import ShardPlan, make_plan, scale_unit, set_active_plan
from .kernels import attention as _attention_kernels
from .kernels.attention import (decode_attention, decode_attention_partials, decode_attention_partials_supported,
                                shared_prefix_decode_attention, shared_prefix_supported)
from .kernels.norm_act import Int8Rows, PartialSums, ScaledInt32Partials, rope_and_cache, skip_rmsnorm_partials, skip_rmsnorm_q8
from .kernels import (
    flash_attention2_no_pad,
    flash_decoding,
    rope_emb_forward,
    skip_rmsnorm,
    swiglu_forward,
    update_kv_buffer,
    update_kv_buffer_fp8,
    flash_decoding_fp8kv,
    prefill_paged_attention,
)
from .linear import ColumnParallelLinear, LinearBase, MergedColumnLinear, RowParallelLinear
from .quantization import QuantConfig, get_moe_method
from .quantization.derived_layouts import derived_tensors, holds_packed

_LOG2E = 1.4426950408889634  # prefill kernel evaluates exp2 (base.py:45-47)


@dataclass(frozen=True)
class ModelGeometry:
    """Static geometry (public HF configs)."""

    name: str
    hidden_size: int
    num_layers: int
    num_heads: int
    num_kv_heads: int
    head_dim: int
    intermediate_size: int
    vocab_size: int
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    qkv_bias: bool = False
    use_qk_norm: bool = False
    tie_word_embeddings: bool = False
    rope_type: str = "default"
    rope_scaling: dict = field(default_factory=dict)
    # MoE (0 experts = dense MLP)
    num_experts: int = 0
    num_experts_per_tok: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = True

    @property
    def q_size(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim


GEOMETRY = {
    "qwen2.5-0.5b": ModelGeometry("qwen2.5-0.5b", 896, 24, 14, 2, 64, 4864, 151936, qkv_bias=True,
                                  tie_word_embeddings=True),
    "qwen2.5-1.5b": ModelGeometry("qwen2.5-1.5b", 1536, 28, 12, 2, 128, 8960, 151936, qkv_bias=True,
                                  tie_word_embeddings=True),
    "qwen2.5-7b": ModelGeometry("qwen2.5-7b", 3584, 28, 28, 4, 128, 18944, 152064, qkv_bias=True),
    "llama-3-8b": ModelGeometry("llama-3-8b", 4096, 32, 32, 8, 128, 14336, 128256, rms_norm_eps=1e-5,
                                rope_theta=5e5),
    "qwen3-30b-a3b": ModelGeometry("qwen3-30b-a3b", 2048, 48, 32, 4, 128, 6144, 151936, use_qk_norm=True,
                                   num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768),
}


def shard_plan(geo: ModelGeometry, quant: QuantConfig | None, tp: int | None = None) -> ShardPlan | None:
    """The tensor-parallel cut of this geometry: ``None`` when the reference's equal division applies (its code path and
    error messages stay in charge), else the extension plan of distributed/partition.py (KV-head replication, whole scale
    groups per rank).  MoE geometries: the plan only lays out the attention heads (KV heads replicated for tp > Hkv --
    Qwen3-30B-A3B's 32 / 4 heads at TP = 8); the experts keep the reference's equal cut of their intermediate dimension
    (SparseMoeBlock checks it against the scale granularity)."""
    tp = get_tp_world_size() if tp is None else tp
    if tp == 1:
        return None
    if geo.num_experts:
        try:
            plan = make_plan(geo.num_heads, geo.num_kv_heads, geo.head_dim, tp * 128, tp)  # (dense intermediate unused)
        except ValueError:
            return None
        return None if plan.uniform else plan
    try:
        plan = make_plan(geo.num_heads, geo.num_kv_heads, geo.head_dim, geo.intermediate_size, tp,
                         unit=scale_unit(quant, geo.intermediate_size))
    except ValueError:
        return None  # no plan: the reference's divide() raises its own error below
    return None if plan.uniform else plan


def tiny_geometry(**kw) -> ModelGeometry:
    """A small Qwen2-shaped geometry for tests / smoke."""
    base = dict(name="tiny", hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
                intermediate_size=512, vocab_size=1024, qkv_bias=True)
    base.update(kw)
    return ModelGeometry(**base)


# ------------------------------------------------------------------------------------- #
# rotary tables (rotary_embedding.py:34-137): fp32 math, cos/sin in the activation dtype,
# halves duplicated across the full head dim
# ------------------------------------------------------------------------------------- #
class RopeTables(tuple):
    """``(cos_table [P, D], sin_table [P, D], positions [tokens])``: the decode-step form of the
    position embeddings (instead of materialised ``[batch, 1, D]`` cos/sin)."""

    def __new__(cls, cos, sin, positions):
        return super().__new__(cls, (cos, sin, positions))

    def materialise(self):
        cos, sin, pos = self
        return cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)


class RotaryEmbedding(nn.Module):
    def __init__(self, geo: ModelGeometry):
        super().__init__()
        dim = geo.head_dim
        inv_freq = 1.0 / (geo.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        if geo.rope_type in ("llama3", "yarn"):
            sc = geo.rope_scaling
            factor, lo, hi = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"]
            orig = sc["original_max_position_embeddings"]
            wavelen = 2 * math.pi / inv_freq
            scaled = torch.where(wavelen > orig / lo, inv_freq / factor, inv_freq)
            smooth = (orig / wavelen - lo) / (hi - lo)
            smoothed = (1 - smooth) * scaled / factor + smooth * scaled
            mid = (wavelen <= orig / lo) & (wavelen >= orig / hi)
            inv_freq = torch.where(mid, smoothed, scaled)
        self.register_buffer("inv_freq", inv_freq, persistent=False)
        self._cache = None  # (cos [P, D], sin [P, D]) for positions 0..P-1, built with the very same ops

    @torch.no_grad()
    def _tables(self, pos: torch.Tensor, dtype):
        freqs = pos.to(torch.float32)[..., None] * self.inv_freq.to(pos.device)
        emb = torch.cat((freqs, freqs), dim=-1)
        return emb.cos().to(dtype), emb.sin().to(dtype)

    @torch.no_grad()
    def ensure(self, max_positions: int, device, dtype=torch.float16) -> None:
        """Pre-build the position-indexed cos/sin cache (a decode step then needs one gather per table
        instead of seven elementwise launches).  Entries are computed by exactly the ops of the direct
        path, so both paths return identical values.  Call before graph capture."""
        c = self._cache
        if c is not None and c[0].shape[0] >= max_positions and c[0].device == torch.device(device) and c[0].dtype == dtype:
            return
        self._cache = self._tables(torch.arange(max_positions, device=device), dtype)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, position_ids: torch.Tensor):
        """``(cos, sin)`` shaped ``[batch, seq, head_dim]`` in ``x.dtype``."""
        c = self._cache
        if (c is not None and position_ids.shape[1] == 1 and c[0].dtype == x.dtype and c[0].device == x.device):
            # decode: hand out the position-indexed tables themselves; the fused rope kernel reads row
            # positions[i] (callers guarantee positions < the size given to ``ensure``)
            return RopeTables(c[0], c[1], position_ids.reshape(-1))
        return self._tables(position_ids, x.dtype)


# ------------------------------------------------------------------------------------- #
# attention
# ------------------------------------------------------------------------------------- #
# A/B knob for measurements: keep rope + KV scatter and flash_decoding as two launches
_TWO_CALL_ATTENTION = os.environ.get("LL_TWO_CALL_ATTENTION", "0") == "1"
_Q8_FUSION = os.environ.get("LL_NO_Q8_FUSION", "0") != "1"  # smoothquant: quantiser inside the norm launch (A/B knob)


def shared_prefix_route(atten_info, is_prefill: bool) -> bool:
    """Whether this step's attention takes the shared-prefix decode route: a decode step (not a chunk step) whose metadata
    names a shared prefix of at least ``SHARED_PREFIX_MIN_LEN`` positions (the measured routing threshold, read at call
    time; never below the kernel's one 64-key tile)."""
    plen = int(getattr(atten_info, "shared_prefix_len", 0) or 0)
    if plen <= 0 or is_prefill or getattr(atten_info, "b_ctx_len", None) is not None:
        return False
    return plen >= max(_attention_kernels.SHARED_PREFIX_MIN_LEN, 64) and int(atten_info.max_actual_seq_len) >= plen


class PagedAttention(nn.Module):
    """KV scatter + phase kernel over the token-attention pool ``[max_tokens, 2*Hkv, D]``
    (K heads first, then V heads) -- base.py:50-142."""

    def __init__(self, num_kv_heads: int, head_dim: int):
        super().__init__()
        self.num_kv_heads = num_kv_heads
        self.head_dim = head_dim
        self.scale = 1.0 / math.sqrt(head_dim)

    def forward(self, xq, xkv, atten_info, layer_index: int, is_prefill: bool, cached: bool = False):
        """``xkv [n, 2*Hkv, D]`` = this step's K heads then V heads (the pool's row layout), possibly
        a strided view of the fused projection output; ``cached``: already scattered to the pool."""
        pool = atten_info.kv_buffer[layer_index]
        chunked = getattr(atten_info, "b_ctx_len", None) is not None  # a step that continues cached sequences
        if pool.element_size() == 1:
            # fp8 KV cache (extension): quantising scatter, then -- decode -- attention over the e4m3 pool; the prefill
            # attention reads the fresh fp16 q / k / v as always
            ks, vs = getattr(atten_info, "kv_scales", (1.0, 1.0))
            if cached:
                raise ValueError("an fp8 KV pool is written by update_kv_buffer_fp8 only (no fused rope + scatter)")
            update_kv_buffer_fp8(xkv, atten_info.cur_select_index, pool, self.num_kv_heads, ks, vs)
            if chunked:
                return self._paged_prefill(xq, pool, atten_info, (ks, vs))
            if not is_prefill:
                return flash_decoding_fp8kv(xq, pool[:, : self.num_kv_heads, :], pool[:, self.num_kv_heads :, :], self.scale,
                                            atten_info.b_req_tokens_table, atten_info.b_req_idx, atten_info.b_seq_len,
                                            atten_info.max_actual_seq_len, ks, vs)
        elif not cached:
            update_kv_buffer(xkv, atten_info.cur_select_index, atten_info.kv_buffer[layer_index])
        if chunked:
            return self._paged_prefill(xq, pool, atten_info)
        if is_prefill:
            xk, xv = xkv[:, : self.num_kv_heads], xkv[:, self.num_kv_heads :]
            return flash_attention2_no_pad(xq, xk, xv, self.scale * _LOG2E, atten_info.b_start_loc,
                                           atten_info.b_seq_len, atten_info.max_actual_seq_len)
        kv = atten_info.kv_buffer[layer_index]
        if shared_prefix_route(atten_info, is_prefill):
            # the batch shares its first positions (same pool rows in every table row): their K/V are read once per query
            # tile; None = shape not served, the ordinary route reads the aliased table as it is
            out = shared_prefix_decode_attention(xq, kv[:, : self.num_kv_heads, :], kv[:, self.num_kv_heads :, :], self.scale,
                                                 atten_info.b_req_tokens_table, atten_info.b_req_idx, atten_info.b_seq_len,
                                                 atten_info.max_actual_seq_len, atten_info.shared_prefix_len,
                                                 atten_info.shared_prefix_req)
            if out is not None:
                return out
        return flash_decoding(xq, kv[:, : self.num_kv_heads, :], kv[:, self.num_kv_heads :, :], self.scale,
                              atten_info.b_req_tokens_table, atten_info.b_req_idx, atten_info.b_seq_len,
                              atten_info.max_actual_seq_len)


    def _paged_prefill(self, xq, pool, atten_info, kv_scales=(1.0, 1.0)):
        """Chunk step (``b_ctx_len`` set, any chunk width, 1 included): the new tokens are in the pool, every query
        attends over its sequence's cached and new positions through the table."""
        return prefill_paged_attention(xq, pool, self.scale * _LOG2E, atten_info.b_req_tokens_table, atten_info.b_req_idx,
                                       atten_info.b_start_loc, atten_info.b_seq_len, atten_info.b_ctx_len,
                                       atten_info.max_actual_seq_len, atten_info.max_ctx_len, kv_scales)


class Attention(nn.Module):
    """q/kv column-parallel, o row-parallel (one all-reduce) -- base.py:145-245."""

    def __init__(self, geo: ModelGeometry, quant: QuantConfig | None):
        super().__init__()
        tp = get_tp_world_size()
        plan = shard_plan(geo, quant)
        if plan is None:
            self.num_heads = divide(geo.num_heads, tp, "attention heads")
            self.num_kv_heads = divide(geo.num_kv_heads, tp, "key/value heads")
            lq = lkv = None
        else:  # extension: uneven query heads, replicated KV heads
            self.num_heads = plan.q_heads[get_tp_rank()][1]
            self.num_kv_heads = plan.kv_heads[get_tp_rank()][1]
            lq, lkv = self.num_heads * geo.head_dim, 2 * self.num_kv_heads * geo.head_dim
        self.head_dim = geo.head_dim
        self.hidden_size = geo.hidden_size
        self.q_size = self.num_heads * self.head_dim
        self.kv_size = self.num_kv_heads * self.head_dim
        self.eps = geo.rms_norm_eps
        self.use_qk_norm = geo.use_qk_norm
        self.q_proj = ColumnParallelLinear(geo.hidden_size, geo.q_size, bias=geo.qkv_bias, quant=quant,
                                           what="query features", local_size=lq)
        self.kv_proj = ColumnParallelLinear(geo.hidden_size, 2 * geo.kv_size, bias=geo.qkv_bias, quant=quant,
                                            what="key/value features", local_size=lkv)
        self.o_proj = RowParallelLinear(geo.q_size, geo.hidden_size, quant=quant, what="query features", local_size=lq)
        if self.use_qk_norm:
            self.q_norm_weight = nn.Parameter(torch.ones(self.head_dim, dtype=torch.float16), requires_grad=False)
            self.k_norm_weight = nn.Parameter(torch.ones(self.head_dim, dtype=torch.float16), requires_grad=False)
        self.attn = PagedAttention(self.num_kv_heads, self.head_dim)
        object.__setattr__(self, "_qkv", MergedColumnLinear([self.q_proj, self.kv_proj]))

    def forward(self, x, atten_info, layer_index, position_embeddings, partials_ok=False):
        batch, seq_len, _ = x.shape
        x2 = x.view(-1, self.hidden_size)
        fp8_pool = atten_info.kv_buffer[layer_index].element_size() == 1  # extension: e4m3 KV cache, unfused route
        # Qwen3: the per-head q / k RMSNorm rides inside the one-launch decode attention (head size 128)
        qk_norm = (self.q_norm_weight, self.k_norm_weight, self.eps) if self.use_qk_norm else None
        norm_fused = qk_norm is None or (self.head_dim == 128 and not os.environ.get("LL_NO_FUSED_QK_NORM"))
        # smoothquant q|k|v planes are int32: the attention launch only takes them for head size 128, an fp16 pool and no head
        # norm -- known before the projection runs, so other geometries keep the finished projection (the
        # planes GEMM + a torch finish on every step otherwise, and a bias added after the first rounding)
        chunked = getattr(atten_info, "b_ctx_len", None) is not None  # chunk step: b_seq_len counts new tokens only
        # a decode step over a shared prompt prefix: rope + KV scatter, then PagedAttention's shared-prefix route
        two_call = _TWO_CALL_ATTENTION or (
            seq_len == 1 and shared_prefix_route(atten_info, False)
            and shared_prefix_supported(x.dtype, atten_info.kv_buffer[layer_index].dtype, self.num_heads, self.num_kv_heads,
                                        self.head_dim, atten_info.shared_prefix_len, atten_info.max_actual_seq_len))
        int32_planes_ok = not getattr(self.q_proj.quant_method, "takes_int8_rows", False) or (
            self.head_dim == 128 and qk_norm is None and atten_info.kv_buffer[layer_index].dtype == torch.float16)
        if (seq_len == 1 and not chunked and norm_fused and not two_call and isinstance(position_embeddings, RopeTables)
                and not fp8_pool and int32_planes_ok and self._qkv.refresh() and not os.environ.get("LL_NO_QKV_PARTIALS")
                and decode_attention_partials_supported(atten_info.max_actual_seq_len, self.num_heads, self.num_kv_heads,
                                                        self.head_dim, batch=x2.shape[0])):
            # decode, int4, TP = 1: the fused q|k|v projection leaves fp32 split-K partials and the one-launch attention
            # adds them up (+ bias) while its first K/V gathers are in flight -- the GEMM has no merge at all
            pq = self._qkv.partials(x2)
            if pq is not None:
                tables = position_embeddings
                out = decode_attention_partials(pq[0], pq[1], self.num_heads, self.num_kv_heads, self.head_dim, tables[0],
                                                tables[1], tables[2], atten_info.cur_select_index,
                                                atten_info.kv_buffer[layer_index], self.attn.scale,
                                                atten_info.b_req_tokens_table, atten_info.b_req_idx, atten_info.b_seq_len,
                                                atten_info.max_actual_seq_len, qk_norm=qk_norm)
                if out is not None:
                    return self.o_proj(out.view(batch, seq_len, self.q_size), partials_ok)
                # not served (context outside 129..1024 tokens, ...): finish the sums and take the ordinary route
                if isinstance(pq[0], ScaledInt32Partials):
                    # one rounding, the bias added in fp32 like smoothquant_matmul's epilogue (w8a8.py:118-149)
                    sp = pq[0]
                    qkv = ScaledInt32Partials(sp.parts, sp.shape, sp.a_scale, sp.w_scale,
                                              bias=pq[1] if pq[1] is not None else sp.bias).materialise()
                else:
                    qkv = pq[0].materialise() if pq[1] is None else (pq[0].parts.sum(0) + pq[1].float()).to(pq[0].dtype)
                xq, xkv = torch.split(qkv.view(-1, self.q_size + 2 * self.kv_size), [self.q_size, 2 * self.kv_size], dim=-1)
            else:
                xq, xkv = self._qkv(x2)
        elif self._qkv.refresh():
            xq, xkv = self._qkv(x2)  # one launch; strided column views of [n, q + 2 kv]
        else:
            xq = self.q_proj(x2)
            xkv = self.kv_proj(x2)
        n = batch * seq_len
        xq = xq.view(n, self.num_heads, self.head_dim)
        xkv = xkv.view(n, 2 * self.num_kv_heads, self.head_dim)
        xk, xv = xkv[:, : self.num_kv_heads], xkv[:, self.num_kv_heads :]
        tables = position_embeddings if isinstance(position_embeddings, RopeTables) else None
        dense_rows = xkv.stride(1) == self.head_dim and xq.stride(1) == self.head_dim and not fp8_pool
        if dense_rows and norm_fused and tables is not None and seq_len == 1 and not chunked and not two_call:
            # decode: (q / k head norm +) rope + KV scatter + attention + partition merge in ONE launch
            out = decode_attention(xq, xkv, tables[0], tables[1], tables[2], atten_info.cur_select_index,
                                   atten_info.kv_buffer[layer_index], self.attn.scale, atten_info.b_req_tokens_table,
                                   atten_info.b_req_idx, atten_info.b_seq_len, atten_info.max_actual_seq_len,
                                   qk_norm=qk_norm)
            if out is not None:
                return self.o_proj(out.view(batch, seq_len, self.q_size), partials_ok)
        if self.use_qk_norm:
            xq, _ = skip_rmsnorm(xq, None, self.q_norm_weight, self.eps)
            xk, _ = skip_rmsnorm(xk, None, self.k_norm_weight, self.eps)
        fused = not self.use_qk_norm and dense_rows
        if tables is not None and not fused:
            position_embeddings = tables.materialise()
        if fused and tables is not None:
            # rope (position-indexed tables) + KV scatter in one launch, in place
            rope_and_cache(xq, xkv, tables[0], tables[1], batch, seq_len, atten_info.cur_select_index,
                           atten_info.kv_buffer[layer_index], positions=tables[2])
            out = self.attn(xq, xkv, atten_info, layer_index, is_prefill=seq_len > 1, cached=True)
            return self.o_proj(out.view(batch, seq_len, self.q_size))
        cos, sin = position_embeddings
        if fused:
            # rope + KV scatter in one launch, in place on the projection output
            rope_and_cache(xq, xkv, cos, sin, batch, seq_len, atten_info.cur_select_index,
                           atten_info.kv_buffer[layer_index])
            out = self.attn(xq, xkv, atten_info, layer_index, is_prefill=seq_len > 1, cached=True)
        else:
            xq, xk = rope_emb_forward(xq, xk, cos, sin, batch, seq_len)
            if xk.data_ptr() != xkv.data_ptr():  # rope returned a copy of k: rebuild the [K heads | V heads] row
                xkv = torch.cat([xk, xv], dim=-2)
            out = self.attn(xq, xkv, atten_info, layer_index, is_prefill=seq_len > 1)
        return self.o_proj(out.view(batch, seq_len, self.q_size))


def _takes_int8_rows(*linears) -> bool:
    """Whether every one of these projections reads smoothquant-quantised rows (so the norm in front of them can run the
    per-token quantiser itself and hand over ``Int8Rows``)."""
    return _Q8_FUSION and all(getattr(l.quant_method, "takes_int8_rows", False) for l in linears)


def add_norm(hidden_states, residual, weight, eps, q8: bool = False):
    """``skip_rmsnorm`` that also accepts a projection left as split-K partials (kernels/norm_act.py::PartialSums).
    ``q8`` (smoothquant blocks): the consumer reads per-token int8 rows -- the quantiser runs inside the norm launch and the
    result is an ``Int8Rows``."""
    if isinstance(hidden_states, ScaledInt32Partials):
        s_count, _, width = hidden_states.parts.shape
        # rows wider than 4096 keep four 8-value vectors per thread: more than 4 planes of them do not fit the register
        # file at a useful occupancy (307 / 396 registers for 8 / 12 planes) -- finish those sums first
        if width % 8 == 0 and width <= 8192 and (width <= 4096 or s_count <= 4):
            return skip_rmsnorm_q8(hidden_states, residual, weight, eps, quantize=q8)
        hidden_states = hidden_states.materialise()
    if (q8 and torch.is_tensor(hidden_states) and hidden_states.is_cuda and hidden_states.dtype == torch.float16
            and hidden_states.shape[-1] % 8 == 0 and hidden_states.shape[-1] <= 8192):
        return skip_rmsnorm_q8(hidden_states, residual, weight, eps)
    if isinstance(hidden_states, PartialSums):
        return skip_rmsnorm_partials(hidden_states, residual, weight, eps)
    return skip_rmsnorm(hidden_states, residual, weight, eps)


class FusedMLP(nn.Module):
    """down(silu(gate(x)) * up(x)) -- base.py:248-264."""

    def __init__(self, geo: ModelGeometry, quant: QuantConfig | None):
        super().__init__()
        h, i = geo.hidden_size, geo.intermediate_size
        plan = shard_plan(geo, quant)
        li = None if plan is None else plan.inter[get_tp_rank()][1]
        self.gate_proj = ColumnParallelLinear(h, i, quant=quant, what="MLP intermediate", local_size=li)
        self.up_proj = ColumnParallelLinear(h, i, quant=quant, what="MLP intermediate", local_size=li)
        self.down_proj = RowParallelLinear(i, h, quant=quant, what="MLP intermediate", local_size=li)
        object.__setattr__(self, "_gate_up", MergedColumnLinear([self.gate_proj, self.up_proj], interleave=True))

    def forward(self, x, partials_ok=False):
        if self._gate_up.refresh():
            return self.down_proj(self._gate_up.swiglu(x), partials_ok)  # one launch (int4 decode) or merged GEMM + swiglu
        return self.down_proj(swiglu_forward(self.gate_proj(x), self.up_proj(x)), partials_ok)


class SparseMoeBlock(nn.Module):
    """Top-k routed experts, TP-sharded on the expert intermediate dim -- qwen3_moe.py:60-111.
    Router: fp16 linear -> fp32 softmax over ALL experts -> top-k -> renormalise."""

    def __init__(self, geo: ModelGeometry, quant: QuantConfig | None):
        super().__init__()
        self.register_state_dict_post_hook(SparseMoeBlock._export_stacked_gate_up)
        self.register_load_state_dict_pre_hook(SparseMoeBlock._refuse_load_into_interleaved)
        tp = get_tp_world_size()
        self.hidden_size = geo.hidden_size
        self.num_experts = geo.num_experts
        self.top_k = geo.num_experts_per_tok
        self.norm_topk_prob = geo.norm_topk_prob
        self.moe_intermediate_size = divide(geo.moe_intermediate_size, tp, "MoE intermediate")
        # Extension: a shard that cuts the checkpoint's scale blocks -- Qwen3-30B-A3B's 768 channels over 4 / 8
        # ranks = 192 / 96 -- keeps the block's scale value on a finer grid of cut = gcd(block, shard) channels: gate|up's
        # grid is refined along N, down's along K (the loader / quantise-then-cut path repeats every scale block / cut
        # times, weights.py::expand_scale_grid).  Same dequantised weights, so the ranks still partition the unsharded model.
        self.scale_cut = 0
        if quant is not None and not quant.shard_is_aligned(self.moe_intermediate_size):
            block = max(quant.group_n, quant.group_k)
            cut = math.gcd(block, self.moe_intermediate_size)
            if quant.is_int4 or quant.group_n != quant.group_k or cut % 8 != 0:
                raise ValueError(
                    f"tensor-parallel shard of MoE intermediate is {self.moe_intermediate_size} channels, which is not "
                    f"a multiple of the {quant.format} scale block ({quant.group_n}x{quant.group_k}); "
                    "use a smaller tensor_parallel_size"
                )
            self.scale_cut = cut
        self.quant = quant
        self.quant_method = get_moe_method(quant)
        self.gate_weight = nn.Parameter(torch.empty(self.num_experts, self.hidden_size, dtype=torch.float16),
                                        requires_grad=False)
        self.experts = nn.ParameterDict(self.quant_method.create_weights(self))

    def _route(self, x):
        """``(weights, ids, aligned)``: ``aligned`` is ``moe_align_block_size`` of the ids when the router's launch produced it
        (decode batches: gate GEMM + tail + align in-tree, round 6), else ``None``."""
        if x.is_cuda and x.shape[0] <= 64 and self.top_k <= 64 and not os.environ.get("LL_MOE_LIBRARY_GATE"):
            from .kernels.fused_moe import fused_moe_block_m, moe_router
            routed = moe_router(x, self.gate_weight, self.top_k, self.norm_topk_prob, align_block=fused_moe_block_m(x.shape[0]))
            if routed is not None:
                return routed
        return (*self._route_library_gate(x), None)

    def _route_library_gate(self, x):
        logits = F.linear(x, self.gate_weight)
        if logits.is_cuda and self.num_experts <= 1024 and self.top_k <= 64 and not os.environ.get("LL_MOE_TORCH_ROUTER"):
            from .kernels.fused_moe import moe_route_topk
            return moe_route_topk(logits, self.top_k, self.norm_topk_prob)  # softmax + top-k + renorm + cast: one launch
        probs = torch.softmax(logits, dim=-1, dtype=torch.float32)
        w, ids = torch.topk(probs, self.top_k, dim=-1)
        if self.norm_topk_prob:
            w = w / w.sum(dim=-1, keepdim=True)
        return w, ids

    def forward(self, x, partials_ok: bool = False):
        """``partials_ok`` (extension, TP = 1): the caller's add-and-normalise adds the top-k slots up itself -- the result is a
        ``SlotSums`` and the ``moe_sum`` launch is skipped."""
        shape = x.shape
        x2 = x.reshape(-1, self.hidden_size)
        w, ids, aligned = self._route(x2)
        slots = (partials_ok and get_tp_world_size() == 1 and x2.is_cuda and not os.environ.get("LL_MOE_NO_SLOTS"))
        out = self.quant_method.apply(self, x2, w, ids, slots_ok=bool(slots), aligned=aligned)
        if isinstance(out, PartialSums):
            out.shape = tuple(shape)
            return out
        return all_reduce_tp(out).view(shape)

    # ---- load-time interleave of the stacked gate|up rows (round 5) ------------------------------------------------------
    @staticmethod
    def _export_stacked_gate_up(module, state_dict, prefix, local_metadata):
        """state_dict post-hook: an interleaved block EXPORTS the checkpoint's stacked order (fresh tensors; the block and the
        graphs captured over it are not touched -- ADVICE round 5)."""
        if getattr(module, "_gu_interleaved", False):
            w, sc = module.stacked_gate_up()
            for key, val in ((prefix + "experts.gate_up_proj", w), (prefix + "experts.gate_up_proj_scale_inv", sc)):
                if val is not None and key in state_dict:
                    state_dict[key] = val.detach()

    @staticmethod
    def _refuse_load_into_interleaved(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """load_state_dict pre-hook: stacked checkpoint rows copied into interleaved storage (same shapes with per-channel
        scales) would be multiplied as pairs -- silently wrong.  ``CausalLM.load_state_dict`` expands first."""
        if getattr(module, "_gu_interleaved", False) and (prefix + "experts.gate_up_proj") in state_dict:
            raise RuntimeError(f"{prefix}experts.gate_up_proj is row-interleaved (compact_weights): call model.expand_weights() "
                               "before loading a checkpoint into it")

    @torch.no_grad()
    def interleave_gate_up_(self) -> bool:
        """Re-order the rows of ``experts.gate_up_proj`` from the checkpoint's stacked halves ``[gate_0.. | up_0..]`` to pairs
        ``(gate_j, up_j)`` IN PLACE (same storage, a permutation of the same rows; scales follow: per-row grids are permuted,
        coarser blocks along N are first repeated down to one value per row), so that ``silu(gate) * up`` runs in the epilogue
        of the first grouped GEMM (``fused_moe(..., w1_interleaved=True)``): one launch and a ``[slots, 2 I]`` round trip less
        per layer.  Like ``CausalLM.compact_weights`` this changes what ``state_dict()`` would export:
        ``deinterleave_gate_up_`` (called by ``expand_weights``) restores the checkpoint order bit for bit."""
        if getattr(self, "_gu_interleaved", False) or os.environ.get("LL_MOE_NO_INTERLEAVE"):
            return False
        w = self.experts["gate_up_proj"]
        if not w.is_cuda or torch.cuda.is_current_stream_capturing():
            return False
        e, two_i, h = w.shape
        i = two_i // 2
        w.data.copy_(torch.stack((w.data[:, :i], w.data[:, i:]), dim=2).reshape(e, two_i, h))
        key = "gate_up_proj_scale_inv"
        if key in self.experts:
            sc = self.experts[key].data
            gn = -(-two_i // sc.shape[1])  # rows per scale value along N
            self._gu_scale_rows = gn
            if gn > 1:
                sc = sc.repeat_interleave(gn, dim=1)[:, :two_i]
            sc = torch.stack((sc[:, :i], sc[:, i:]), dim=2).reshape(e, two_i, -1).contiguous()
            if gn > 1:
                # (block scales grow from one value per gn rows to one per row: e.g. 128 x 128 fp8 blocks of Qwen3-30B-A3B,
                # 4.7 MB -> ~600 MB resident -- the price of pairing rows that sit in different scale blocks)
                self.experts[key] = nn.Parameter(sc, requires_grad=False)
            else:
                self.experts[key].data.copy_(sc)
        self._gu_interleaved = True
        return True

    def stacked_gate_up(self):
        """``(gate_up_proj, gate_up_proj_scale_inv or None)`` in the CHECKPOINT's stacked order, as fresh tensors when the
        block is interleaved (the block itself is not touched) -- what ``state_dict()`` exports."""
        w = self.experts["gate_up_proj"].data
        key = "gate_up_proj_scale_inv"
        sc = self.experts[key].data if key in self.experts else None
        if not getattr(self, "_gu_interleaved", False):
            return w, sc
        e, two_i, h = w.shape
        i = two_i // 2
        pairs = w.view(e, i, 2, h)
        w = torch.cat((pairs[:, :, 0], pairs[:, :, 1]), dim=1)
        if sc is not None:
            pairs = sc.view(e, i, 2, -1)
            sc = torch.cat((pairs[:, :, 0], pairs[:, :, 1]), dim=1).contiguous()
            gn = getattr(self, "_gu_scale_rows", 1)
            if gn > 1:
                sc = sc[:, ::gn].contiguous()
        return w, sc

    @torch.no_grad()
    def deinterleave_gate_up_(self) -> None:
        if not getattr(self, "_gu_interleaved", False):
            return
        w, sc = self.stacked_gate_up()
        self.experts["gate_up_proj"].data.copy_(w)
        key = "gate_up_proj_scale_inv"
        if sc is not None:
            if getattr(self, "_gu_scale_rows", 1) > 1:
                self.experts[key] = nn.Parameter(sc, requires_grad=False)
            else:
                self.experts[key].data.copy_(sc)
        self._gu_interleaved = False

    @torch.no_grad()
    def quantize_experts_(self, quant: QuantConfig) -> None:
        if self.quant is not None:
            return
        method = get_moe_method(quant)
        method.convert_from_fp16(self, quant)
        self.quant, self.quant_method = quant, method


class DecoderLayer(nn.Module):
    """Pre-norm block with the fused add-and-normalise threading ``residual`` -- base.py:267-319."""

    def __init__(self, geo: ModelGeometry, quant: QuantConfig | None):
        super().__init__()
        self.eps = geo.rms_norm_eps
        self.input_layernorm_weight = nn.Parameter(torch.ones(geo.hidden_size, dtype=torch.float16), requires_grad=False)
        self.post_attention_layernorm_weight = nn.Parameter(torch.ones(geo.hidden_size, dtype=torch.float16),
                                                            requires_grad=False)
        self.self_attn = Attention(geo, quant)
        self.mlp = SparseMoeBlock(geo, quant) if geo.num_experts else FusedMLP(geo, quant)

    def forward(self, hidden_states, atten_info, layer_index, position_embeddings, residual=None):
        """``hidden_states`` in and out may be a :class:`PartialSums` (decode, int4, TP = 1): the row-parallel
        projections leave fp32 split-K partials and the add-and-normalise that follows adds them up."""
        hidden_states, residual = add_norm(hidden_states, residual, self.input_layernorm_weight, self.eps,
                                           q8=_takes_int8_rows(self.self_attn.q_proj, self.self_attn.kv_proj))
        hidden_states = self.self_attn(hidden_states, atten_info, layer_index, position_embeddings, partials_ok=True)
        hidden_states, residual = add_norm(hidden_states, residual, self.post_attention_layernorm_weight, self.eps,
                                           q8=isinstance(self.mlp, FusedMLP)
                                           and _takes_int8_rows(self.mlp.gate_proj, self.mlp.up_proj))
        hidden_states = self.mlp(hidden_states, partials_ok=True)
        return hidden_states, residual


class CausalLM(nn.Module):
    """token ids -> logits (base.py:322-489).  Embedding, final norm and ``lm_head`` are fp16 and
    replicated under TP (every rank computes full logits and the same argmax)."""

    def __init__(self, geo: ModelGeometry, quant: QuantConfig | None = None):
        super().__init__()
        self.geo = geo
        self.quant = quant
        self.layout_epoch = 0  # moves with every compact / expand: graphs captured under another epoch are stale
        self.shard_plan = shard_plan(geo, quant)  # None: the reference's equal cuts
        set_active_plan(self.shard_plan, geo.num_heads, geo.num_kv_heads, geo.intermediate_size)
        self.embed_tokens = nn.Embedding(geo.vocab_size, geo.hidden_size, dtype=torch.float16)
        self.embed_tokens.weight.requires_grad_(False)
        self.layers = nn.ModuleList(DecoderLayer(geo, quant) for _ in range(geo.num_layers))
        self.norm_weight = nn.Parameter(torch.ones(geo.hidden_size, dtype=torch.float16), requires_grad=False)
        if geo.tie_word_embeddings:
            self.lm_head_weight = self.embed_tokens.weight
        else:
            self.lm_head_weight = nn.Parameter(torch.empty(geo.vocab_size, geo.hidden_size, dtype=torch.float16),
                                               requires_grad=False)
        self.rotary_emb = RotaryEmbedding(geo)
        self.eps = geo.rms_norm_eps

    @torch.no_grad()
    def forward(self, input_ids, position_ids, atten_info, logits_rows=None):
        """``[batch, seq]`` ids -> ``[batch, seq, vocab]`` fp16 logits.  ``logits_rows`` (extension:
        flat token indices) restricts the lm_head to those rows -- prefill only needs the last
        prompt position of every sequence, not ``batch*seq*vocab`` logits."""
        hidden_states = self.final_hidden_states(input_ids, position_ids, atten_info)
        if logits_rows is not None:
            hidden_states = hidden_states.view(-1, hidden_states.shape[-1])[logits_rows]
        return self.logits_from_hidden(hidden_states)

    @torch.no_grad()
    def final_hidden_states(self, input_ids, position_ids, atten_info):
        """First half of :meth:`forward`: ``[batch, seq]`` ids -> the normalised final hidden states ``[batch, seq, hidden]``
        (everything up to and including the final norm)."""
        hidden_states = self.embed_tokens(input_ids)
        position_embeddings = self.rotary_emb(hidden_states, position_ids)
        residual = None
        for i, layer in enumerate(self.layers):
            hidden_states, residual = layer(hidden_states, atten_info, i, position_embeddings, residual)
        hidden_states, _ = add_norm(hidden_states, residual, self.norm_weight, self.eps)
        return hidden_states

    @torch.no_grad()
    def logits_from_hidden(self, hidden_states):
        """Second half of :meth:`forward`: normalised hidden rows ``[..., hidden]`` -> logits ``[..., vocab]`` (the lm_head);
        callers that need the logits of many rows take them a bounded number of rows at a time."""
        if hidden_states.is_cuda and not os.environ.get("LL_LM_HEAD_LIBRARY"):
            from .kernels.quantization import dense16_linear, dense16_rows_linear, dense16_rows_wins
            rows = hidden_states.numel() // hidden_states.shape[-1]
            if dense16_rows_wins(rows, self.lm_head_weight.shape[0], self.lm_head_weight.shape[1]):
                logits = dense16_rows_linear(hidden_states, self.lm_head_weight)  # the row-group loop (round 5): 5.3 - 5.8 TB/s
                if logits is not None:
                    return logits
            logits = dense16_linear(hidden_states, self.lm_head_weight, policy="auto")
            if logits is not None:
                return logits
        return F.linear(hidden_states, self.lm_head_weight)

    @torch.no_grad()
    def quantize_(self, quant: QuantConfig) -> None:
        """Convert every fp16 projection to ``quant`` in place (the ``--quantization`` path)."""
        for m in self.modules():
            if isinstance(m, LinearBase):
                m.quantize_(quant)
            elif hasattr(m, "quantize_experts_"):
                m.quantize_experts_(quant)
        self.quant = quant

    # --------------------------------------------------------------------------------- #
    # one resident copy of the int4 weights (round 4; VERDICT round 3 "weak" 7)
    # --------------------------------------------------------------------------------- #
    def _merged_linears(self):
        return [v for mod in self.modules() for v in vars(mod).values() if hasattr(v, "compact") and hasattr(v, "refresh")]

    @torch.no_grad()
    def compact_weights(self) -> int:
        """The decode engine streams int4 weights from a load-time layout that used to sit NEXT to the reference-format
        parameter (2 x 0.5 B per weight).  After this call the load-time layout is the only resident copy: the parameters
        alias it (same shapes / dtypes, permuted words), the reference-format tensors are rebuilt on demand for calls of more
        than 64 rows (prefill) -- ``W4A16LinearMethod.reference_weight``.  Call after the weights are final (after loading /
        quantising) and BEFORE any decode step is captured: the int4 storage a captured graph points at does not move, but a MoE
        block's gate|up rows are re-ordered in place for the fused epilogue, and a graph captured over the stacked rows would
        replay over pairs -- ``layout_epoch`` moves with every layout change and ``StepGraphs`` drops the graphs it cached under
        another epoch (``DecodeEngine.decode`` captures per call); a graph the CALLER captured is the caller's to drop.  Returns
        the bytes released.
        ``state_dict()`` of a compacted model still exports the reference layouts (rebuilt per entry, nothing is mutated);
        ``expand_weights()`` undoes the compaction (``load_state_dict`` calls it first)."""
        freed = sum(mc.compact() for mc in self._merged_linears())
        for m in self.modules():
            if isinstance(m, LinearBase) and hasattr(m.quant_method, "compact"):  # (members of a compacted holder: 0)
                freed += m.quant_method.compact(m)
            if isinstance(m, SparseMoeBlock):
                if m.interleave_gate_up_():  # (frees nothing: rows re-ordered for the fused epilogue; block scales GROW, see there)
                    self.layout_epoch += 1
        if freed:
            self.layout_epoch += 1
            torch.cuda.empty_cache()
        return freed

    def is_compacted(self) -> bool:
        return any(getattr(m, "_gu_interleaved", False) for m in self.modules() if isinstance(m, SparseMoeBlock)) or \
            any(holds_packed(m) for m in self.modules() if isinstance(m, LinearBase))  # (a compacted holder's members: too)

    # (state_dict(): the per-module post-hooks -- linear.py::_export_reference_weight, SparseMoeBlock._export_stacked_gate_up --
    # export reference layouts from a compacted model without touching it)

    def load_state_dict(self, state_dict, *args, **kwargs):
        """Checkpoint tensors are in the reference layouts: a compacted model is expanded first (``layout_epoch`` moves, so
        engines drop the graphs captured over the compacted storage); compact again afterwards."""
        if self.is_compacted():
            self.expand_weights()
        return super().load_state_dict(state_dict, *args, **kwargs)

    @torch.no_grad()
    def expand_weights(self) -> None:
        """Undo ``compact_weights``: fresh reference-format int4 tensors, MoE rows back in the stacked order.  Graphs captured
        over the compacted storage are stale afterwards (``layout_epoch`` moves; engines re-capture)."""
        if self.is_compacted():
            self.layout_epoch += 1
        for mc in self._merged_linears():
            mc.expand()
        for m in self.modules():
            if isinstance(m, LinearBase) and hasattr(m.quant_method, "expand"):
                m.quant_method.expand(m)
            if isinstance(m, SparseMoeBlock):
                m.deinterleave_gate_up_()

    def weight_bytes(self) -> int:
        """Bytes of every distinct parameter / derived-layout storage the model keeps resident (aliases counted once)."""
        seen, total = set(), 0

        def add(t):
            nonlocal total
            if isinstance(t, torch.Tensor) and t.is_cuda:
                st = t.untyped_storage()
                if st.data_ptr() not in seen:
                    seen.add(st.data_ptr())
                    total += st.nbytes()

        for p_ in self.parameters():
            add(p_)
        holders = [mc._holder for mc in self._merged_linears() if mc._holder is not None]
        for obj in list(self.modules()) + holders:
            for t in derived_tensors(obj) + list(vars(obj).values()):
                add(t)
        return total

    # --------------------------------------------------------------------------------- #
    # synthetic weights (no checkpoints exist offline): seeded, reference quantiser semantics
    # --------------------------------------------------------------------------------- #
    @torch.no_grad()
    def init_synthetic(self, seed: int = 0, quant: QuantConfig | None = None, device="cuda") -> "CausalLM":
        """fp16 masters ``randn * 0.02`` per projection (each TP rank draws the FULL matrix from the
        same seed and keeps its shard, so all ranks hold consistent weights), norms ``1 + 0.1 randn``,
        biases ``0.01 randn``; then quantised layer by layer with the reference quantisers."""
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        tp, rank = get_tp_world_size(), get_tp_rank()

        def randn(*shape, std=0.02):
            return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std).to(torch.float16)

        plan = shard_plan(self.geo, quant if quant is not None else self.quant)

        def shard(full, dim, kind=None):
            """This rank's slice: the reference's equal chunk, or -- extension plan -- the range of its query heads ("q"),
            its KV head ("kv") or its MLP intermediate channels ("inter")."""
            if tp == 1:
                return full
            if plan is None or kind is None:
                return full.chunk(tp, dim=dim)[rank].contiguous()
            start, count = {"q": plan.q_range, "kv": plan.kv_range, "inter": plan.inter_range}[kind](rank)
            return full.narrow(dim, start, count).contiguous()

        def fill_linear(lin: LinearBase, full_out: int, full_in: int, shard_dim: int | None, kind=None):
            w = randn(full_out, full_in)
            w = w if shard_dim is None else shard(w, shard_dim, kind)
            lin.weight = nn.Parameter(w, requires_grad=False)
            if lin.bias is not None:
                b = randn(full_out, std=0.01)
                lin.bias = nn.Parameter(b if shard_dim != 0 else shard(b, 0, kind), requires_grad=False)
            lin.quant, lin.quant_method = None, get_linear_method_for(None)
            if quant is not None:
                lin.quantize_(quant)

        geo = self.geo
        self.to(device)
        self.embed_tokens.weight.copy_(randn(geo.vocab_size, geo.hidden_size))
        if not geo.tie_word_embeddings:
            self.lm_head_weight.copy_(randn(geo.vocab_size, geo.hidden_size))
        self.norm_weight.copy_((1 + 0.1 * torch.randn(geo.hidden_size, generator=g, device=device)).half())
        for layer in self.layers:
            layer.input_layernorm_weight.copy_((1 + 0.1 * torch.randn(geo.hidden_size, generator=g, device=device)).half())
            layer.post_attention_layernorm_weight.copy_(
                (1 + 0.1 * torch.randn(geo.hidden_size, generator=g, device=device)).half())
            at = layer.self_attn
            fill_linear(at.q_proj, geo.q_size, geo.hidden_size, 0, "q")
            # fused kv: each rank takes its slice of k_proj and of v_proj and fuses locally
            # (weights.py:99,166-169): rank r's rows are [K_r ; V_r]
            kw, vw = randn(geo.kv_size, geo.hidden_size), randn(geo.kv_size, geo.hidden_size)
            kv = torch.cat([shard(kw, 0, "kv"), shard(vw, 0, "kv")], dim=0)
            at.kv_proj.weight = nn.Parameter(kv, requires_grad=False)
            if at.kv_proj.bias is not None:
                kb, vb = randn(geo.kv_size, std=0.01), randn(geo.kv_size, std=0.01)
                at.kv_proj.bias = nn.Parameter(torch.cat([shard(kb, 0, "kv"), shard(vb, 0, "kv")]), requires_grad=False)
            at.kv_proj.quant, at.kv_proj.quant_method = None, get_linear_method_for(None)
            if quant is not None:
                at.kv_proj.quantize_(quant)
            fill_linear(at.o_proj, geo.hidden_size, geo.q_size, 1, "q")
            if geo.use_qk_norm:
                at.q_norm_weight.copy_((1 + 0.1 * torch.randn(geo.head_dim, generator=g, device=device)).half())
                at.k_norm_weight.copy_((1 + 0.1 * torch.randn(geo.head_dim, generator=g, device=device)).half())
            if geo.num_experts:
                blk = layer.mlp
                blk.gate_weight.copy_(randn(geo.num_experts, geo.hidden_size))
                e, i_full = geo.num_experts, geo.moe_intermediate_size
                gate = shard(randn(e, i_full, geo.hidden_size, std=1.0 / math.sqrt(geo.hidden_size)), 1)
                up = shard(randn(e, i_full, geo.hidden_size, std=1.0 / math.sqrt(geo.hidden_size)), 1)
                down = shard(randn(e, geo.hidden_size, i_full, std=1.0 / math.sqrt(i_full)), 2)
                blk.quant, blk.quant_method = None, get_moe_method(None)
                blk.experts = nn.ParameterDict({
                    "gate_up_proj": nn.Parameter(torch.cat([gate, up], dim=1), requires_grad=False),
                    "down_proj": nn.Parameter(down, requires_grad=False),
                })
                if quant is not None:
                    blk.quantize_experts_(quant)
            else:
                mlp = layer.mlp
                fill_linear(mlp.gate_proj, geo.intermediate_size, geo.hidden_size, 0, "inter")
                fill_linear(mlp.up_proj, geo.intermediate_size, geo.hidden_size, 0, "inter")
                fill_linear(mlp.down_proj, geo.hidden_size, geo.intermediate_size, 1, "inter")
        self.quant = quant
        return self


def get_linear_method_for(quant):
    from .quantization import get_linear_method

    return get_linear_method(quant)
