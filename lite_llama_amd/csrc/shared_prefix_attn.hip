// Decode attention for a batch whose sequences share their first prefix_len positions (extension): the same pool rows are
// named by every row's table, so over the prefix the batch's queries for one KV head are a MATRIX -- [batch x (hq / hkv), D]
// against K [prefix_len, D] -- and the K/V rows are read once per 64-row query tile instead of once per batch row.
// The result is ll_flash_decoding's: out[b, h] = softmax(q[b, h] . K[rows]^T * scale) V[rows], rows = table[b_req_idx[b],
// :b_seq_len[b]], computed as three launches that meet in fp32 records:
//
//   prefix  sp_prefix: grid (split of the prefix, 64-row tile of the flattened (batch row, head of the group) queries, KV head).
//           The workgroup keeps its Q tile in registers (a wave owns 16 query rows) and walks the 64-key tiles of its split:
//           paged_prefill4's walk (csrc/prefill_paged_attn.hip) without the causal mask -- a tile's table entries are read
//           once, one tile ahead of the K/V gathers, through table[prefix_req] only; S = Q K^T and O += P V on
//           mfma_f32_16x16x32, fp32 running max / sum in log2 units, P rounded to the storage dtype before PV.  Only the
//           prefix's last tile is partial: keys are clamped to prefix_len - 1, their scores dropped and their V rows zeroed.
//           Leaves a normalised fp32 o and lse = m ln2 + log d per (row, head, split): fd_stage1's record.
//   suffix  flash_decoding's stage 1 (fd_stage1_records) over the table shifted by prefix_len and the lengths b_seq_len -
//           prefix_len, which sp_prefix's first workgroup leaves in the workspace (the lengths live on the device).
//   merge   sp_merge: one workgroup per (row, head), fd_stage2's recurrence over the prefix splits, then the valid suffix
//           partitions; one rounding to the q dtype.  A row with an empty tail has no suffix partition: the prefix alone.
//
// No host synchronisation, no allocation: the launches are capturable and the workspace is the caller's.
#include "attn_engines.h"
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct alignas(16) Q4 {
  uint32_t x, y, z, w;
};

template <int DT>
__device__ __forceinline__ f32x4 mfma16(const Q4& a, const Q4& b, f32x4 c) {
  if constexpr (DT == LL_F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                   0);
}

template <int DT>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return (uint32_t)from_f32<DT>(lo) | ((uint32_t)from_f32<DT>(hi) << 16);
}

__device__ __forceinline__ int64_t load_idx(const void* p, int64_t i, int w) {
  return w == LL_I32 ? (int64_t)((const int32_t*)p)[i] : ((const int64_t*)p)[i];
}

constexpr int SP_TQ = 64;          // query rows of a workgroup (flattened batch row x head of the KV group)
constexpr int SP_TK = 64;          // keys of a tile
constexpr int SP_MAX_SPLITS = 64;  // prefix splits a row's merge reads at most
constexpr int SP_PART = 128;       // flash_decoding's partition (the suffix records)

struct SpPlan {
  int qtiles;       // 64-row query tiles per KV head
  int nsplit;       // splits of the prefix
  int64_t split;    // keys per split (a multiple of 64)
  int nparts;       // suffix partitions of the launch
  int64_t pre_o, pre_lse, suf_o, suf_lse, suf_len, floats;  // workspace offsets (floats) and its size
};

// Split length: enough workgroups to fill the CUs where the prefix allows, never below one 64-key tile.
SpPlan sp_plan(int batch, int hq, int hkv, int d, int64_t prefix_len, int64_t max_len) {
  SpPlan p;
  const int groups = hq / hkv;
  p.qtiles = (int)(((int64_t)batch * groups + SP_TQ - 1) / SP_TQ);
  const int64_t tiles = (prefix_len + SP_TK - 1) / SP_TK;
  const int64_t base = (int64_t)hkv * p.qtiles;
  int64_t want = (ll_num_cus() + base - 1) / base;
  if (want > tiles) want = tiles;
  if (want > SP_MAX_SPLITS) want = SP_MAX_SPLITS;
  if (want < 1) want = 1;
  const int64_t per = (tiles + want - 1) / want;
  p.split = per * SP_TK;
  p.nsplit = (int)((tiles + per - 1) / per);
  p.nparts = (int)((max_len - prefix_len + SP_PART - 1) / SP_PART);
  const int64_t rows = (int64_t)batch * hq;
  p.pre_o = 0;
  p.pre_lse = p.pre_o + rows * p.nsplit * d;
  p.suf_o = p.pre_lse + (rows * p.nsplit + 3) / 4 * 4;
  p.suf_lse = p.suf_o + rows * p.nparts * d;
  p.suf_len = p.suf_lse + (rows * p.nparts + 3) / 4 * 4;
  p.floats = p.suf_len + ((int64_t)batch + 3) / 4 * 4;
  return p;
}

bool sp_shape_ok(int batch, int hq, int hkv, int d, int64_t prefix_len, int64_t max_len) {
  return batch >= 0 && batch <= (1 << 20) && hq > 0 && hkv > 0 && hkv <= 65535 && hq % hkv == 0 && hq / hkv <= 16 &&
         (d == 64 || d == 128) && prefix_len >= SP_TK && prefix_len < (1ll << 31) && max_len >= prefix_len &&
         max_len < (1ll << 31);
}

struct SpArgs {
  const int32_t* trow;    // table[prefix_req]
  const void* seq_len;    // b_seq_len [batch]
  int32_t* suf_len;       // out: b_seq_len - prefix_len [batch]
  float *pre_o, *pre_lse;
  int batch, hq, groups, nsplit, seq_w;
  int64_t prefix_len, split;
  float sm_scale;         // qk_scale * log2 e
  int64_t q_sb, q_sh, k_st, k_sh, v_st, v_sh;
};

// grid = (nsplit, qtiles, hkv), block = 256: wave w owns query rows 16 w .. 16 w + 15 of the tile
template <int DT, int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void sp_prefix(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp, SpArgs a) {
  constexpr int NS = D / 32, NT = D / 16, STR = D + 8, TK = SP_TK;
  constexpr int TPR = D / 8, RPP = 256 / TPR, PASSES = TK / RPP;  // 8-element pieces per row, rows per pass
  __shared__ __attribute__((aligned(16))) uint16_t lds_k[TK * STR];
  __shared__ __attribute__((aligned(16))) uint16_t lds_v[TK * STR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, c = lane >> 4;
  const int sp = blockIdx.x, kvh = blockIdx.z;
  const int64_t P = a.prefix_len;

  // the suffix lengths stage 1 reads next (one workgroup writes them; the launches are ordered by the stream)
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    for (int b = tid; b < a.batch; b += 256) {
      const int64_t n = load_idx(a.seq_len, b, a.seq_w) - P;
      a.suf_len[b] = n > 0 ? (int32_t)n : 0;
    }
  }

  const int nrows = a.batch * a.groups;                   // flattened query rows of this KV head
  const int r = (int)blockIdx.y * SP_TQ + wave * 16 + t;  // this lane's query row
  const int rr = r < nrows ? r : nrows - 1;               // rows past the batch: a valid row, never stored
  const int qb = rr / a.groups, qh = kvh * a.groups + rr % a.groups;
  const float sm_scale = a.sm_scale;

  Q4 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = *reinterpret_cast<const Q4*>(q + (int64_t)qb * a.q_sb + (int64_t)qh * a.q_sh + s * 32 + c * 8);
  float m_i = -INFINITY, d_i = 0.f;
  f32x4 ot[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) ot[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t k0 = (int64_t)sp * a.split;                           // this split: keys k0 .. kend - 1 (never empty)
  const int64_t kend = k0 + a.split < P ? k0 + a.split : P;
  const int lrow = tid / TPR, lcol = (tid % TPR) * 8;
  i32x4 kr[PASSES], vr[PASSES];
  auto table_entries = [&](int64_t p0) {  // lane l: the row of key p0 + l (clamped to the prefix's last position)
    const int64_t key = p0 + lane < P ? p0 + lane : P - 1;
    return a.trow[key];
  };
  auto fetch = [&](int tr) {  // tr: this lane's table entry of the tile being fetched
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int64_t row = __shfl(tr, ps * RPP + lrow, 64);
      kr[ps] = *reinterpret_cast<const i32x4*>(kp + row * a.k_st + (int64_t)kvh * a.k_sh + lcol);
      vr[ps] = *reinterpret_cast<const i32x4*>(vp + row * a.v_st + (int64_t)kvh * a.v_sh + lcol);
    }
  };
  auto stage = [&](int64_t p0) {
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int row = ps * RPP + lrow;
      *reinterpret_cast<i32x4*>(&lds_k[row * STR + lcol]) = kr[ps];
      // rows past the prefix are multiplied by p = 0: they must not hold NaN / Inf bit patterns
      *reinterpret_cast<i32x4*>(&lds_v[row * STR + lcol]) = p0 + row < P ? vr[ps] : i32x4{0, 0, 0, 0};
    }
  };
  auto next_tile = [&](int64_t p0) { return p0 + TK < kend ? p0 + TK : p0; };
  const uint16_t* vtr = lds_v + (4 * c + (t >> 2)) * STR + (t & 3) * 4;

  fetch(table_entries(k0));
  int tr = table_entries(next_tile(k0));  // invariant at the top of iteration p0: the entries of next_tile(p0)
  for (int64_t p0 = k0; p0 < kend; p0 += TK) {
    __syncthreads();  // the previous tile's fragment reads are done
    stage(p0);
    __syncthreads();
    const int64_t pn = next_tile(p0);
    fetch(tr);  // tile pn, in flight under this tile's arithmetic (unconditional, as in paged_prefill4)
    tr = table_entries(next_tile(pn));
    f32x4 sacc[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) sacc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const Q4 kf = *reinterpret_cast<const Q4*>(&lds_k[(kb * 16 + t) * STR + s * 32 + c * 8]);
        sacc[kb] = mfma16<DT>(kf, qf[s], sacc[kb]);
      }
    }
    float sc[16];
    if (p0 + TK <= P) {  // whole tile inside the prefix (workgroup-uniform)
#pragma unroll
      for (int j = 0; j < 16; ++j) sc[j] = sacc[j >> 2][j & 3];
    } else {  // the prefix's last tile: key p0 is valid, so the running max stays finite
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t key = p0 + 16 * (j >> 2) + 4 * c + (j & 3);
        sc[j] = key < P ? sacc[j >> 2][j & 3] : -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; j += 2) mx = fmaxf(mx, fmaxf(sc[j], sc[j + 1]));
    mx *= sm_scale;
    mx = rows_max(mx);
    const float m_new = fmaxf(m_i, mx);
    const float alpha = __builtin_amdgcn_exp2f(m_i - m_new);
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      sc[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j], sm_scale, -m_new));
      psum += sc[j];
    }
    psum = rows_sum(psum);
    d_i = d_i * alpha + psum;
    m_i = m_new;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        ot[dt][0] *= alpha; ot[dt][1] *= alpha; ot[dt][2] *= alpha; ot[dt][3] *= alpha;
      }
    }
    Q4 pf[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      pf[hf].x = pack2<DT>(sc[8 * hf + 0], sc[8 * hf + 1]);
      pf[hf].y = pack2<DT>(sc[8 * hf + 2], sc[8 * hf + 3]);
      pf[hf].z = pack2<DT>(sc[8 * hf + 4], sc[8 * hf + 5]);
      pf[hf].w = pack2<DT>(sc[8 * hf + 6], sc[8 * hf + 7]);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        const s16x4 tlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(vtr + (32 * hf) * STR + dt * 16));
        const s16x4 thi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(vtr + (32 * hf + 16) * STR + dt * 16));
        Q4 vf;
        vf.x = (uint32_t)(uint16_t)tlo.x | ((uint32_t)(uint16_t)tlo.y << 16);
        vf.y = (uint32_t)(uint16_t)tlo.z | ((uint32_t)(uint16_t)tlo.w << 16);
        vf.z = (uint32_t)(uint16_t)thi.x | ((uint32_t)(uint16_t)thi.y << 16);
        vf.w = (uint32_t)(uint16_t)thi.z | ((uint32_t)(uint16_t)thi.w << 16);
        ot[dt] = mfma16<DT>(vf, pf[hf], ot[dt]);
      }
    }
  }

  if (r < nrows) {
    const float inv = 1.0f / d_i;
    const int64_t rec = ((int64_t)qb * a.hq + qh) * a.nsplit + sp;
    float* mo = a.pre_o + rec * D;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
      f32x4 o = ot[dt];
      o[0] *= inv; o[1] *= inv; o[2] *= inv; o[3] *= inv;
      *reinterpret_cast<f32x4*>(mo + dt * 16 + 4 * c) = o;
    }
    if (c == 0) a.pre_lse[rec] = m_i * 0.69314718055994530942f + logf(d_i);
  }
}

// grid = (hq, batch), block = d threads: fd_stage2's recurrence over the prefix splits, then the valid suffix partitions
template <int DT>
__global__ void sp_merge(uint16_t* __restrict__ out, const float* __restrict__ pre_o, const float* __restrict__ pre_lse,
                         const float* __restrict__ suf_o, const float* __restrict__ suf_lse,
                         const int32_t* __restrict__ suf_len, int hq, int d, int nsplit, int nparts, int64_t o_sb,
                         int64_t o_sh) {
  const int h = blockIdx.x, b = blockIdx.y;
  const int64_t hrow = (int64_t)b * hq + h;
  int np = (suf_len[b] + SP_PART - 1) / SP_PART;
  if (np > nparts) np = nparts;
  float m_i = -INFINITY, d_i = 0.f, acc = 0.f;
  // records in batches of 8: all 16 loads of a batch are issued before the first use (indices clamped, none in a branch)
  auto fold = [&](const float* mo, const float* ml, int n) {
    for (int p0 = 0; p0 < n; p0 += 8) {
      float lse[8], mo_v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int pp = p0 + u < n ? p0 + u : n - 1;
        lse[u] = ml[pp];
        mo_v[u] = mo[(int64_t)pp * d + threadIdx.x];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool live = p0 + u < n;
        const float m_new = fmaxf(m_i, lse[u]);
        const float alpha = expf(m_i - m_new);
        const float w = expf(lse[u] - m_new);
        const float acc_n = acc * alpha + w * mo_v[u];
        const float d_n = d_i * alpha + w;
        acc = live ? acc_n : acc;
        d_i = live ? d_n : d_i;
        m_i = live ? m_new : m_i;
      }
    }
  };
  fold(pre_o + hrow * nsplit * d, pre_lse + hrow * nsplit, nsplit);
  fold(suf_o + hrow * nparts * d, suf_lse + hrow * nparts, np);
  out[b * o_sb + (int64_t)h * o_sh + threadIdx.x] = from_f32<DT>(acc / d_i);
}

template <int DT>
int sp_launch_prefix(const void* q, const void* kc, const void* vc, const SpArgs& a, const SpPlan& p, int hkv, int d,
                     hipStream_t st) {
  const dim3 grid((unsigned)p.nsplit, (unsigned)p.qtiles, (unsigned)hkv);
  if (d == 64)
    sp_prefix<DT, 64><<<grid, 256, 0, st>>>((const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, a);
  else
    sp_prefix<DT, 128><<<grid, 256, 0, st>>>((const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, a);
  return LL_LAUNCH_CHECK();
}

template <int DT>
int sp_launch_merge(void* out, const SpArgs& a, const SpPlan& p, float* ws, int d, int64_t o_sb, int64_t o_sh,
                    hipStream_t st) {
  sp_merge<DT><<<dim3((unsigned)a.hq, (unsigned)a.batch), d, 0, st>>>(
      (uint16_t*)out, ws + p.pre_o, ws + p.pre_lse, ws + p.suf_o, ws + p.suf_lse, (const int32_t*)(ws + p.suf_len), a.hq, d,
      p.nsplit, p.nparts, o_sb, o_sh);
  return LL_LAUNCH_CHECK();
}

}  // namespace

extern "C" int ll_shared_prefix_num_splits(int batch, int hq, int hkv, int d, int64_t prefix_len, int64_t max_len) {
  if (!sp_shape_ok(batch, hq, hkv, d, prefix_len, max_len) || batch == 0) return 0;
  return sp_plan(batch, hq, hkv, d, prefix_len, max_len).nsplit;
}

extern "C" int64_t ll_shared_prefix_workspace_floats(int batch, int hq, int hkv, int d, int64_t prefix_len, int64_t max_len) {
  if (!sp_shape_ok(batch, hq, hkv, d, prefix_len, max_len) || batch == 0) return 0;
  return sp_plan(batch, hq, hkv, d, prefix_len, max_len).floats;
}

extern "C" int ll_shared_prefix_decode_attention(void* out, const void* q, const void* k_cache, const void* v_cache,
                                                 const int32_t* table, const void* b_req_idx, const void* b_seq_len,
                                                 int64_t prefix_req, int64_t prefix_len, float* workspace, int batch, int hq,
                                                 int hkv, int d, int64_t max_len, float qk_scale, int64_t q_stride_b,
                                                 int64_t q_stride_h, int64_t k_stride_t, int64_t k_stride_h,
                                                 int64_t v_stride_t, int64_t v_stride_h, int64_t o_stride_b,
                                                 int64_t o_stride_h, int64_t table_stride_b, int dtype, int req_width,
                                                 int seq_width, void* stream) {
  if (dtype != LL_F16 && dtype != LL_BF16) return LL_ERR_SHAPE;  // e4m3 pools are not served
  if ((req_width | seq_width) & ~1) return LL_ERR_DTYPE;
  if (!sp_shape_ok(batch, hq, hkv, d, prefix_len, max_len) || prefix_req < 0 || table_stride_b < prefix_len)
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!out || !q || !k_cache || !v_cache || !table || !b_req_idx || !b_seq_len || !workspace) return LL_ERR_ARG;
  // 16-byte fragment loads and record stores: every row / head stride and base must be 8-element aligned
  if ((q_stride_b | q_stride_h | k_stride_t | k_stride_h | v_stride_t | v_stride_h) % 8 != 0 || !ll_aligned16(q) ||
      !ll_aligned16(k_cache) || !ll_aligned16(v_cache) || !ll_aligned16(workspace))
    return LL_ERR_ARG;
  const SpPlan p = sp_plan(batch, hq, hkv, d, prefix_len, max_len);
  SpArgs a;
  a.trow = table + prefix_req * table_stride_b;
  a.seq_len = b_seq_len;
  a.suf_len = (int32_t*)(workspace + p.suf_len);
  a.pre_o = workspace + p.pre_o;
  a.pre_lse = workspace + p.pre_lse;
  a.batch = batch;
  a.hq = hq;
  a.groups = hq / hkv;
  a.nsplit = p.nsplit;
  a.seq_w = seq_width;
  a.prefix_len = prefix_len;
  a.split = p.split;
  a.sm_scale = qk_scale * 1.44269504088896340736f;
  a.q_sb = q_stride_b; a.q_sh = q_stride_h;
  a.k_st = k_stride_t; a.k_sh = k_stride_h;
  a.v_st = v_stride_t; a.v_sh = v_stride_h;
  hipStream_t st = (hipStream_t)stream;
  int rc = dtype == LL_F16 ? sp_launch_prefix<LL_F16>(q, k_cache, v_cache, a, p, hkv, d, st)
                           : sp_launch_prefix<LL_BF16>(q, k_cache, v_cache, a, p, hkv, d, st);
  if (rc != LL_OK) return rc;
  if (p.nparts > 0) {
    // positions prefix_len .. of every row: the shifted table, the lengths sp_prefix left
    rc = fd_stage1_records(q, k_cache, v_cache, table + prefix_len, b_req_idx, a.suf_len, workspace + p.suf_o,
                           workspace + p.suf_lse, batch, hq, hkv, d, max_len - prefix_len, qk_scale, q_stride_b, q_stride_h,
                           k_stride_t, k_stride_h, v_stride_t, v_stride_h, table_stride_b, dtype, req_width, LL_I32, stream);
    if (rc != LL_OK) return rc;
  }
  return dtype == LL_F16 ? sp_launch_merge<LL_F16>(out, a, p, workspace, d, o_stride_b, o_stride_h, st)
                         : sp_launch_merge<LL_BF16>(out, a, p, workspace, d, o_stride_b, o_stride_h, st);
}
