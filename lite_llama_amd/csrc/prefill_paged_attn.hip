// Causal prefill attention over the paged KV pool (extension; the reference's prefill only attends over the q/k/v the
// same step has just projected).  Sequence b holds ctx[b] cached tokens and n[b] new ones: the new tokens' queries are
// rows b_start_loc[b] + j (j < n[b]) of q [T, Hq, D], their K/V are already in the pool, and query j attends to key
// positions 0 .. ctx[b] + j, position p living in pool row table[b_req_idx[b]][p] (the pool layout decode reads:
// [rows, 2 Hkv, D], K heads first).  Same arithmetic as fa_prefill2 / fa_prefill (csrc/prefill_attn.hip): exp2 with
// sm_scale carrying log2 e, masked score -1e8, fp32 accumulators, P rounded to the storage dtype before PV; query rows
// j >= n[b] are not written.  With ctx = 0 and an identity table this is ll_flash_attention_nopad.
//
// The only change in the key walk is the row a key comes from: a 64-key tile's table entries are read once per tile
// (lane l of every wave holds the entry of key p0 + l, one tile ahead of the K/V gathers that use it) and handed to the
// gathering lanes by a lane permute, so the K/V loads of tile p0 + 64 stay in flight under tile p0's MFMAs as in
// fa_prefill2.  Keys are clamped to the sequence's last named position (ctx + n - 1): rows the table does not name for
// this sequence are never read, and V rows past the valid range are zeroed in LDS (they meet p = 0).
//
// e4m3 pool (KV8): K/V are gathered as 8-byte pieces and widened to fp16 while staging into LDS
// (v_cvt_scalef32_pk_f16_fp8, exact); the LDS image and the MFMA code are the fp16 ones, k_scale rides on the softmax
// scale (the host folds it into sm_scale) and v_scale on the final normalisation -- ll_flash_decoding_fp8kv's semantics.
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

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

// One 8-element piece of a K/V row: 16 bytes of a 16-bit pool, or 8 e4m3 bytes widened to fp16 at staging.
template <bool KV8>
struct PagedKv {
  using Elem = uint16_t;
  using Raw = i32x4;
  static __device__ __forceinline__ i32x4 widen(const i32x4& r) { return r; }
};
template <>
struct PagedKv<true> {
  using Elem = uint8_t;
  using Raw = i32x2;
  static __device__ __forceinline__ i32x4 widen(const i32x2& r) {
    i32x4 o;
    o.x = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(r.x, 1.0f, false));
    o.y = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(r.x, 1.0f, true));
    o.z = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(r.y, 1.0f, false));
    o.w = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(r.y, 1.0f, true));
    return o;
  }
};

struct PagedArgs {
  const int32_t* table;
  const void *req_idx, *start_loc, *q_len, *ctx_len;
  int hq, hkv;
  float sm_scale, v_scale;  // sm_scale: log2 e / sqrt(D) (x k_scale for an e4m3 pool)
  int64_t q_st, q_sh, k_st, k_sh, v_st, v_sh, o_st, o_sh, t_st;
  int req_w, start_w, qlen_w, ctx_w;
};

// Four-wave form (D = 64 / 128): a workgroup owns 64 * QB consecutive new queries of one (sequence, head) and walks the
// keys in 64-row tiles, global -> registers -> LDS, the next tile in flight (fa_prefill2's structure).
// grid = (ceil(max_q_len / (64 QB)), hq, batch), block = 256
template <int DT, int D, int QB, bool KV8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void paged_prefill4(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ q, const typename PagedKv<KV8>::Elem* __restrict__ kp,
    const typename PagedKv<KV8>::Elem* __restrict__ vp, PagedArgs a) {
  using Kv = PagedKv<KV8>;
  constexpr int NS = D / 32, NT = D / 16, STR = D + 8, TK = 64;
  constexpr int TPR = D / 8, RPP = 256 / TPR, PASSES = TK / RPP;  // 8-element pieces per row, rows per pass
  __shared__ __attribute__((aligned(16))) uint16_t lds_k[TK * STR];
  __shared__ __attribute__((aligned(16))) uint16_t lds_v[TK * STR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane & 15, c = lane >> 4;
  const int head = blockIdx.y, b = blockIdx.z;
  const int kvh = head / (a.hq / a.hkv);
  const int64_t n = load_idx(a.q_len, b, a.qlen_w);
  const int64_t q0 = (int64_t)(gridDim.x - 1 - blockIdx.x) * (64 * QB);  // the longest key ranges are dispatched first
  if (q0 >= n) return;
  const int64_t ctx = load_idx(a.ctx_len, b, a.ctx_w);
  const int64_t start = load_idx(a.start_loc, b, a.start_w);
  const int32_t* trow = a.table + load_idx(a.req_idx, b, a.req_w) * a.t_st;
  const int64_t total = ctx + n;             // named positions of this sequence
  const int64_t qw = q0 + wave * (16 * QB);  // this wave's first new query
  const float sm_scale = a.sm_scale;

  Q4 qf[QB][NS];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int64_t qi = qw + qb * 16 + t;
    const int64_t qrow = qi < n ? qi : n - 1;  // rows past the chunk: a valid row, never stored
#pragma unroll
    for (int s = 0; s < NS; ++s)
      qf[qb][s] = *reinterpret_cast<const Q4*>(q + (start + qrow) * a.q_st + (int64_t)head * a.q_sh + s * 32 + c * 8);
  }
  float m_i[QB], d_i[QB];
  f32x4 ot[QB][NT];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    m_i[qb] = -INFINITY;
    d_i[qb] = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) ot[qb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // causal: the workgroup needs key positions < kend
  const int64_t kend = ctx + (q0 + 64 * QB < n ? q0 + 64 * QB : n);
  const int lrow = tid / TPR, lcol = (tid % TPR) * 8;
  typename Kv::Raw kr[PASSES], vr[PASSES];
  auto table_entries = [&](int64_t p0) {  // lane l: the row of key p0 + l (clamped to the last named position)
    const int64_t key = p0 + lane < total ? p0 + lane : total - 1;
    return trow[key];
  };
  auto fetch = [&](int tr) {  // tr: this lane's table entry of the tile being fetched
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int64_t row = __shfl(tr, ps * RPP + lrow, 64);
      kr[ps] = *reinterpret_cast<const typename Kv::Raw*>(kp + row * a.k_st + (int64_t)kvh * a.k_sh + lcol);
      vr[ps] = *reinterpret_cast<const typename Kv::Raw*>(vp + row * a.v_st + (int64_t)kvh * a.v_sh + lcol);
    }
  };
  auto stage = [&](int64_t p0) {
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int row = ps * RPP + lrow;
      *reinterpret_cast<i32x4*>(&lds_k[row * STR + lcol]) = Kv::widen(kr[ps]);
      // rows past the named range are multiplied by p = 0: they must not hold NaN / Inf bit patterns
      *reinterpret_cast<i32x4*>(&lds_v[row * STR + lcol]) = p0 + row < total ? Kv::widen(vr[ps]) : i32x4{0, 0, 0, 0};
    }
  };
  auto next_tile = [&](int64_t p0) { return p0 + TK < kend ? p0 + TK : p0; };
  const uint16_t* vtr = lds_v + (4 * c + (t >> 2)) * STR + (t & 3) * 4;

  fetch(table_entries(0));
  int tr = table_entries(next_tile(0));  // invariant at the top of iteration p0: the entries of next_tile(p0)
  for (int64_t p0 = 0; p0 < kend; p0 += TK) {
    __syncthreads();  // the previous tile's fragment reads are done
    stage(p0);
    __syncthreads();
    const int64_t pn = next_tile(p0);
    fetch(tr);  // tile pn, in flight under this tile's arithmetic (unconditional: a branch around loads parks the
                // prefetch registers in scratch)
    tr = table_entries(next_tile(pn));
    if (p0 >= ctx + qw + 16 * QB) continue;  // every key of the tile lies after this wave's last query
    f32x4 sacc[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) sacc[qb][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const Q4 kf = *reinterpret_cast<const Q4*>(&lds_k[(kb * 16 + t) * STR + s * 32 + c * 8]);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) sacc[qb][kb] = mfma16<DT>(kf, qf[qb][s], sacc[qb][kb]);
      }
    }
    Q4 pf[QB][2];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const int64_t qfirst = ctx + qw + qb * 16;  // absolute position of the block's first query
      float sc[16];
      float mx = -INFINITY;
      if (p0 + TK - 1 <= qfirst) {  // whole tile at or before the block's first query: no mask (wave-uniform)
#pragma unroll
        for (int j = 0; j < 16; ++j) sc[j] = sacc[qb][j >> 2][j & 3];
      } else {
        const int64_t qi = qfirst + t;
        const float masked = -1.0e8f / sm_scale;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int64_t key = p0 + 16 * (j >> 2) + 4 * c + (j & 3);
          sc[j] = key <= qi ? sacc[qb][j >> 2][j & 3] : masked;
        }
      }
#pragma unroll
      for (int j = 0; j < 16; j += 2) mx = fmaxf(mx, fmaxf(sc[j], sc[j + 1]));
      mx *= sm_scale;
      mx = rows_max(mx);
      const float m_new = fmaxf(m_i[qb], mx);
      const float alpha = __builtin_amdgcn_exp2f(m_i[qb] - m_new);
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        sc[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j], sm_scale, -m_new));
        psum += sc[j];
      }
      psum = rows_sum(psum);
      d_i[qb] = d_i[qb] * alpha + psum;
      m_i[qb] = m_new;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) {
          ot[qb][dt][0] *= alpha; ot[qb][dt][1] *= alpha; ot[qb][dt][2] *= alpha; ot[qb][dt][3] *= alpha;
        }
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        pf[qb][hf].x = pack2<DT>(sc[8 * hf + 0], sc[8 * hf + 1]);
        pf[qb][hf].y = pack2<DT>(sc[8 * hf + 2], sc[8 * hf + 3]);
        pf[qb][hf].z = pack2<DT>(sc[8 * hf + 4], sc[8 * hf + 5]);
        pf[qb][hf].w = pack2<DT>(sc[8 * hf + 6], sc[8 * hf + 7]);
      }
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
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) ot[qb][dt] = mfma16<DT>(vf, pf[qb][hf], ot[qb][dt]);
      }
    }
  }

#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int64_t qi = qw + qb * 16 + t;
    if (qi < n) {
      const float inv = (KV8 ? a.v_scale : 1.0f) / d_i[qb];
      uint16_t* o = out + (start + qi) * a.o_st + (int64_t)head * a.o_sh;
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        uint2 pk;
        pk.x = pack2<DT>(ot[qb][dt][0] * inv, ot[qb][dt][1] * inv);
        pk.y = pack2<DT>(ot[qb][dt][2] * inv, ot[qb][dt][3] * inv);
        *reinterpret_cast<uint2*>(o + dt * 16 + 4 * c) = pk;
      }
    }
  }
}

// One-wave form (D = 32 / 256, 16-bit pools; fa_prefill's structure): a wave owns 16 new queries of one (sequence,
// head), K fragments come straight from the gathered rows, V is staged per 32-key tile through LDS.  Each lane reads
// the table entries of its two keys (t, 16 + t) of the next tile while the current one is computed.
// grid = (ceil(max_q_len / 16), hq, batch), block = 64
template <int DT, int D>
__global__ __launch_bounds__(64) void paged_prefill1(uint16_t* __restrict__ out, const uint16_t* __restrict__ q,
                                                     const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
                                                     PagedArgs a) {
  constexpr int NS = D / 32, DQ = D / 4, NT = D / 16, VSTR = D + 8;
  __shared__ __attribute__((aligned(16))) uint16_t lds_v[32 * VSTR];

  const int lane = threadIdx.x;
  const int t = lane & 15, c = lane >> 4;
  const int head = blockIdx.y, b = blockIdx.z;
  const int kvh = head / (a.hq / a.hkv);
  const int64_t n = load_idx(a.q_len, b, a.qlen_w);
  const int64_t q0 = (int64_t)(gridDim.x - 1 - blockIdx.x) * 16;  // the longest key ranges are dispatched first
  if (q0 >= n) return;
  const int64_t ctx = load_idx(a.ctx_len, b, a.ctx_w);
  const int64_t start = load_idx(a.start_loc, b, a.start_w);
  const int32_t* trow = a.table + load_idx(a.req_idx, b, a.req_w) * a.t_st;
  const float sm_scale = a.sm_scale;

  const int64_t qrow = (q0 + t < n) ? q0 + t : n - 1;
  Q4 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    qf[s] = *reinterpret_cast<const Q4*>(q + (start + qrow) * a.q_st + (int64_t)head * a.q_sh + c * DQ + s * 8);

  float m_i = -INFINITY, d_i = 0.f;
  f32x4 ot[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) ot[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t qi = ctx + q0 + t;                               // this lane's query, absolute position
  const int64_t kend = ctx + ((q0 + 16 < n) ? q0 + 16 : n);      // causal: keys < kend (all named)
  auto entry = [&](int64_t key) { return (int64_t)trow[key < kend ? key : kend - 1]; };
  int64_t ra = entry(t), rb = entry(16 + t);
  for (int64_t p0 = 0; p0 < kend; p0 += 32) {
    const int64_t ka_i = p0 + t, kb_i = p0 + 16 + t;
    const bool okA = ka_i < kend, okB = kb_i < kend;
    const uint16_t* kA = kp + ra * a.k_st + (int64_t)kvh * a.k_sh + c * DQ;
    const uint16_t* kB = kp + rb * a.k_st + (int64_t)kvh * a.k_sh + c * DQ;
    const uint16_t* vA = vp + ra * a.v_st + (int64_t)kvh * a.v_sh + c * DQ;
    const uint16_t* vB = vp + rb * a.v_st + (int64_t)kvh * a.v_sh + c * DQ;
    Q4 ka[NS], kb[NS], va[NS], vb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      ka[s] = *reinterpret_cast<const Q4*>(kA + s * 8);
      kb[s] = *reinterpret_cast<const Q4*>(kB + s * 8);
      va[s] = *reinterpret_cast<const Q4*>(vA + s * 8);
      vb[s] = *reinterpret_cast<const Q4*>(vB + s * 8);
    }
    ra = entry(p0 + 32 + t);
    rb = entry(p0 + 48 + t);
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) sa = mfma16<DT>(ka[s], qf[s], sa);
#pragma unroll
    for (int s = 0; s < NS; ++s) sb = mfma16<DT>(kb[s], qf[s], sb);

    float sc[8];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t k0i = p0 + 4 * c + r, k1i = p0 + 16 + 4 * c + r;
      sc[r] = (k0i <= qi && k0i < kend) ? sa[r] * sm_scale : -1.0e8f;
      sc[4 + r] = (k1i <= qi && k1i < kend) ? sb[r] * sm_scale : -1.0e8f;
      mx = fmaxf(mx, fmaxf(sc[r], sc[4 + r]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_i, mx);
    const float alpha = exp2f(m_i - m_new);
    float p[8];
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[j] = exp2f(sc[j] - m_new);
      ps += p[j];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    d_i = d_i * alpha + ps;
    m_i = m_new;
    Q4 pf;
    pf.x = pack2<DT>(p[0], p[1]);
    pf.y = pack2<DT>(p[2], p[3]);
    pf.z = pack2<DT>(p[4], p[5]);
    pf.w = pack2<DT>(p[6], p[7]);

    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      *reinterpret_cast<Q4*>(&lds_v[t * VSTR + c * DQ + s * 8]) = okA ? va[s] : Q4{0, 0, 0, 0};
      *reinterpret_cast<Q4*>(&lds_v[(16 + t) * VSTR + c * DQ + s * 8]) = okB ? vb[s] : Q4{0, 0, 0, 0};
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
      uint32_t w[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j0 = 2 * jj, j1 = 2 * jj + 1;
        const int r0 = 16 * (j0 >> 2) + 4 * c + (j0 & 3);
        const int r1 = 16 * (j1 >> 2) + 4 * c + (j1 & 3);
        const uint32_t lo = lds_v[r0 * VSTR + dt * 16 + t];
        const uint32_t hi = lds_v[r1 * VSTR + dt * 16 + t];
        w[jj] = lo | (hi << 16);
      }
      const Q4 vf = {w[0], w[1], w[2], w[3]};
      f32x4 acc = ot[dt];
      acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
      ot[dt] = mfma16<DT>(vf, pf, acc);
    }
  }

  if (q0 + t < n) {
    const float inv = 1.0f / d_i;
    uint16_t* o = out + (start + q0 + t) * a.o_st + (int64_t)head * a.o_sh;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
      uint2 pk;
      pk.x = pack2<DT>(ot[dt][0] * inv, ot[dt][1] * inv);
      pk.y = pack2<DT>(ot[dt][2] * inv, ot[dt][3] * inv);
      *reinterpret_cast<uint2*>(o + dt * 16 + 4 * c) = pk;
    }
  }
}

template <int DT, bool KV8>
int launch_paged(void* out, const void* q, const void* k, const void* v, int batch, int d, int64_t max_q_len,
                 const PagedArgs& a, hipStream_t st) {
  using E = typename PagedKv<KV8>::Elem;
  if (d == 64 || d == 128) {
    const int qb = max_q_len > 64 ? 2 : 1;
    const dim3 grid((unsigned)((max_q_len + 64 * qb - 1) / (64 * qb)), (unsigned)a.hq, (unsigned)batch);
#define LL_PP4(DD, QQ) \
  paged_prefill4<DT, DD, QQ, KV8><<<grid, 256, 0, st>>>((uint16_t*)out, (const uint16_t*)q, (const E*)k, (const E*)v, a)
    if (d == 64) {
      if (qb == 2) LL_PP4(64, 2); else LL_PP4(64, 1);
    } else {
      if (qb == 2) LL_PP4(128, 2); else LL_PP4(128, 1);
    }
#undef LL_PP4
    return LL_LAUNCH_CHECK();
  }
  if constexpr (!KV8) {
    const dim3 grid((unsigned)((max_q_len + 15) / 16), (unsigned)a.hq, (unsigned)batch);
#define LL_PP1(DD) \
  paged_prefill1<DT, DD><<<grid, 64, 0, st>>>((uint16_t*)out, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, a)
    switch (d) {
      case 32: LL_PP1(32); break;
      case 256: LL_PP1(256); break;
      default: return LL_ERR_SHAPE;
    }
#undef LL_PP1
    return LL_LAUNCH_CHECK();
  }
  return LL_ERR_SHAPE;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int ll_prefill_paged_attention(void* out, const void* q, const void* k_cache, const void* v_cache,
                                          const int32_t* table, const void* b_req_idx, const void* b_start_loc,
                                          const void* b_q_len, const void* b_ctx_len, int batch, int hq, int hkv, int d,
                                          int64_t max_q_len, int64_t max_ctx_len, float sm_scale, float k_scale,
                                          float v_scale, int64_t q_stride_t, int64_t q_stride_h, int64_t k_stride_t,
                                          int64_t k_stride_h, int64_t v_stride_t, int64_t v_stride_h,
                                          int64_t o_stride_t, int64_t o_stride_h, int64_t table_stride, int dtype,
                                          int kv_dtype, int req_width, int start_width, int q_len_width,
                                          int ctx_width, void* stream) {
  if (dtype != LL_F16 && dtype != LL_BF16) return LL_ERR_DTYPE;
  const bool kv8 = kv_dtype == LL_FP8E4M3;
  if (kv_dtype != dtype && !(kv8 && dtype == LL_F16)) return LL_ERR_DTYPE;
  if ((req_width | start_width | q_len_width | ctx_width) & ~1) return LL_ERR_DTYPE;
  if (batch < 0 || batch > 65535 || hq <= 0 || hkv <= 0 || hq % hkv != 0 || max_q_len < 0 || max_ctx_len < 0)
    return LL_ERR_SHAPE;
  if (kv8 ? (d != 64 && d != 128) : (d != 32 && d != 64 && d != 128 && d != 256)) return LL_ERR_SHAPE;
  if (kv8 && !(k_scale > 0.f && v_scale > 0.f)) return LL_ERR_ARG;
  if (batch == 0 || max_q_len == 0) return LL_OK;
  if (!out || !q || !k_cache || !v_cache || !table || !b_req_idx || !b_start_loc || !b_q_len || !b_ctx_len ||
      table_stride < 1)
    return LL_ERR_ARG;
  // 16-byte query / output pieces; 16-byte (16-bit pool) or 8-byte (e4m3 pool) K / V pieces
  if ((q_stride_t | q_stride_h | o_stride_t | o_stride_h | k_stride_t | k_stride_h | v_stride_t | v_stride_h) % 8 != 0 ||
      !ll_aligned16(q) || !ll_aligned16(out))
    return LL_ERR_ARG;
  if (kv8 ? !(aligned8(k_cache) && aligned8(v_cache)) : !(ll_aligned16(k_cache) && ll_aligned16(v_cache)))
    return LL_ERR_ARG;
  PagedArgs a;
  a.table = table;
  a.req_idx = b_req_idx;
  a.start_loc = b_start_loc;
  a.q_len = b_q_len;
  a.ctx_len = b_ctx_len;
  a.hq = hq;
  a.hkv = hkv;
  a.sm_scale = kv8 ? sm_scale * k_scale : sm_scale;
  a.v_scale = kv8 ? v_scale : 1.0f;
  a.q_st = q_stride_t; a.q_sh = q_stride_h;
  a.k_st = k_stride_t; a.k_sh = k_stride_h;
  a.v_st = v_stride_t; a.v_sh = v_stride_h;
  a.o_st = o_stride_t; a.o_sh = o_stride_h;
  a.t_st = table_stride;
  a.req_w = req_width;
  a.start_w = start_width;
  a.qlen_w = q_len_width;
  a.ctx_w = ctx_width;
  hipStream_t st = (hipStream_t)stream;
  if (kv8) return launch_paged<LL_F16, true>(out, q, k_cache, v_cache, batch, d, max_q_len, a, st);
  if (dtype == LL_F16) return launch_paged<LL_F16, false>(out, q, k_cache, v_cache, batch, d, max_q_len, a, st);
  return launch_paged<LL_BF16, false>(out, q, k_cache, v_cache, batch, d, max_q_len, a, st);
}
