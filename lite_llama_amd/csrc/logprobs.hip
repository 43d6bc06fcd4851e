// Sampler row, third kernel (after argmax and the nucleus draw): token log-probabilities.
//   ll_token_logprobs -- per row of logits [rows, vocab]: lse = max + ln(sum exp(z - max)) in fp32, the log-probability
//                        of one named token and the top_k largest logits ordered by (logit descending, index ascending).
// The row is read from HBM once.  A 256-thread workgroup walks its span of the row in tiles of 4096 logits held in
// REGISTERS (16 per thread, 16-byte loads): every thread keeps an online (max, sum) pair, and the k selection passes are
// block-wide arg-max reductions over the threads' register-resident candidates -- no second pass over memory, no
// vocabulary-sized temporary.  A workgroup leaves (max, sum, k candidates) in caller-supplied scratch; a one-wave merge
// launch per row combines the <= 64 partials (lane = chunk: a k-way merge of sorted lists) and writes the results at a
// column read from device memory, so one captured launch fills successive columns on successive graph replays.
// Two regimes, one code path: few rows (decode) -> grid [rows x chunks], one or two tiles per workgroup; many rows
// (scoring) -> chunks = 1, a workgroup per row walks all its tiles and merges every tile's winners into a running list
// (after the first tiles almost no tile beats the list's last entry: one reduction per tile).
#include "common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_E = 16;                     // logits per thread per tile
constexpr int LP_TILE = LP_THREADS * LP_E;   // 4096 logits per tile
constexpr int LP_MAX_K = 20;
constexpr int LP_MAX_CHUNKS = 64;            // one merge lane per chunk
constexpr int64_t LP_MAX_VOCAB = 1 << 30;     // indices and chunk bounds are 32-bit
constexpr int LP_NONE = INT32_MAX;           // index of "no candidate"
constexpr float LP_LOG2E = 1.4426950408889634f;

struct LpPlan {
  int chunks;
  int64_t per;  // logits per chunk: a whole number of tiles
};
// rows x chunks ~ 4096 workgroups (8 resident per CU at 4 waves each, two rounds) while a chunk keeps at least one tile
inline LpPlan lp_plan(int64_t rows, int64_t vocab) {
  const int64_t tiles = (vocab + LP_TILE - 1) / LP_TILE;
  int64_t want = 4096 / (rows > 0 ? rows : 1);
  want = want < 1 ? 1 : (want > LP_MAX_CHUNKS ? LP_MAX_CHUNKS : want);
  if (want > tiles) want = tiles;
  const int64_t tiles_per = (tiles + want - 1) / want;
  LpPlan p;
  p.chunks = (int)((tiles + tiles_per - 1) / tiles_per);
  p.per = tiles_per * LP_TILE;
  return p;
}
// one partial = {max, sum, k x {logit, index}} 32-bit words
__host__ __device__ inline int64_t lp_record_words(int k) { return 2 + 2 * (int64_t)k; }

template <int CTRL>
__device__ __forceinline__ int lp_dpp(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
// minimum over the wave, same moves as wave_max (common.h); every lane active
__device__ __forceinline__ int wave_min_i32(int v) {
  int t;
  t = lp_dpp<0xB1>(v); v = v < t ? v : t;
  t = lp_dpp<0x4E>(v); v = v < t ? v : t;
  t = lp_dpp<0x124>(v); v = v < t ? v : t;
  t = lp_dpp<0x128>(v); v = v < t ? v : t;
  auto a = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  v = (int)a[0] < (int)a[1] ? (int)a[0] : (int)a[1];
  auto b = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  v = (int)b[0] < (int)b[1] ? (int)b[0] : (int)b[1];
  return __builtin_amdgcn_readfirstlane(v);
}
// the wave's best (logit descending, index ascending); exhausted lanes hold (-inf, LP_NONE)
__device__ __forceinline__ void wave_best(float& v, int& i) {
  const float m = wave_max(v);
  i = wave_min_i32(v == m ? i : LP_NONE);
  v = m;
}

__device__ __forceinline__ float lp_exp(float d) { return __builtin_amdgcn_exp2f(d * LP_LOG2E); }  // d <= 0

template <int DT>
__device__ __forceinline__ float lp_load(const void* p, int64_t i) {
  if constexpr (DT == LL_F32) return ((const float*)p)[i];
  else return to_f32<DT>(((const uint16_t*)p)[i]);
}

// Thread t's element e of the tile starting at `lo` is row index lo + ((e / VW) * 256 + t) * VW + e % VW: with VW = the
// logits of one 16-byte load every load instruction of a wave covers 1 KiB contiguous; indices ascend with e.
template <int DT, bool VEC>
struct LpTile {
  static constexpr int VW = !VEC ? 1 : (DT == LL_F32 ? 4 : 8);
  __device__ static __forceinline__ int index(int lo, int e) {
    return lo + ((e / VW) * LP_THREADS + (int)threadIdx.x) * VW + e % VW;
  }
  // values past `hi` read as -inf and are never dereferenced
  __device__ static __forceinline__ void load(float (&v)[LP_E], const void* row, int lo, int hi) {
#pragma unroll
    for (int g = 0; g < LP_E / VW; ++g) {
      const int i0 = index(lo, g * VW);
      if (VEC && i0 + VW <= hi) {
        if constexpr (DT == LL_F32) {
          const f32x4 t = *reinterpret_cast<const f32x4*>((const float*)row + i0);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[g * VW + j] = t[j];
        } else {
          const U16x8 t = *reinterpret_cast<const U16x8*>((const uint16_t*)row + i0);
#pragma unroll
          for (int j = 0; j < VW; ++j) v[g * VW + j] = to_f32<DT>(t.v[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < VW; ++j) v[g * VW + j] = i0 + j < hi ? lp_load<DT>(row, i0 + j) : -INFINITY;
      }
    }
  }
};

// grid = (rows, chunks).  part: [rows, chunks] records of lp_record_words(k) words.
template <int DT, bool VEC>
__global__ __launch_bounds__(LP_THREADS) void logprobs_part_kernel(uint32_t* __restrict__ part,
                                                                   const void* __restrict__ logits, int vocab,
                                                                   int64_t stride, int per, int k) {
  using T = LpTile<DT, VEC>;
  __shared__ float s_rv[2][LP_MAX_K];  // the running top-k list, double-buffered for the per-tile merge
  __shared__ int s_ri[2][LP_MAX_K];
  __shared__ float s_wv[2][4];         // per-wave winners of a selection pass, double-buffered by pass parity
  __shared__ int s_wi[2][4];
  __shared__ float s_red[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c_lo = (int)blockIdx.y * per;
  const int c_hi = c_lo + per < vocab ? c_lo + per : vocab;
  const void* rowp = DT == LL_F32 ? (const void*)((const float*)logits + row * stride)
                                  : (const void*)((const uint16_t*)logits + row * stride);
  float m_t = -INFINITY, s_t = 0.f;  // this thread's online max / sum of exp(z - max)
  int n_r = 0, cur = 0, par = 0;     // running list length, its buffer, selection-pass parity (all block-uniform)

  for (int lo = c_lo; lo < c_hi; lo += LP_TILE) {
    float v[LP_E];
    T::load(v, rowp, lo, c_hi);
    float tm = v[0];
#pragma unroll
    for (int e = 1; e < LP_E; ++e) tm = fmaxf(tm, v[e]);
    if (tm > m_t) {
      s_t *= lp_exp(m_t - tm);  // first tile: 0 * exp2(-inf) = 0
      m_t = tm;
    }
    if (m_t > -INFINITY) {
      float x[LP_E];
#pragma unroll
      for (int e = 0; e < LP_E; ++e) x[e] = lp_exp(v[e] - m_t);  // pads: exp2(-inf) = 0
#pragma unroll
      for (int h = LP_E / 2; h > 0; h >>= 1)
#pragma unroll
        for (int e = 0; e < h; ++e) x[e] += x[e + h];
      s_t += x[0];
    }
    if (k == 0) continue;

    // selection: repeatedly take the block's best remaining logit of this tile and merge it with the running list
    // (entries of earlier tiles: lower indices, so they win ties).  Every branch below is block-uniform.
    int a = 0, j = 0;
    const int nxt = cur ^ 1;
    bool first = true;
    // this thread's best remaining logit of the tile: recomputed only by the thread that loses its candidate to the list
    float my_v = -INFINITY;
    int my_i = LP_NONE;
#pragma unroll
    for (int e = 0; e < LP_E; ++e)
      if (v[e] > my_v) {  // indices ascend with e: strict > keeps the first maximum
        my_v = v[e];
        my_i = T::index(lo, e);
      }
    while (true) {
      float lb = my_v;
      int li = my_i;
      wave_best(lb, li);
      if (lane == 0) {
        s_wv[par][w] = lb;
        s_wi[par][w] = li;
      }
      __syncthreads();
      float bm = s_wv[par][0];
      int bi = s_wi[par][0];
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        const float qv = s_wv[par][q];
        const int qi = s_wi[par][q];
        if (qv > bm || (qv == bm && qi < bi)) {
          bm = qv;
          bi = qi;
        }
      }
      par ^= 1;
      if (first && n_r == k && !(bm > s_rv[cur][k - 1])) break;  // the tile cannot enter a full list: nothing to merge
      first = false;
      // copy list entries that precede the tile's candidate
      while (j < k && a < n_r && (bi == LP_NONE || s_rv[cur][a] >= bm)) {
        if (tid == 0) {
          s_rv[nxt][j] = s_rv[cur][a];
          s_ri[nxt][j] = s_ri[cur][a];
        }
        ++a;
        ++j;
      }
      if (j < k && bi != LP_NONE) {
        if (tid == 0) {
          s_rv[nxt][j] = bm;
          s_ri[nxt][j] = bi;
        }
        ++j;
        if (my_i == bi) {
          my_v = -INFINITY;
          my_i = LP_NONE;
#pragma unroll
          for (int e = 0; e < LP_E; ++e) {
            if (T::index(lo, e) == bi) v[e] = -INFINITY;
            if (v[e] > my_v) {
              my_v = v[e];
              my_i = T::index(lo, e);
            }
          }
        }
      }
      if (j >= k || (bi == LP_NONE && a >= n_r)) {
        n_r = j;
        cur = nxt;
        __syncthreads();  // the new list is complete before anyone reads it
        break;
      }
    }
  }

  // block totals
  float bm = wave_max(m_t);
  if (lane == 0) s_red[w] = bm;
  __syncthreads();
  bm = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  float bs = wave_sum(m_t > -INFINITY ? s_t * lp_exp(m_t - bm) : 0.f);
  __syncthreads();
  if (lane == 0) s_red[w] = bs;
  __syncthreads();
  bs = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  uint32_t* rec = part + (row * gridDim.y + blockIdx.y) * lp_record_words(k);
  if (tid == 0) {
    rec[0] = __float_as_uint(bm);
    rec[1] = __float_as_uint(bs);
  }
  if (tid < k) {
    rec[2 + 2 * tid] = __float_as_uint(tid < n_r ? s_rv[cur][tid] : -INFINITY);
    rec[3 + 2 * tid] = (uint32_t)(tid < n_r ? s_ri[cur][tid] : LP_NONE);
  }
}

// grid = rows, one wave: lane c owns chunk c's record.
template <int DT>
__global__ __launch_bounds__(64) void logprobs_merge_kernel(float* __restrict__ chosen, float* __restrict__ top_lp,
                                                            int64_t* __restrict__ top_ids,
                                                            const uint32_t* __restrict__ part,
                                                            const void* __restrict__ logits,
                                                            const int64_t* __restrict__ token_ids,
                                                            const int64_t* __restrict__ column, int64_t vocab,
                                                            int64_t stride, int chunks, int k, int64_t num_columns,
                                                            int64_t chosen_stride, int64_t top_lp_stride,
                                                            int64_t top_ids_stride) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const bool has = lane < chunks;
  const uint32_t* rec = part + (row * chunks + (has ? lane : 0)) * lp_record_words(k);
  const float m_c = has ? __uint_as_float(rec[0]) : -INFINITY;
  const float s_c = has ? __uint_as_float(rec[1]) : 0.f;
  const float m = wave_max(m_c);
  const float s = wave_sum(m_c > -INFINITY ? s_c * lp_exp(m_c - m) : 0.f);
  const float lse = m + logf(s);
  const int64_t col = column ? *column : 0;
  const bool store = lane == 0 && col >= 0 && col < num_columns;  // a column outside the buffers writes nothing
  if (store && chosen) {
    const int64_t tok = token_ids[row];
    chosen[row * chosen_stride + col] =
        tok >= 0 && tok < vocab ? lp_load<DT>(logits, row * stride + tok) - lse : __uint_as_float(0x7fc00000u);
  }
  int p = 0;
  float hv = has && k > 0 ? __uint_as_float(rec[2]) : -INFINITY;
  int hi = has && k > 0 ? (int)rec[3] : LP_NONE;
  for (int j = 0; j < k; ++j) {
    float bv = hv;
    int bi = hi;
    wave_best(bv, bi);
    if (store) {
      top_lp[row * top_lp_stride + col * k + j] = bv - lse;
      top_ids[row * top_ids_stride + col * k + j] = bi == LP_NONE ? -1 : (int64_t)bi;
    }
    if (hi == bi && bi != LP_NONE) {  // the winning lane moves to its next candidate
      ++p;
      hv = p < k ? __uint_as_float(rec[2 + 2 * p]) : -INFINITY;
      hi = p < k ? (int)rec[3 + 2 * p] : LP_NONE;
    }
  }
}

}  // namespace

extern "C" int64_t ll_token_logprobs_scratch_bytes(int64_t rows, int64_t vocab, int top_k) {
  if (rows <= 0 || vocab <= 0 || vocab > LP_MAX_VOCAB) return LL_ERR_SHAPE;
  if (top_k < 0 || top_k > LP_MAX_K || top_k > vocab) return LL_ERR_ARG;
  return rows * lp_plan(rows, vocab).chunks * lp_record_words(top_k) * 4;
}

extern "C" int ll_token_logprobs(float* chosen, float* top_logprobs, int64_t* top_ids, const void* logits,
                                 const int64_t* token_ids, const int64_t* column, int64_t rows, int64_t vocab,
                                 int64_t logits_stride, int top_k, int64_t num_columns, int64_t chosen_stride,
                                 int64_t top_logprobs_stride, int64_t top_ids_stride, int dtype, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
  if (rows < 0 || vocab <= 0 || vocab > LP_MAX_VOCAB || logits_stride < vocab || num_columns <= 0)
    return LL_ERR_SHAPE;
  if (top_k < 0 || top_k > LP_MAX_K || top_k > vocab) return LL_ERR_ARG;
  if (!logits || !scratch || (chosen != nullptr) != (token_ids != nullptr)) return LL_ERR_ARG;
  if (top_k > 0 && (!top_logprobs || !top_ids)) return LL_ERR_ARG;
  if (!chosen && top_k == 0) return LL_ERR_ARG;
  if (dtype != LL_F16 && dtype != LL_BF16 && dtype != LL_F32) return LL_ERR_DTYPE;
  if (rows == 0) return LL_OK;
  if (scratch_bytes < ll_token_logprobs_scratch_bytes(rows, vocab, top_k) || (reinterpret_cast<uintptr_t>(scratch) & 3u))
    return LL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const LpPlan plan = lp_plan(rows, vocab);
  const int64_t esize = dtype == LL_F32 ? 4 : 2;
  const bool vec = ll_aligned16(logits) && (logits_stride * esize) % 16 == 0;
  const dim3 grid((unsigned)rows, (unsigned)plan.chunks);
  uint32_t* part = (uint32_t*)scratch;
#define LL_LP_PART(DT)                                                                                              \
  do {                                                                                                              \
    if (vec)                                                                                                        \
      logprobs_part_kernel<DT, true><<<grid, LP_THREADS, 0, st>>>(part, logits, (int)vocab, logits_stride,          \
                                                                  (int)plan.per, top_k);                            \
    else                                                                                                            \
      logprobs_part_kernel<DT, false><<<grid, LP_THREADS, 0, st>>>(part, logits, (int)vocab, logits_stride,         \
                                                                   (int)plan.per, top_k);                           \
    logprobs_merge_kernel<DT><<<dim3((unsigned)rows), 64, 0, st>>>(                                                 \
        chosen, top_logprobs, top_ids, part, logits, token_ids, column, vocab, logits_stride, plan.chunks, top_k,   \
        num_columns, chosen_stride, top_logprobs_stride, top_ids_stride);                                           \
  } while (0)
  if (dtype == LL_F16) LL_LP_PART(LL_F16);
  else if (dtype == LL_BF16) LL_LP_PART(LL_BF16);
  else LL_LP_PART(LL_F32);
#undef LL_LP_PART
  return LL_LAUNCH_CHECK();
}
