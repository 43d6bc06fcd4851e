// ll_logit_penalties: repetition, presence and frequency penalties plus a sparse per-row logit bias in ONE pass over the
// logits -- the read and the write ll_repetition_penalty already costs.  Per row b and token v, with c = the number of
// masked-in entries of the generated span equal to v, in fp32 from the ORIGINAL stored logit:
//   1. x = z[v] + bias[v]                         (no bias named: x = z[v], -0 included)
//   2. c > 0:  x = x < 0 ? x * r : x / r          (ll_repetition_penalty's expression)
//   3. x = fma(-f, c, x) - (c > 0 ? p : 0)
// and one rounding to the output dtype.  With p = f = 0 and no bias every step but 2 is the identity on the bits, so the
// output is ll_repetition_penalty's.
//
// grid = (chunks of LP_CHUNK tokens, batch), 256 threads.  A workgroup keeps its chunk's counts and biases in LDS: zero
// them, scatter the span with LDS atomic adds (a token repeated span times is one hot LDS word) and the row's bias entries
// with plain LDS stores, barrier, then one dense pass: 16-byte loads, the rule above, 16-byte stores.  A workgroup writes
// its own chunk only: nothing races, whatever the span holds.
//
// ll_seeded_uniform: one Philox4x32-10 block per row, key = the row's seed, counter = a 64-bit step counter read on the
// device; the first output word's top 24 bits are the uniform number.
#include "sampler_rows.h"

constexpr int LP_CHUNK = 4096;   // tokens per workgroup: 16 KB of counts + 16 KB of biases, five workgroups per CU
constexpr int LP_THREADS = 256;

template <int DT>
__device__ __forceinline__ void lp_load8(const void* p, int64_t i, int n, bool vec, float (&z)[8]) {
  if (vec && n == 8) {
    if constexpr (DT == LL_F32) {
      const f32x4 a = *reinterpret_cast<const f32x4*>((const float*)p + i);
      const f32x4 b = *reinterpret_cast<const f32x4*>((const float*)p + i + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        z[k] = a[k];
        z[4 + k] = b[k];
      }
    } else {
      uint16_t h[8];
      VecIO<8>::load((const uint16_t*)p + i, h);
#pragma unroll
      for (int k = 0; k < 8; ++k) z[k] = to_f32<DT>(h[k]);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = k < n ? ld_logit<DT>(p, i + k) : 0.f;
}

template <int DT>
__device__ __forceinline__ void lp_store8(void* p, int64_t i, int n, bool vec, const float (&x)[8]) {
  if (vec && n == 8) {
    if constexpr (DT == LL_F32) {
      f32x4 a, b;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = x[k];
        b[k] = x[4 + k];
      }
      *reinterpret_cast<f32x4*>((float*)p + i) = a;
      *reinterpret_cast<f32x4*>((float*)p + i + 4) = b;
    } else {
      uint16_t h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = from_f32<DT>(x[k]);
      VecIO<8>::store((uint16_t*)p + i, h);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < n) {
      if constexpr (DT == LL_F32) ((float*)p)[i + k] = x[k];
      else ((uint16_t*)p)[i + k] = from_f32<DT>(x[k]);
    }
  }
}

template <int DTI, int DTO>
__global__ __launch_bounds__(LP_THREADS) void logit_penalties_kernel(
    void* __restrict__ out, const void* __restrict__ logits, const int64_t* __restrict__ ids,
    const uint8_t* __restrict__ mask, const float* __restrict__ rep_rows, float rep_scalar,
    const float* __restrict__ pres_rows, float pres_scalar, const float* __restrict__ freq_rows, float freq_scalar,
    const int32_t* __restrict__ bias_offsets, const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_values,
    int64_t vocab, int64_t span, int64_t lstride, int64_t ostride, int64_t istride, int64_t mstride) {
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[LP_CHUNK];
  __shared__ __attribute__((aligned(16))) float s_bias[LP_CHUNK];
  const int64_t b = blockIdx.y;
  const int64_t c_lo = (int64_t)blockIdx.x * LP_CHUNK;
  const int64_t c_hi = c_lo + LP_CHUNK < vocab ? c_lo + LP_CHUNK : vocab;
  const int tid = threadIdx.x;
  const bool has_bias = bias_offsets != nullptr;

  // -0.0 is the additive identity that keeps the sign of a -0.0 logit
  for (int i = tid; i < LP_CHUNK / 4; i += LP_THREADS) {
    reinterpret_cast<i32x4*>(s_cnt)[i] = i32x4{0, 0, 0, 0};
    if (has_bias) reinterpret_cast<f32x4*>(s_bias)[i] = f32x4{-0.f, -0.f, -0.f, -0.f};
  }
  __syncthreads();
  for (int64_t j = tid; j < span; j += LP_THREADS) {
    if (!mask[b * mstride + j]) continue;
    const int64_t tok = ids[b * istride + j];
    if (tok < c_lo || tok >= c_hi) continue;  // another chunk's token, or an id outside the vocabulary
    atomicAdd(&s_cnt[tok - c_lo], 1u);
  }
  if (has_bias) {
    const int64_t e_lo = bias_offsets[b], e_hi = bias_offsets[b + 1];
    for (int64_t j = e_lo + tid; j < e_hi; j += LP_THREADS) {
      const int64_t tok = bias_ids[j];
      if (tok < c_lo || tok >= c_hi) continue;
      s_bias[tok - c_lo] = bias_values[j];  // a row names a token once
    }
  }
  __syncthreads();

  const float r = rep_rows ? rep_rows[b] : rep_scalar;
  const float p = pres_rows ? pres_rows[b] : pres_scalar;
  const float nf = -(freq_rows ? freq_rows[b] : freq_scalar);
  constexpr int ISZ = DTI == LL_F32 ? 4 : 2, OSZ = DTO == LL_F32 ? 4 : 2;
  // groups of eight tokens start at multiples of eight from the chunk's first token: 16-byte accesses when the chunk's
  // first element is 16-byte aligned in the row at hand
  const bool in_vec = (((uintptr_t)logits + (uint64_t)(b * lstride + c_lo) * ISZ) & 15u) == 0;
  const bool out_vec = (((uintptr_t)out + (uint64_t)(b * ostride + c_lo) * OSZ) & 15u) == 0;
#pragma unroll
  for (int g0 = 0; g0 < LP_CHUNK / 8; g0 += LP_THREADS) {
    const int t0 = (g0 + tid) * 8;  // offset in the chunk
    const int64_t left = c_hi - (c_lo + t0);
    if (left <= 0) break;
    const int n = left < 8 ? (int)left : 8;
    float x[8];
    lp_load8<DTI>(logits, b * lstride + c_lo + t0, n, in_vec, x);
    const i32x4 ca = reinterpret_cast<const i32x4*>(s_cnt)[t0 / 4], cb = reinterpret_cast<const i32x4*>(s_cnt)[t0 / 4 + 1];
    f32x4 ba = f32x4{-0.f, -0.f, -0.f, -0.f}, bb = ba;
    if (has_bias) {
      ba = reinterpret_cast<const f32x4*>(s_bias)[t0 / 4];
      bb = reinterpret_cast<const f32x4*>(s_bias)[t0 / 4 + 1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t c = (uint32_t)(k < 4 ? ca[k] : cb[k - 4]);
      float v = x[k] + (k < 4 ? ba[k] : bb[k - 4]);
      if (c > 0) v = v < 0.f ? v * r : v / r;
      v = __builtin_fmaf(nf, (float)c, v);
      v = v - (c > 0 ? p : 0.f);
      x[k] = v;
    }
    lp_store8<DTO>(out, b * ostride + c_lo + t0, n, out_vec, x);
  }
}

extern "C" int ll_logit_penalties(void* out, const void* logits, const int64_t* token_ids, const void* mask,
                                  const float* repetition_rows, float repetition_scalar, const float* presence_rows,
                                  float presence_scalar, const float* frequency_rows, float frequency_scalar,
                                  const int32_t* bias_offsets, const int32_t* bias_ids, const float* bias_values,
                                  int64_t batch, int64_t vocab, int64_t span, int64_t logits_stride, int64_t out_stride,
                                  int64_t ids_stride, int64_t mask_stride, int in_dtype, int out_dtype, void* stream) {
  if (batch < 0 || batch > 65535 || vocab <= 0 || vocab > (1ll << 40) || span < 0) return LL_ERR_SHAPE;
  if (!out || !logits || out == logits || (span > 0 && (!token_ids || !mask))) return LL_ERR_ARG;
  if (bias_offsets && (!bias_ids || !bias_values)) return LL_ERR_ARG;
  if (batch == 0) return LL_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((vocab + LP_CHUNK - 1) / LP_CHUNK), (unsigned)batch);
#define LL_LP(DTI, DTO)                                                                                                  \
  logit_penalties_kernel<DTI, DTO><<<grid, LP_THREADS, 0, st>>>(                                                         \
      out, logits, token_ids, (const uint8_t*)mask, repetition_rows, repetition_scalar, presence_rows, presence_scalar, \
      frequency_rows, frequency_scalar, bias_offsets, bias_ids, bias_values, vocab, span, logits_stride, out_stride,    \
      ids_stride, mask_stride)
  if (in_dtype == LL_F32 && out_dtype == LL_F32) LL_LP(LL_F32, LL_F32);
  else if (in_dtype == LL_F16 && out_dtype == LL_F16) LL_LP(LL_F16, LL_F16);
  else if (in_dtype == LL_F16 && out_dtype == LL_F32) LL_LP(LL_F16, LL_F32);
  else if (in_dtype == LL_BF16 && out_dtype == LL_BF16) LL_LP(LL_BF16, LL_BF16);
  else if (in_dtype == LL_BF16 && out_dtype == LL_F32) LL_LP(LL_BF16, LL_F32);
  else return LL_ERR_DTYPE;
#undef LL_LP
  return LL_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------- //
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
// ------------------------------------------------------------------------------------------- //
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)m1;
    c3 = (uint32_t)m0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__global__ __launch_bounds__(256) void seeded_uniform_kernel(float* __restrict__ out, const int64_t* __restrict__ seeds,
                                                             const int64_t* __restrict__ counter, int64_t batch) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const uint64_t seed = (uint64_t)seeds[b], c = counter ? (uint64_t)*counter : 0ull;
  const uint32_t w = philox_word0((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  out[b] = (float)(w >> 8) * 5.9604644775390625e-8f;  // 24 bits times 2^-24: exact, in [0, 1)
}

extern "C" int ll_seeded_uniform(float* out, const int64_t* seeds, const int64_t* counter, int64_t batch, void* stream) {
  if (batch < 0 || batch > (1ll << 31)) return LL_ERR_SHAPE;
  if (!out || !seeds) return LL_ERR_ARG;
  if (batch == 0) return LL_OK;
  seeded_uniform_kernel<<<dim3((unsigned)((batch + 255) / 256)), 256, 0, (hipStream_t)stream>>>(out, seeds, counter, batch);
  return LL_LAUNCH_CHECK();
}
