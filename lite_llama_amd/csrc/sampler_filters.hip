// ll_sample_filtered: top-k and min-p on top of the nucleus sampler, one launch, one 1024-thread workgroup per row.
// Per row, with p = softmax(stored logit / T), T > 0:
//   1. top-k: v = the k-th largest STORED logit; the survivors are all tokens with logit >= v (every token tied with the
//      k-th survives).  k <= 0 or k >= vocab: off.  -inf sorts last; v = -inf keeps everything.
//   2. top-p over the survivors: ll_sample_top_p's rule restricted to them (the nucleus mass is top_p * their mass; ties at
//      the threshold rationed in ascending index order).
//   3. min-p: a kept token with p_i < min_p * p_max is dropped -- e_i < min_p in fp32, the maximum's e being exp2(0) = 1.
//      It acts AFTER the nucleus has been chosen.  0: off.
//   4. the draw: inverse CDF in token order over what is left, as ll_sample_top_p.
// The maximum survives all three, so the set is never empty.
//
// Selection: the k-th largest value is found by bisection over an order-preserving integer key of the stored value
// (16 bits for fp16 / bf16, 32 for fp32): "how many logits are >= the value of this key" is a load and a compare per
// token, counted per lane and added up across the wave and the workgroup -- an exact integer -- and the largest key that
// still counts k is the k-th value.  16 (fp32: 32) such passes over a row that the nucleus bisection then reads ~30 more
// times through the exp2 unit.
// A row with both filters off runs nucleus_row<DT, false>, the code of ll_sample_top_p: the same tokens.
#include "sampler_rows.h"

// key <-> stored bits: positive values keep their order with the sign bit set, negative ones are complemented
template <int DT>
struct LogitKey {
  static constexpr uint32_t SIGN = DT == LL_F32 ? 0x80000000u : 0x8000u;
  static constexpr uint32_t ALL = DT == LL_F32 ? 0xFFFFFFFFu : 0xFFFFu;
  static constexpr uint32_t PINF = DT == LL_F32 ? 0x7F800000u : (DT == LL_F16 ? 0x7C00u : 0x7F80u);
  static constexpr uint32_t LO = ~(PINF | SIGN) & ALL;  // key of -inf
  static constexpr uint32_t HI = PINF | SIGN;           // key of +inf: no NaN pattern lies between the two
  static __device__ __forceinline__ float value(uint32_t key) {
    const uint32_t bits = (key & SIGN) ? key ^ SIGN : ~key & ALL;
    if constexpr (DT == LL_F32) return __uint_as_float(bits);
    else return to_f32<DT>((uint16_t)bits);
  }
};

// The k-th largest stored logit of the row, 0 < kk < vocab.  count(t) = tokens with logit >= value(t) falls as t grows and
// count(LO) = vocab >= kk: the largest t with count(t) >= kk is the key of the k-th value.  (+0 and -0 count alike and
// compare alike afterwards.)
template <int DT>
__device__ __forceinline__ float kth_largest(const void* __restrict__ logits, int64_t base, int64_t vocab, int64_t kk,
                                             SampleShared& s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const RowSegment sg = row_segment(vocab);
  uint32_t lo = LogitKey<DT>::LO, hi = LogitKey<DT>::HI;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    const float tv = LogitKey<DT>::value(mid);
    int c = 0;  // per lane, the form of the nucleus passes: eight independent loads in flight per lane
#pragma unroll 8
    for (int64_t i = sg.lo + lane; i < sg.hi; i += 64) c += ld_logit<DT>(logits, base + i) >= tv ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    __syncthreads();  // cnt may still be read from the previous pass
    if (lane == 0) s.cnt[w] = c;
    __syncthreads();
    int64_t total = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) total += s.cnt[j];
    if (total >= kk) lo = mid;
    else hi = mid - 1;
  }
  return LogitKey<DT>::value(lo);
}

template <int DT>
__global__ __launch_bounds__(1024) void filtered_sample_kernel(int64_t* __restrict__ out, const void* __restrict__ logits,
                                                               const float* __restrict__ temperature,
                                                               const float* __restrict__ top_p,
                                                               const int32_t* __restrict__ top_k,
                                                               const float* __restrict__ min_p,
                                                               const float* __restrict__ uniform,
                                                               const uint8_t* __restrict__ greedy, int64_t vocab,
                                                               int64_t stride) {
  __shared__ SampleShared s;
  const int64_t b = blockIdx.x;
  const int64_t base = b * stride;
  if (greedy && greedy[b]) {
    greedy_row<DT>(out, logits, b, base, vocab, s);
    return;
  }
  const int64_t kk = top_k ? top_k[b] : 0;
  const bool k_on = kk > 0 && kk < vocab;
  float mp = min_p ? min_p[b] : 0.f;
  mp = mp > 0.f ? fminf(mp, 1.f) : 0.f;  // the maximum (e = 1) always stays; a negative or NaN min_p is off
  if (!k_on && mp == 0.f) {  // both off: the nucleus sampler itself
    nucleus_row<DT, false>(out, logits, temperature[b], top_p[b], uniform[b], -INFINITY, 0.f, b, base, vocab, s);
    return;
  }
  const float v = k_on ? kth_largest<DT>(logits, base, vocab, kk, s) : -INFINITY;
  nucleus_row<DT, true>(out, logits, temperature[b], top_p[b], uniform[b], v, mp, b, base, vocab, s);
}

extern "C" int ll_sample_filtered(int64_t* out, const void* logits, const float* temperature, const float* top_p,
                                  const int32_t* top_k, const float* min_p, const float* uniform, const void* greedy,
                                  int64_t batch, int64_t vocab, int64_t stride, int dtype, void* stream) {
  if (batch < 0 || vocab <= 0) return LL_ERR_SHAPE;
  if (!out || !logits || !temperature || !top_p || !uniform) return LL_ERR_ARG;
  if (batch == 0) return LL_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)batch);
#define LL_SF(DT)                                                                                                    \
  filtered_sample_kernel<DT><<<grid, 1024, 0, st>>>(out, logits, temperature, top_p, top_k, min_p, uniform,        \
                                                     (const uint8_t*)greedy, vocab, stride)
  if (dtype == LL_F32) LL_SF(LL_F32);
  else if (dtype == LL_F16) LL_SF(LL_F16);
  else if (dtype == LL_BF16) LL_SF(LL_BF16);
  else return LL_ERR_DTYPE;
#undef LL_SF
  return LL_LAUNCH_CHECK();
}
