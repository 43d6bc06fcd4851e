// Sampler row: reference lite_llama/engine/sampler.py:77-137,199-270.
//   ll_repetition_penalty -- apply_repetition_penalty (:77-115): one scatter over the generated span.
//   ll_sample_top_p       -- softmax(logits / T) + nucleus filter (:118-137) + one draw per row from a
//                            caller-supplied uniform number, WITHOUT the reference's full sort.
// The nucleus is the set of tokens whose strictly-more-probable mass does not exceed top_p: with
// e_i = exp(z_i - max) and f(t) = sum of e_i > t, a token is kept iff f(e_i) <= top_p * sum(e).  The
// smallest t with f(t) <= P is itself a data value (f only jumps at data values); positive floats
// order like their bit patterns, so a bisection over the pattern (<= 30 passes of a cheap
// compare-accumulate over the row) finds it exactly; tokens
// tied at that value are kept in ascending index order while the mass before them fits (the
// reference leaves tie order to torch.sort); the draw is the inverse CDF over the kept tokens in index order (same distribution as the reference's
// torch.multinomial over the sorted row, different random stream).  One 1024-thread workgroup per row.
#include "sampler_rows.h"

template <int DT>
__device__ __forceinline__ void st_logit(void* p, int64_t i, float v) {
  if constexpr (DT == LL_F32) ((float*)p)[i] = v;
  else ((uint16_t*)p)[i] = from_f32<DT>(v);
}

// ------------------------------------------------------------------------------------------- //
// repetition penalty: out = logits, then for every (b, j) with mask: out[b, tok] = penalised value of
// the ORIGINAL logit (so repeated tokens are penalised once -- sampler.py:99-101).  out != logits.
// ------------------------------------------------------------------------------------------- //
// grid = (chunks, batch): a workgroup copies its chunk of the row and then applies the penalties of
// the span tokens that fall INTO that chunk (so no other workgroup's copy can overwrite them).
template <int DTI, int DTO>
__global__ __launch_bounds__(256) void rep_penalty_kernel(void* __restrict__ out, const void* __restrict__ logits,
                                                          const int64_t* __restrict__ ids,
                                                          const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ pen_rows, float pen_scalar,
                                                          int64_t vocab, int64_t span, int64_t lstride,
                                                          int64_t ostride, int64_t istride, int64_t mstride) {
  const int64_t b = blockIdx.y;
  const int64_t per = (vocab + gridDim.x - 1) / gridDim.x;
  const int64_t c_lo = (int64_t)blockIdx.x * per;
  const int64_t c_hi = c_lo + per < vocab ? c_lo + per : vocab;
  for (int64_t i = c_lo + threadIdx.x; i < c_hi; i += 256)
    st_logit<DTO>(out, b * ostride + i, ld_logit<DTI>(logits, b * lstride + i));
  __syncthreads();  // this chunk's copy is complete before any penalised value lands on it
  const float pen = pen_rows ? pen_rows[b] : pen_scalar;
  for (int64_t j = threadIdx.x; j < span; j += 256) {
    if (!mask[b * mstride + j]) continue;
    const int64_t tok = ids[b * istride + j];
    if (tok < c_lo || tok >= c_hi) continue;
    const float x = ld_logit<DTI>(logits, b * lstride + tok);
    st_logit<DTO>(out, b * ostride + tok, x < 0.f ? x * pen : x / pen);
  }
}

extern "C" int ll_repetition_penalty(void* out, const void* logits, const int64_t* token_ids, const void* mask,
                                     const float* penalty_rows, float penalty_scalar, int64_t batch,
                                     int64_t vocab, int64_t span, int64_t logits_stride, int64_t out_stride,
                                     int64_t ids_stride, int64_t mask_stride, int in_dtype, int out_dtype,
                                     void* stream) {
  if (batch < 0 || vocab <= 0 || span < 0) return LL_ERR_SHAPE;
  if (!out || !logits || out == logits || (span > 0 && (!token_ids || !mask))) return LL_ERR_ARG;
  if (batch == 0) return LL_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned chunks = (unsigned)((vocab + 8191) / 8192);  // ~8 K logits per workgroup
  if (chunks > 64) chunks = 64;
#define LL_RP(DTI, DTO)                                                                                   \
  rep_penalty_kernel<DTI, DTO><<<dim3(chunks, (unsigned)batch), 256, 0, st>>>(                            \
      out, logits, token_ids, (const uint8_t*)mask, penalty_rows, penalty_scalar, vocab, span, logits_stride, \
      out_stride, ids_stride, mask_stride)
  if (in_dtype == LL_F32 && out_dtype == LL_F32) LL_RP(LL_F32, LL_F32);
  else if (in_dtype == LL_F16 && out_dtype == LL_F16) LL_RP(LL_F16, LL_F16);
  else if (in_dtype == LL_F16 && out_dtype == LL_F32) LL_RP(LL_F16, LL_F32);
  else if (in_dtype == LL_BF16 && out_dtype == LL_BF16) LL_RP(LL_BF16, LL_BF16);
  else if (in_dtype == LL_BF16 && out_dtype == LL_F32) LL_RP(LL_BF16, LL_F32);
  else return LL_ERR_DTYPE;
#undef LL_RP
  return LL_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------- //
// nucleus sampling
// ------------------------------------------------------------------------------------------- //
// The row code lives in sampler_rows.h (ll_sample_filtered runs the same passes): one 1024-thread workgroup per row.
template <int DT>
__global__ __launch_bounds__(1024) void top_p_sample_kernel(int64_t* __restrict__ out, const void* __restrict__ logits,
                                                            const float* __restrict__ temperature,
                                                            const float* __restrict__ top_p,
                                                            const float* __restrict__ uniform,
                                                            const uint8_t* __restrict__ greedy, int64_t vocab,
                                                            int64_t stride) {
  __shared__ SampleShared s;
  const int64_t b = blockIdx.x;
  if (greedy && greedy[b]) {
    greedy_row<DT>(out, logits, b, b * stride, vocab, s);
    return;
  }
  nucleus_row<DT, false>(out, logits, temperature[b], top_p[b], uniform[b], -INFINITY, 0.f, b, b * stride, vocab, s);
}

extern "C" int ll_sample_top_p(int64_t* out, const void* logits, const float* temperature, const float* top_p,
                               const float* uniform, const void* greedy, int64_t batch, int64_t vocab,
                               int64_t stride, int dtype, void* stream) {
  if (batch < 0 || vocab <= 0) return LL_ERR_SHAPE;
  if (!out || !logits || !temperature || !top_p || !uniform) return LL_ERR_ARG;
  if (batch == 0) return LL_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)batch);
  if (dtype == LL_F32)
    top_p_sample_kernel<LL_F32><<<grid, 1024, 0, st>>>(out, logits, temperature, top_p, uniform, (const uint8_t*)greedy, vocab, stride);
  else if (dtype == LL_F16)
    top_p_sample_kernel<LL_F16><<<grid, 1024, 0, st>>>(out, logits, temperature, top_p, uniform, (const uint8_t*)greedy, vocab, stride);
  else if (dtype == LL_BF16)
    top_p_sample_kernel<LL_BF16><<<grid, 1024, 0, st>>>(out, logits, temperature, top_p, uniform, (const uint8_t*)greedy, vocab, stride);
  else return LL_ERR_DTYPE;
  return LL_LAUNCH_CHECK();
}
