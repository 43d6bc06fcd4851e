// Constrained decoding over a token automaton (executor extension; executor/constraints.py states the semantics, and
// tests/_constraint_ref.py restates them in plain Python).  The automaton is CSR over token ids: offsets[S + 1],
// tokens[E] strictly ascending inside a state, next_states[E]; a row's state is one int32.
//   ll_constrained_argmax -- in greedy_argmax's slot: a row in state s looks only at edges offsets[s] .. offsets[s + 1],
//       emits the token of the edge with the largest logit (stored value compared as fp32; first maximum in edge order =
//       lowest token id; all -inf: the first edge) and moves to that edge's next state.  One 1024-thread workgroup per
//       row: token ids are read coalesced, logits gathered.
//   ll_constraint_mask    -- out[b, :] = -inf except the allowed entries, copied bit for bit (the sampling route: the
//       nucleus sampler then draws from out).  grid = (chunks, batch): a workgroup fills its chunk of the row and then
//       copies the allowed entries that fall INTO that chunk, found by bisection in the sorted edge list.
//   ll_constraint_advance -- the state follows a token chosen elsewhere (bisection, one thread per row); an absent token
//       sets bit 1 of the sticky error word and leaves the state.
// A state outside [0, S) sets bit 2 of the error word; the row then emits token 0 / a fully masked row and keeps its state.
// A token id outside [0, vocab) is never used as an index: the edge counts as -inf (argmax) or is skipped (mask).
// finished (optional, int32 per row): rows with finished[b] != 0 keep their state (argmax: they emit their first edge's
// token, which the caller replaces with the pad).
#include "common.h"

namespace {

constexpr int kThreads = 256;
// the argmax's workgroup: a row is one workgroup, so its width is the row's memory parallelism (16 waves x 4 edges in flight)
constexpr int kArgmaxThreads = 1024;
constexpr int kWaves = kArgmaxThreads / LL_WAVE;
constexpr int kUnroll = 4;

template <int DT>
__device__ __forceinline__ float ld_logit(const void* p, int64_t i) {
  if constexpr (DT == LL_F32) return ((const float*)p)[i];
  else return to_f32<DT>(((const uint16_t*)p)[i]);
}

// (value, edge) pairs ordered by value descending, edge ascending; edge < 0: no candidate yet
__device__ __forceinline__ bool better(float ov, int oe, float v, int e) {
  return oe >= 0 && (e < 0 || ov > v || (ov == v && oe < e));
}

template <int DT>
__global__ __launch_bounds__(kArgmaxThreads) void constrained_argmax_kernel(
    int64_t* __restrict__ out, int32_t* __restrict__ states, const void* __restrict__ logits,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ tokens, const int32_t* __restrict__ next_states,
    const int32_t* __restrict__ finished, int32_t* __restrict__ error, int64_t vocab, int64_t stride, int num_states) {
  __shared__ float s_val[kWaves];
  __shared__ int s_edge[kWaves];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int s = states[b];
  if (s < 0 || s >= num_states) {  // uniform over the workgroup
    if (tid == 0) {
      atomicOr(error, 2);
      out[b] = 0;
    }
    return;
  }
  const int lo = offsets[s], hi = offsets[s + 1];
  if (finished && finished[b]) {
    if (tid == 0) out[b] = lo < hi ? tokens[lo] : 0;
    return;
  }
  const int64_t base = b * stride;
  float best = -INFINITY;
  int be = -1;
  // four edges per thread and pass: the four token ids (coalesced) are in flight together, then the four gathers
  for (int e0 = lo + tid; e0 < hi; e0 += kUnroll * kArgmaxThreads) {
    int tok[kUnroll];
    float v[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int e = e0 + j * kArgmaxThreads;
      tok[j] = e < hi ? tokens[e] : -1;
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) v[j] = tok[j] >= 0 && tok[j] < vocab ? ld_logit<DT>(logits, base + tok[j]) : -INFINITY;
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int e = e0 + j * kArgmaxThreads;
      if (e < hi && (be < 0 || v[j] > best)) {  // a thread's edges ascend: strict > keeps its first maximum
        best = v[j];
        be = e;
      }
    }
  }
#pragma unroll
  for (int off = LL_WAVE / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, LL_WAVE);
    const int oe = __shfl_xor(be, off, LL_WAVE);
    if (better(ov, oe, best, be)) {
      best = ov;
      be = oe;
    }
  }
  if ((tid & (LL_WAVE - 1)) == 0) {
    s_val[tid / LL_WAVE] = best;
    s_edge[tid / LL_WAVE] = be;
  }
  __syncthreads();  // also orders every thread's read of states[b] before the store below
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
      if (better(s_val[w], s_edge[w], best, be)) {
        best = s_val[w];
        be = s_edge[w];
      }
    if (be < 0) {  // a state without edges: refused when the automaton is built
      atomicOr(error, 2);
      out[b] = 0;
    } else {
      out[b] = tokens[be];
      states[b] = next_states[be];
    }
  }
}

// first edge in [lo, hi) whose token is >= t
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ tokens, int lo, int hi, int64_t t) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tokens[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// T: the storage word (uint16_t for fp16 / bf16, uint32_t for fp32); ninf: its -inf pattern
template <typename T>
__global__ __launch_bounds__(kThreads) void constraint_mask_kernel(T* __restrict__ out, const T* __restrict__ logits,
                                                                   const int32_t* __restrict__ states,
                                                                   const int32_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ tokens,
                                                                   int32_t* __restrict__ error, T ninf, int64_t vocab,
                                                                   int64_t lstride, int64_t ostride, int num_states,
                                                                   int64_t per, int vec_ok) {
  constexpr int kVec = 16 / (int)sizeof(T);
  const int64_t b = blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t c_lo = (int64_t)blockIdx.x * per;  // per is a multiple of kVec
  const int64_t c_hi = c_lo + per < vocab ? c_lo + per : vocab;
  if (c_lo >= c_hi) return;
  T* orow = out + b * ostride;
  int64_t i0 = c_lo;
  if (vec_ok) {  // rows 16-byte aligned: whole 16-byte stores, then the tail
    struct alignas(16) Vec {
      T v[kVec];
    };
    Vec fill;
#pragma unroll
    for (int j = 0; j < kVec; ++j) fill.v[j] = ninf;
    const int64_t n_vec = (c_hi - c_lo) / kVec;
    Vec* dst = reinterpret_cast<Vec*>(orow + c_lo);
    for (int64_t i = tid; i < n_vec; i += kThreads) dst[i] = fill;
    i0 = c_lo + n_vec * kVec;
  }
  for (int64_t i = i0 + tid; i < c_hi; i += kThreads) orow[i] = ninf;
  const int s = states[b];
  if (s < 0 || s >= num_states) {
    if (tid == 0 && blockIdx.x == 0) atomicOr(error, 2);
    return;
  }
  __syncthreads();  // this chunk's fill is complete before any allowed value lands on it
  const int lo = offsets[s], hi = offsets[s + 1];
  const int e_lo = lower_bound(tokens, lo, hi, c_lo), e_hi = lower_bound(tokens, e_lo, hi, c_hi);
  const T* lrow = logits + b * lstride;
  for (int e = e_lo + tid; e < e_hi; e += kThreads) {
    const int64_t tok = tokens[e];
    if (tok >= c_lo && tok < c_hi) orow[tok] = lrow[tok];  // always true for a sorted list; never index outside the chunk
  }
}

__global__ __launch_bounds__(kThreads) void constraint_advance_kernel(int32_t* __restrict__ states,
                                                                      const int64_t* __restrict__ chosen,
                                                                      const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ tokens,
                                                                      const int32_t* __restrict__ next_states,
                                                                      const int32_t* __restrict__ finished,
                                                                      int32_t* __restrict__ error, int batch,
                                                                      int num_states) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= batch || (finished && finished[i])) return;
  const int s = states[i];
  if (s < 0 || s >= num_states) {
    atomicOr(error, 2);
    return;
  }
  const int lo = offsets[s], hi = offsets[s + 1];
  const int64_t tok = chosen[i];
  const int e = lower_bound(tokens, lo, hi, tok);
  if (e < hi && tokens[e] == tok) states[i] = next_states[e];
  else atomicOr(error, 1);
}

}  // namespace

extern "C" int ll_constrained_argmax(int64_t* out, int32_t* states, const void* logits, const int32_t* offsets,
                                     const int32_t* tokens, const int32_t* next_states, const int32_t* finished,
                                     int32_t* error, int64_t batch, int64_t vocab, int64_t stride, int num_states,
                                     int dtype, void* stream) {
  if (batch < 0 || batch > INT32_MAX || vocab <= 0 || vocab > INT32_MAX || stride < vocab || num_states < 1)
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!out || !states || !logits || !offsets || !tokens || !next_states || !error) return LL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)batch);
#define LL_CA(DT)                                                                                                     \
  constrained_argmax_kernel<DT><<<grid, kArgmaxThreads, 0, st>>>(out, states, logits, offsets, tokens, next_states,     \
                                                                 finished, error, vocab, stride, num_states)
  if (dtype == LL_F32) LL_CA(LL_F32);
  else if (dtype == LL_F16) LL_CA(LL_F16);
  else if (dtype == LL_BF16) LL_CA(LL_BF16);
  else return LL_ERR_DTYPE;
#undef LL_CA
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_constraint_mask(void* out, const void* logits, const int32_t* states, const int32_t* offsets,
                                  const int32_t* tokens, int32_t* error, int64_t batch, int64_t vocab,
                                  int64_t logits_stride, int64_t out_stride, int num_states, int dtype, void* stream) {
  if (batch < 0 || batch > 65535 || vocab <= 0 || vocab > INT32_MAX || logits_stride < vocab || out_stride < vocab ||
      num_states < 1)
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!out || !logits || out == logits || !states || !offsets || !tokens || !error) return LL_ERR_ARG;
  if (dtype != LL_F32 && dtype != LL_F16 && dtype != LL_BF16) return LL_ERR_DTYPE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t elt = dtype == LL_F32 ? 4 : 2;
  int64_t chunks = (vocab + 8191) / 8192;  // ~8 K logits per workgroup
  if (chunks > 64) chunks = 64;
  const int64_t per = ((vocab + chunks - 1) / chunks + 7) / 8 * 8;
  const int vec_ok = ll_aligned16(out) && (out_stride * elt) % 16 == 0;
  const dim3 grid((unsigned)chunks, (unsigned)batch);
  if (dtype == LL_F32)
    constraint_mask_kernel<uint32_t><<<grid, kThreads, 0, st>>>((uint32_t*)out, (const uint32_t*)logits, states, offsets,
                                                                tokens, error, 0xFF800000u, vocab, logits_stride,
                                                                out_stride, num_states, per, vec_ok);
  else
    constraint_mask_kernel<uint16_t><<<grid, kThreads, 0, st>>>((uint16_t*)out, (const uint16_t*)logits, states, offsets,
                                                                tokens, error,
                                                                (uint16_t)(dtype == LL_F16 ? 0xFC00u : 0xFF80u), vocab,
                                                                logits_stride, out_stride, num_states, per, vec_ok);
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_constraint_advance(int32_t* states, const int64_t* chosen, const int32_t* offsets,
                                     const int32_t* tokens, const int32_t* next_states, const int32_t* finished,
                                     int32_t* error, int64_t batch, int num_states, void* stream) {
  if (batch < 0 || batch > INT32_MAX || num_states < 1) return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!states || !chosen || !offsets || !tokens || !next_states || !error) return LL_ERR_ARG;
  constraint_advance_kernel<<<dim3((unsigned)((batch + kThreads - 1) / kThreads)), kThreads, 0, (hipStream_t)stream>>>(
      states, chosen, offsets, tokens, next_states, finished, error, (int)batch, num_states);
  return LL_LAUNCH_CHECK();
}
