// Row-level device code shared by the sampling kernels (sampler.hip: ll_sample_top_p; sampler_filters.hip:
// ll_sample_filtered): one 1024-thread workgroup owns one row of logits.
//   greedy_row   -- first argmax of the stored values.
//   nucleus_row  -- softmax(logit / T) + nucleus + one inverse-CDF draw.  FILT = false is the nucleus sampler as
//                   ll_sample_top_p has always run it; FILT = true runs the SAME passes in the same order with an "alive"
//                   predicate (top-k: logit >= v) and a min-p floor on the kept set, so v = -inf, min_p = 0 reproduces
//                   FILT = false bit for bit.
#pragma once
#include "common.h"

template <int DT>
__device__ __forceinline__ float ld_logit(const void* p, int64_t i) {
  if constexpr (DT == LL_F32) return ((const float*)p)[i];
  else return to_f32<DT>(((const uint16_t*)p)[i]);
}

struct SampleShared {
  float sh[16];
  float gw[16], cw[16];
  int64_t idx[16];
  int cnt[16];
};

__device__ __forceinline__ float block_sum_1024(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) t += sh[i];  // same order in every thread: identical result everywhere
  return t;
}
__device__ __forceinline__ float block_max_1024(float v, float* sh) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float t = sh[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) t = fmaxf(t, sh[i]);
  return t;
}

// e_i = exp(z_i - max) through the hardware exp2 (one v_exp_f32, ~1 ulp): the whole kernel is a few
// dozen passes over the row and is instruction-issue bound, so the libm expf (~20 instructions) would
// dominate it; equal logits still give equal e, which is all the tie rule needs.
__device__ __forceinline__ float fast_e(float l, float k, float mk) { return __builtin_amdgcn_exp2f(l * k - mk); }

// Row layout: wave w owns the contiguous segment [w*seg, (w+1)*seg) and walks it 64 tokens at a time
// with lane = token offset, so every load is one coalesced 128-B (fp16) request; token order is
// (wave, iteration, lane), which is what the final inverse-CDF walk needs.
struct RowSegment {
  int64_t lo, hi;
};
__device__ __forceinline__ RowSegment row_segment(int64_t vocab) {
  const int w = threadIdx.x >> 6;
  const int64_t seg = ((vocab + 15) / 16 + 63) / 64 * 64;
  const int64_t s_lo = w * seg < vocab ? w * seg : vocab;
  const int64_t s_hi = s_lo + seg < vocab ? s_lo + seg : vocab;
  return {s_lo, s_hi};
}

// temperature == 0 rows: first maximum, like torch.argmax
template <int DT>
__device__ __forceinline__ void greedy_row(int64_t* __restrict__ out, const void* __restrict__ logits, int64_t b,
                                           int64_t base, int64_t vocab, SampleShared& s) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const RowSegment sg = row_segment(vocab);
  const int64_t s_lo = sg.lo, s_hi = sg.hi;
  float best = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int64_t i = s_lo + lane; i < s_hi; i += 64) {
    const float v = ld_logit<DT>(logits, base + i);
    if (bi == INT64_MAX || v > best) {  // per-lane indices ascend: strict > keeps the first max
      best = v;
      bi = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int64_t oi = __shfl_xor(bi, off, 64);
    if (oi != INT64_MAX && (bi == INT64_MAX || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    s.sh[w] = best;
    s.idx[w] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < 16; ++j)
      if (s.idx[j] != INT64_MAX && (bi == INT64_MAX || s.sh[j] > best || (s.sh[j] == best && s.idx[j] < bi))) {
        best = s.sh[j];
        bi = s.idx[j];
      }
    out[b] = bi;
  }
}

// One draw of row b at u from the nucleus of softmax(logit / T).  FILT: only tokens with logit >= v are alive (a dead
// token reads as e = -1: it is above no threshold, tied with none and carries no mass), the nucleus is chosen among the
// alive ones, and a kept token with e < min_p is dropped afterwards (e of the maximum is exp2(0) = 1, so e is p / p_max).
template <int DT, bool FILT>
__device__ __forceinline__ void nucleus_row(int64_t* __restrict__ out, const void* __restrict__ logits, float T,
                                            float top_p, float u, float v, float min_p, int64_t b, int64_t base,
                                            int64_t vocab, SampleShared& s) {
  float* sh = s.sh;
  float* gw = s.gw;
  float* cw = s.cw;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const RowSegment sg = row_segment(vocab);
  const int64_t s_lo = sg.lo, s_hi = sg.hi;

  // z = logit / T evaluated as logit * (1 / T): equal logits stay equal
  const float k = 1.4426950408889634f / T;  // log2(e) / T
  float mk = -INFINITY;
  for (int64_t i = s_lo + lane; i < s_hi; i += 64) mk = fmaxf(mk, ld_logit<DT>(logits, base + i) * k);
  mk = block_max_1024(mk, sh);  // the maximum is alive under every v the selection returns
  auto e_at = [&](int64_t i) -> float {
    const float l = ld_logit<DT>(logits, base + i);
    const float e = fast_e(l, k, mk);
    if constexpr (FILT) return l >= v ? e : -1.f;
    else return e;
  };
  float sum = 0.f;
  for (int64_t i = s_lo + lane; i < s_hi; i += 64) {
    const float e = e_at(i);
    if constexpr (FILT) sum += e < 0.f ? 0.f : e;
    else sum += e;
  }
  const float S = block_sum_1024(sum, sh);
  const float P = top_p * S;

  // tau = the smallest kept value = smallest t with (mass of e > t) <= P.  Positive floats order
  // like their bit patterns: bisection over the pattern in [0, 1.0f] (f(1.0) = 0 <= P always holds).
  uint32_t blo = 0, bhi = 0x3F800000u;
  float G = 0.f;  // mass strictly above the current upper bound
  while (blo < bhi) {
    const uint32_t mid = blo + ((bhi - blo) >> 1);
    const float t = __uint_as_float(mid);
    float a = 0.f;
#pragma unroll 8
    for (int64_t i = s_lo + lane; i < s_hi; i += 64) {
      const float e = e_at(i);
      a += e > t ? e : 0.f;
    }
    a = block_sum_1024(a, sh);
    if (a <= P) {
      bhi = mid;
      G = a;
    } else {
      blo = mid + 1;
    }
  }
  const float tau = __uint_as_float(bhi);
  // min-p acts on the chosen nucleus: everything kept above tau and below the floor goes, and so do the ties at tau when
  // tau itself is below it
  const bool drop_ties = FILT && tau < min_p;

  // per-segment kept mass; tokens tied at tau are kept in ascending index order while the mass
  // before them fits (the first n_tie of the row)
  float g_mine = 0.f, c_mine = 0.f;
  for (int64_t i = s_lo + lane; i < s_hi; i += 64) {
    const float e = e_at(i);
    if constexpr (FILT) {
      g_mine += e > tau && e >= min_p ? e : 0.f;
      c_mine += e == tau && !drop_ties ? 1.f : 0.f;
    } else {
      g_mine += e > tau ? e : 0.f;
      c_mine += e == tau ? 1.f : 0.f;
    }
  }
  g_mine = wave_sum(g_mine);
  c_mine = wave_sum(c_mine);  // counts <= vocab: exact in fp32
  __syncthreads();
  if (lane == 0) {
    gw[w] = g_mine;
    cw[w] = c_mine;
  }
  __syncthreads();
  float C = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) C += cw[j];
  float n_tie = C;  // tau == 0 (top_p = 1 keeps everything): nothing to ration
  if (tau > 0.f && C > 0.f) {
    n_tie = floorf((P - G) / tau) + 1.f;
    n_tie = n_tie < 1.f ? 1.f : (n_tie > C ? C : n_tie);
  }
  // every thread walks the 16 segment totals in the same order: Z, the chosen segment, the mass and
  // the kept ties before it
  float Z = 0.f, ties_seen = 0.f;
  float seg_mass[16], seg_ties[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float kt = n_tie - ties_seen;
    kt = kt < 0.f ? 0.f : (kt > cw[j] ? cw[j] : kt);
    seg_ties[j] = kt;
    seg_mass[j] = gw[j] + tau * kt;
    Z += seg_mass[j];
    ties_seen += cw[j];
  }
  const float target = u * Z;
  int pick_w = -1, last_w = -1;
  float before = 0.f, run = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (seg_mass[j] > 0.f) {
      last_w = j;
      if (pick_w < 0 && target < run + seg_mass[j]) {
        pick_w = j;
        before = run;
      }
    }
    run += seg_mass[j];
  }
  bool overflow = false;
  if (pick_w < 0) {  // target landed on / beyond the total because of rounding (u ~ 1)
    pick_w = last_w;
    overflow = true;
  }
  if (w != pick_w) return;

  // the chosen wave walks its segment in index order
  float ties_left = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) ties_left = j == pick_w ? seg_ties[j] : ties_left;
  float acc_run = before;
  int64_t pick = -1, last_kept = -1;
  for (int64_t i0 = s_lo; i0 < s_hi && pick < 0; i0 += 64) {
    const int64_t i = i0 + lane;
    const float e = i < s_hi ? e_at(i) : -1.f;
    const bool is_tie = e == tau;
    const unsigned long long tb = __ballot(is_tie);
    const float rank = (float)__popcll(tb & ((1ull << lane) - 1ull));
    bool keep;  // with drop_ties no tie was counted, so ties_left is 0 and none is kept
    if constexpr (FILT) keep = (e > tau && e >= min_p) || (is_tie && rank < ties_left);
    else keep = e > tau || (is_tie && rank < ties_left);
    float incl = keep ? e : 0.f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    // the fallback names a token that carries mass: with top_p = 1 tau is 0, so zero-mass tokens (e == 0: a -inf or an
    // underflowed logit) count as kept ties, and one of them after the last positive token must not be the answer
    const unsigned long long kb = __ballot(keep && e > 0.f);
    if (kb) last_kept = i0 + (63 - __builtin_clzll(kb));
    const unsigned long long hit = __ballot(keep && acc_run + incl > target);
    if (hit && !overflow) {
      pick = i0 + (__builtin_ffsll((long long)hit) - 1);
      break;
    }
    acc_run += __shfl(incl, 63, 64);
    float kept_ties = (float)__popcll(tb);
    kept_ties = kept_ties < ties_left ? kept_ties : ties_left;
    ties_left -= kept_ties;
  }
  if (lane == 0) out[b] = pick >= 0 ? pick : last_kept;  // fp rounding: the segment's last kept token
}
