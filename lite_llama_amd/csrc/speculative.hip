// Greedy speculative decoding: the two launches a verify step adds around the model's forward (executor extension;
// executor/speculative.py states the semantics, tests/_spec_ref.py is their plain-Python form).  A row's history is its
// prompt, the token prefill returned and the tokens it emitted: hist_len tokens, of which ctx = hist_len - 1 are cached.
//
// ll_spec_draft, one workgroup per row, writes the step's [k + 1] grid row: column 0 = history[hist_len - 1], columns
// 1 .. d a draft, token 0 beyond; q_len = 1 + d, ctx_len = ctx, positions[j] = ctx + min(j, d) (pads are clamped so that no
// rope-table index leaves max_seq_len).  A finished row gets q_len = 0: the pool pops nothing for it, its cells go to the
// junk block and nobody reads its logits.  The draft: for n = min(max_ngram, hist_len) down to min_ngram the last n tokens
// are looked up (a) in the caller's prediction -- among the ends e (n <= e < pred_len, predicted[e - n : e] == suffix) the
// one nearest to `emitted` (the aligned position), ties to the larger e -- then (b) in the history itself -- the largest
// end e, n <= e < hist_len.  The first n with a candidate decides; the draft is source[e : e + d], d = min(lim, source_len
// - e), lim = min(k, remaining - 1, max_seq_len - hist_len - 1): a step can neither emit past the output row nor outgrow
// the table row.  It may overlap the suffix (periodic text).
//   The row's history is staged ONCE: into LDS while hist_len <= kLdsTokens (4096 tokens, 16 KB), read from global memory
//   beyond that (the candidate loops are the same; only the accessor differs).  Candidate ends are strided over the
//   threads and compared last-token-first; the selected end is a workgroup maximum of one 64-bit key.
//
// ll_spec_accept, after the argmax over the B (k + 1) logits rows, one workgroup, rows strided over the threads: a = the
// number of leading j < d with ids[j + 1] == argmax[j]; the candidates argmax[0 .. a] are appended in order to out (column
// 1 + emitted) and to the history, stopping after the first that is a stop id (reason 1), that brings the count to
// max_tokens (reason 3) or to max_new_tokens (finished, reason 0).  Finished rows are not touched.  running[0] = rows still
// running, reduced in LDS and written once; the step counter (a device word, so that a captured step replays) moves on.
// Rejected positions need no rollback: their K/V sits at positions >= the row's new ctx, which the next step's extend
// names again (same blocks, same cells) and overwrites before anything reads them.
// Plain vector loads and stores only; no length is read from the host.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsTokens = LL_SPEC_LDS_TOKENS;

// workgroup maximum of one value per thread; ends on a barrier, so `red` can be used again at once
__device__ __forceinline__ long long block_max(long long v, long long* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      const long long o = red[tid + off];
      if (o > red[tid]) red[tid] = o;
    }
    __syncthreads();
  }
  const long long r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void spec_draft_kernel(
    const int32_t* __restrict__ history, int64_t hist_stride, const int32_t* __restrict__ hist_len,
    const int32_t* __restrict__ emitted, const int32_t* __restrict__ finished, const int32_t* __restrict__ max_tokens,
    int max_new_tokens, int max_seq_len, int k, int max_ngram, int min_ngram, int use_ngram,
    const int32_t* __restrict__ predicted, int64_t pred_stride, int pred_cols, const int32_t* __restrict__ pred_lens,
    int64_t* __restrict__ ids, int64_t* __restrict__ positions, int32_t* __restrict__ q_len, int32_t* __restrict__ ctx_len) {
  __shared__ int32_t s_hist[kLdsTokens];
  __shared__ long long s_red[kThreads];
  __shared__ int32_t s_suffix[LL_SPEC_MAX_NGRAM];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int32_t* row = history + (int64_t)b * hist_stride;
  int hl = hist_len[b];
  hl = hl < 1 ? 1 : hl > max_seq_len ? max_seq_len : hl;
  const int ctx = hl - 1;
  int64_t* my_ids = ids + (int64_t)b * (k + 1);
  int64_t* my_pos = positions + (int64_t)b * (k + 1);
  if (finished[b] != 0) {  // uniform over the workgroup
    if (tid <= k) {
      my_ids[tid] = 0;
      my_pos[tid] = ctx;
    }
    if (tid == 0) {
      q_len[b] = 0;
      ctx_len[b] = ctx;
    }
    return;
  }
  int cap = max_new_tokens;
  if (max_tokens && max_tokens[b] < cap) cap = max_tokens[b];
  int lim = cap - emitted[b] - 1;
  if (lim > k) lim = k;
  if (lim > max_seq_len - hl - 1) lim = max_seq_len - hl - 1;
  if (lim < 0) lim = 0;

  const bool in_lds = hl <= kLdsTokens;  // the staging switch
  if (in_lds)
    for (int i = tid; i < hl; i += kThreads) s_hist[i] = row[i];
  const int nmax = max_ngram < hl ? max_ngram : hl;
  if (tid < nmax) s_suffix[tid] = row[hl - nmax + tid];
  __syncthreads();
  auto at = [&](int i) -> int32_t { return in_lds ? s_hist[i] : row[i]; };

  const int32_t* pred = predicted ? predicted + (int64_t)b * pred_stride : nullptr;
  int pl = 0;
  if (pred) {
    pl = pred_lens ? pred_lens[b] : pred_cols;
    pl = pl < 0 ? 0 : pl > pred_cols ? pred_cols : pl;
  }
  const int em = emitted[b];
  int source = 0, end = 0;  // source: 0 none, 1 the prediction, 2 the history
  if (lim > 0) {
    for (int n = nmax; n >= min_ngram && n >= 1 && !source; --n) {
      const int32_t* suf = s_suffix + (nmax - n);
      if (pred) {
        long long key = -1;
        for (int e = n + tid; e < pl; e += kThreads) {
          bool hit = true;
          for (int j = n - 1; j >= 0 && hit; --j) hit = pred[e - n + j] == suf[j];
          if (hit) {
            const int dist = e > em ? e - em : em - e;
            const long long cand = ((long long)((1 << 30) - dist) << 32) | (long long)e;
            if (cand > key) key = cand;
          }
        }
        key = block_max(key, s_red);
        if (key >= 0) {
          source = 1;
          end = (int)(key & 0xffffffffll);
        }
      }
      if (!source && use_ngram) {
        long long key = -1;
        for (int e = n + tid; e < hl; e += kThreads) {
          bool hit = true;
          for (int j = n - 1; j >= 0 && hit; --j) hit = at(e - n + j) == suf[j];
          if (hit && e > key) key = e;
        }
        key = block_max(key, s_red);
        if (key >= 0) {
          source = 2;
          end = (int)key;
        }
      }
    }
  }
  int d = 0;
  if (source) {
    const int left = (source == 1 ? pl : hl) - end;
    d = lim < left ? lim : left;
  }
  if (tid <= k) {
    int32_t tok = 0;
    if (tid == 0) tok = at(hl - 1);
    else if (tid <= d) tok = source == 1 ? pred[end + tid - 1] : at(end + tid - 1);
    my_ids[tid] = tok;
    my_pos[tid] = ctx + (tid < d ? tid : d);
  }
  if (tid == 0) {
    q_len[b] = 1 + d;
    ctx_len[b] = ctx;
  }
}

__global__ __launch_bounds__(kThreads) void spec_accept_kernel(
    const int64_t* __restrict__ argmax, const int64_t* __restrict__ ids, const int32_t* __restrict__ q_len,
    int64_t* __restrict__ out, int64_t out_stride, int64_t out_cols, int32_t* __restrict__ history, int64_t hist_stride,
    int hist_cols, int32_t* __restrict__ hist_len, int32_t* __restrict__ emitted, int32_t* __restrict__ finished,
    int32_t* __restrict__ lengths, int32_t* __restrict__ reasons, const int32_t* __restrict__ max_tokens,
    int max_new_tokens, const int64_t* __restrict__ stop_ids, int n_ids, int32_t* __restrict__ verify_steps,
    int32_t* __restrict__ drafted, int32_t* __restrict__ accepted, int32_t* __restrict__ per_step, int64_t per_step_stride,
    int per_step_cols, int32_t* __restrict__ step, int32_t* __restrict__ running, int batch, int k) {
  __shared__ int64_t s_ids[LL_STOP_MAX_IDS];
  __shared__ int s_count[kThreads / LL_WAVE];
  const int tid = threadIdx.x;
  const int st = step[0];
  if (tid < n_ids) s_ids[tid] = stop_ids[tid];
  __syncthreads();
  int live = 0;
  for (int i = tid; i < batch; i += kThreads) {
    if (finished[i] != 0) continue;  // frozen: nothing of the row moves
    const int64_t* am = argmax + (int64_t)i * (k + 1);
    const int64_t* mine = ids + (int64_t)i * (k + 1);
    int d = q_len[i] - 1;
    d = d < 0 ? 0 : d > k ? k : d;
    int a = 0;
    while (a < d && mine[a + 1] == am[a]) ++a;
    int em = emitted[i], hl = hist_len[i], kept = 0, reason = 0;
    bool done = false;
    int64_t* orow = out + (int64_t)i * out_stride;
    int32_t* hrow = history + (int64_t)i * hist_stride;
    for (int j = 0; j <= a && !done; ++j) {
      if (1 + em >= out_cols) {  // no column left: never past the output row
        done = true;
        break;
      }
      const int64_t tok = am[j];
      orow[1 + em] = tok;
      if (hl < hist_cols) hrow[hl++] = (int32_t)tok;  // the last token of a row that fills max_seq_len has no cell, and no reader
      ++em;
      ++kept;
      for (int q = 0; q < n_ids; ++q)
        if (s_ids[q] == tok) reason = 1;
      if (!reason && max_tokens && em >= max_tokens[i]) reason = 3;
      done = reason != 0 || em >= max_new_tokens;
    }
    emitted[i] = em;
    hist_len[i] = hl;
    lengths[i] = em;
    if (done) {
      finished[i] = 1;
      reasons[i] = reason;
    } else {
      ++live;
    }
    verify_steps[i] += 1;
    drafted[i] += d;
    accepted[i] += kept > 0 ? kept - 1 : 0;
    if (st >= 0 && st < per_step_cols) per_step[(int64_t)i * per_step_stride + st] = kept > 0 ? kept - 1 : 0;
  }
#pragma unroll
  for (int off = LL_WAVE / 2; off > 0; off >>= 1) live += __shfl_down(live, off, LL_WAVE);
  if ((tid & (LL_WAVE - 1)) == 0) s_count[tid / LL_WAVE] = live;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / LL_WAVE; ++w) total += s_count[w];
    running[0] = total;
    step[0] = st + 1;
  }
}

}  // namespace

extern "C" int ll_spec_draft(const int32_t* history, int64_t history_stride, const int32_t* hist_len,
                             const int32_t* emitted, const int32_t* finished, const int32_t* max_tokens,
                             int max_new_tokens, int max_seq_len, int num_draft_tokens, int max_ngram, int min_ngram,
                             int use_ngram, const int32_t* predicted, int64_t predicted_stride, int predicted_cols,
                             const int32_t* predicted_lens, int64_t* ids, int64_t* positions, int32_t* q_len,
                             int32_t* ctx_len, int64_t batch, void* stream) {
  if (batch < 0 || batch > INT32_MAX || num_draft_tokens < 1 || num_draft_tokens > LL_SPEC_MAX_DRAFT || min_ngram < 1 ||
      max_ngram < min_ngram || max_ngram > LL_SPEC_MAX_NGRAM || max_seq_len < 1 || history_stride < max_seq_len ||
      max_new_tokens < 1 || predicted_cols < 0 || (predicted && predicted_stride < predicted_cols))
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!history || !hist_len || !emitted || !finished || !ids || !positions || !q_len || !ctx_len) return LL_ERR_ARG;
  spec_draft_kernel<<<dim3((unsigned)batch), kThreads, 0, (hipStream_t)stream>>>(
      history, history_stride, hist_len, emitted, finished, max_tokens, max_new_tokens, max_seq_len, num_draft_tokens,
      max_ngram, min_ngram, use_ngram, predicted, predicted_stride, predicted_cols, predicted_lens, ids, positions, q_len,
      ctx_len);
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_spec_accept(const int64_t* argmax, const int64_t* ids, const int32_t* q_len, int64_t* out,
                              int64_t out_stride, int64_t out_cols, int32_t* history, int64_t history_stride,
                              int history_cols, int32_t* hist_len, int32_t* emitted, int32_t* finished, int32_t* lengths,
                              int32_t* reasons, const int32_t* max_tokens, int max_new_tokens, const int64_t* stop_ids,
                              int n_stop_ids, int32_t* verify_steps, int32_t* drafted, int32_t* accepted,
                              int32_t* accepted_per_step, int64_t per_step_stride, int per_step_cols, int32_t* step,
                              int32_t* running, int64_t batch, int num_draft_tokens, void* stream) {
  if (batch < 0 || batch > INT32_MAX || num_draft_tokens < 1 || num_draft_tokens > LL_SPEC_MAX_DRAFT || out_cols < 2 ||
      out_stride < out_cols || history_cols < 1 || history_stride < history_cols || max_new_tokens < 1 || n_stop_ids < 0 ||
      n_stop_ids > LL_STOP_MAX_IDS || per_step_cols < 0 || per_step_stride < per_step_cols)
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!argmax || !ids || !q_len || !out || !history || !hist_len || !emitted || !finished || !lengths || !reasons ||
      !verify_steps || !drafted || !accepted || !accepted_per_step || !step || !running || (n_stop_ids && !stop_ids))
    return LL_ERR_ARG;
  spec_accept_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(
      argmax, ids, q_len, out, out_stride, out_cols, history, history_stride, history_cols, hist_len, emitted, finished,
      lengths, reasons, max_tokens, max_new_tokens, stop_ids, n_stop_ids, verify_steps, drafted, accepted,
      accepted_per_step, per_step_stride, per_step_cols, step, running, (int)batch, num_draft_tokens);
  return LL_LAUNCH_CHECK();
}
