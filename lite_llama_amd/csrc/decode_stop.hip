// Per-row stopping inside the decode step (executor extension; the reference's loop is "greedy, no EOS stop, lockstep
// batch", engine/llm_engine.py:137-213).  One launch does what ll_decode_advance does (csrc/kv_ops.hip) and also takes the
// stop decision, so a captured step needs no host round trip per token:
//   tok = finished[i] ? pad : next[i];  out[i, step] = tok;  input_ids[i] = tok
//   a running row finishes when tok (1) is a stop id, (2) completes a stop sequence as the tail of out[i, 0 .. step],
//   (3) brings the count of returned tokens (= step: column 0 is the prefill's token) to max_tokens[i]; the lowest number
//   is the reason; lengths[i] = step either way (the finishing token is kept and counted)
//   rows still running afterwards: positions += 1, b_seq_len += 1, table[req, b_seq_len - 1] = cur_select_index (bump form)
//   bump form: cur_select_index[i] += batch for EVERY row -- a finished row keeps writing its K/V into the rows reserved
//   for it, which its table row never names; paged form (cur_select_index == nullptr): the table and the rows are left to
//   the pool's append, which pops nothing for an unchanged length, and ll_decode_stop_redirect points finished rows at the
//   junk block afterwards
//   running[0] = rows still running;  step += 1
// A finished row is frozen: it emits and is fed the pad, advances nothing and cannot finish again.  The row that finishes
// at this step does not advance either: its context ends with the token it was fed, whose K/V is the last it wrote.
// Single workgroup, rows strided over the threads (any batch); the running count is reduced in LDS and written once.
#include "common.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void decode_stop_advance_kernel(
    int64_t* __restrict__ out, int64_t out_stride, int64_t out_cols, int64_t* __restrict__ step,
    const int64_t* __restrict__ next, int64_t* __restrict__ input_ids, int64_t* __restrict__ positions,
    int32_t* __restrict__ cur_select, int32_t* __restrict__ b_seq_len, const int32_t* __restrict__ b_req_idx,
    int32_t* __restrict__ table, int64_t t_sb, int64_t t_ss, int64_t t_cols, const int64_t* __restrict__ stop_ids,
    int n_ids, const int64_t* __restrict__ stop_seqs, const int32_t* __restrict__ seq_lens, int n_seqs,
    const int32_t* __restrict__ max_tokens, int64_t pad, int32_t* __restrict__ finished, int32_t* __restrict__ lengths,
    int32_t* __restrict__ reasons, int32_t* __restrict__ running, int batch) {
  __shared__ int64_t s_ids[LL_STOP_MAX_IDS];
  __shared__ int64_t s_seqs[LL_STOP_MAX_SEQS * LL_STOP_MAX_SEQ_LEN];
  __shared__ int s_lens[LL_STOP_MAX_SEQS];
  __shared__ int s_count[kThreads / LL_WAVE];
  const int tid = threadIdx.x;
  const int64_t st = *step;
  if (st < 1 || st >= out_cols) return;  // no column left to write (uniform: nothing moves, the step counter included)
  if (tid < n_ids) s_ids[tid] = stop_ids[tid];
  if (tid < n_seqs * LL_STOP_MAX_SEQ_LEN) s_seqs[tid] = stop_seqs[tid];
  if (tid < n_seqs) s_lens[tid] = seq_lens[tid];
  __syncthreads();
  int live = 0;
  for (int i = tid; i < batch; i += kThreads) {
    const bool was_done = finished[i] != 0;
    const int64_t tok = was_done ? pad : next[i];
    int64_t* row = out + (int64_t)i * out_stride;
    row[st] = tok;
    input_ids[i] = tok;
    bool done = was_done;
    if (!was_done) {
      int reason = 0;
      for (int j = 0; j < n_ids; ++j)
        if (s_ids[j] == tok) reason = 1;
      if (!reason) {
        for (int q = 0; q < n_seqs && !reason; ++q) {
          const int n = s_lens[q];
          if (n < 1 || n > LL_STOP_MAX_SEQ_LEN || n > st + 1 || s_seqs[q * LL_STOP_MAX_SEQ_LEN + n - 1] != tok) continue;  // never left of column 0
          bool hit = true;
          for (int j = 0; j < n - 1 && hit; ++j) hit = row[st - (n - 1) + j] == s_seqs[q * LL_STOP_MAX_SEQ_LEN + j];
          if (hit) reason = 2;
        }
      }
      if (!reason && max_tokens && st >= max_tokens[i]) reason = 3;
      lengths[i] = (int32_t)st;
      if (reason) {
        finished[i] = 1;
        reasons[i] = reason;
        done = true;
      }
    }
    if (cur_select) cur_select[i] += batch;
    if (!done) {
      ++live;
      positions[i] += 1;
      const int32_t len = b_seq_len[i] + 1;
      b_seq_len[i] = len;
      if (cur_select && len - 1 < t_cols) table[(int64_t)b_req_idx[i] * t_sb + (int64_t)(len - 1) * t_ss] = cur_select[i];
    }
  }
  // rows still running: wave sums, then the four of them through LDS; one ordinary store
#pragma unroll
  for (int off = LL_WAVE / 2; off > 0; off >>= 1) live += __shfl_down(live, off, LL_WAVE);
  if ((tid & (LL_WAVE - 1)) == 0) s_count[tid / LL_WAVE] = live;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / LL_WAVE; ++w) total += s_count[w];
    running[0] = total;
    *step = st + 1;
  }
}

// Paged pool, after the step's append: a finished row's length did not move, so the append named the row of its LAST real
// position again; its (pad) K/V of this step goes to the junk block instead, like every pad's.
__global__ __launch_bounds__(kThreads) void decode_stop_redirect_kernel(int32_t* __restrict__ cur_select,
                                                                        const int32_t* __restrict__ finished,
                                                                        int32_t junk_row, int block_size, int batch) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < batch && finished[i]) cur_select[i] = junk_row + i % block_size;
}

}  // namespace

extern "C" int ll_decode_stop_advance(int64_t* out, int64_t out_stride, int64_t out_cols, int64_t* step,
                                      const int64_t* next_tokens, int64_t* input_ids, int64_t* positions,
                                      int32_t* cur_select_index, int32_t* b_seq_len, const int32_t* b_req_idx,
                                      int32_t* table, int64_t table_stride_b, int64_t table_stride_s, int64_t table_cols,
                                      const int64_t* stop_ids, int n_stop_ids, const int64_t* stop_seqs,
                                      const int32_t* stop_seq_lens, int n_stop_seqs, const int32_t* max_tokens,
                                      int64_t pad_token, int32_t* finished, int32_t* lengths, int32_t* reasons,
                                      int32_t* running, int batch, void* stream) {
  if (batch < 0 || out_cols < 2 || out_stride < out_cols || n_stop_ids < 0 || n_stop_ids > LL_STOP_MAX_IDS ||
      n_stop_seqs < 0 || n_stop_seqs > LL_STOP_MAX_SEQS)
    return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!out || !step || !next_tokens || !input_ids || !positions || !b_seq_len || !finished || !lengths || !reasons ||
      !running || (n_stop_ids && !stop_ids) || (n_stop_seqs && (!stop_seqs || !stop_seq_lens)))
    return LL_ERR_ARG;
  if (cur_select_index && (!b_req_idx || !table || table_cols < 1)) return LL_ERR_ARG;
  decode_stop_advance_kernel<<<dim3(1), kThreads, 0, (hipStream_t)stream>>>(
      out, out_stride, out_cols, step, next_tokens, input_ids, positions, cur_select_index, b_seq_len, b_req_idx, table,
      table_stride_b, table_stride_s, table_cols, stop_ids, n_stop_ids, stop_seqs, stop_seq_lens, n_stop_seqs, max_tokens,
      pad_token, finished, lengths, reasons, running, batch);
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_decode_stop_redirect(int32_t* cur_select_index, const int32_t* finished, int64_t junk_row,
                                       int block_size, int batch, void* stream) {
  if (batch < 0 || block_size < 1 || junk_row < 0 || junk_row + block_size > INT32_MAX) return LL_ERR_SHAPE;
  if (batch == 0) return LL_OK;
  if (!cur_select_index || !finished) return LL_ERR_ARG;
  decode_stop_redirect_kernel<<<dim3((unsigned)((batch + kThreads - 1) / kThreads)), kThreads, 0, (hipStream_t)stream>>>(
      cur_select_index, finished, (int32_t)junk_row, block_size, batch);
  return LL_LAUNCH_CHECK();
}
