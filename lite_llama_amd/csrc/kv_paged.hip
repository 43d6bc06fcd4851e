// Block-granular KV paging on the device (second half).  The reference's pool is token-granular and
// carries the TODO "reshape into [blocks, block_size, ...] to support PagedAttention"
// (lite_llama/executor/kv_cache_manager.py:211); its kernels read a PER-TOKEN table
// (b_req_tokens_table[req][pos] -> pool row, executor/model_runner.py:153-218).  Here the pool is handed out in blocks
// of ``block_size`` consecutive rows -- a request holds ceil(len / block_size) blocks, listed in a block table -- and the
// per-token table the kernels consume is DERIVED from it on the device (row = block * block_size + pos % block_size):
// the attention / KV-write kernels and their results are unchanged, allocation work drops by block_size x, a
// request's rows are contiguous in runs of block_size, and nothing is read back by the host (the free blocks live in a
// device stack; admission, the per-step append and release are stream-ordered launches that can sit inside the
// captured decode step).
//
// State (all int32, device):  free_stack[num_blocks - 1] block ids, state[0] = number of free blocks (the stack
// top), state[1] = error flags (1: out of blocks, 2: a request outgrew its block-table row); block_table
// [max_reqs][bt_stride]; req_blocks[max_reqs] = blocks held.  Block num_blocks - 1 is never handed out: it is the
// JUNK block, the rows that padded prefill positions and refused requests write to (the kernels always get valid
// rows).  Pops come off the top in request order (an exclusive scan over the batch), so the outcome is deterministic:
// a fresh pool hands out blocks 0, 1, 2, ...
//
// Shared blocks (opt-in: ll_kv_paged_fork / ll_kv_paged_release_shared).  block_share[num_blocks] = holders of a block
// minus one (0 for a free block and for a block with one holder).  A fork lets a new request name another request's
// FULL blocks (share count + 1 each) and gives it a private copy of the partial last block, so no shared block is ever
// written: every writer (append, extend_at, the source itself) writes at positions at or beyond its own length, which
// lie in its own blocks -- the entries above and every attention / KV-write kernel stay as they are.  A release gives
// a block back only when its last holder lets go.  Error bit 4: a fork that breaks its contract.  share_scratch
// [2 * num_blocks + 2], zero at rest: per block the holders a release call lists and the largest caller index + 1 among
// them; then the fork's "accepted" flag and the ticket counter of its copy launch.
#include "common.h"

namespace {

constexpr int kMaxBatch = 1024;  // one workgroup scans the batch

// exclusive scan of one int per thread over a 1024-thread workgroup (lds: 16 wave sums + 64 scanned); returns
// (exclusive prefix, total)
__device__ __forceinline__ void block_scan(int v, int* lds, int& prefix, int& total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  if (wave == 0) {
    int w = lane < (int)(blockDim.x >> 6) ? lds[lane] : 0;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const int y = __shfl_up(w, off, 64);
      if (lane >= off) w += y;
    }
    lds[16 + lane] = w;  // inclusive wave totals
  }
  __syncthreads();
  const int before = wave == 0 ? 0 : lds[16 + wave - 1];
  prefix = before + x - v;
  total = lds[16 + (blockDim.x >> 6) - 1];
  __syncthreads();
}

__global__ void paged_reset_kernel(int32_t* free_stack, int32_t* state, int32_t* req_blocks, int64_t num_blocks,
                                   int64_t max_reqs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t usable = num_blocks - 1;
  if (i < usable) free_stack[i] = (int32_t)(usable - 1 - i);  // top of the stack = block 0
  if (i < max_reqs) req_blocks[i] = 0;
  if (i == 0) {
    state[0] = (int32_t)usable;
    state[1] = 0;
  }
}

// Make request req_idx[i] hold ceil(want_len[i] / block_size) blocks (never shrinks).  All-or-nothing per call: if the
// stack is short nothing is popped and error bit 1 is set.
__global__ __launch_bounds__(kMaxBatch) void paged_reserve_kernel(
    const int32_t* __restrict__ free_stack, int32_t* __restrict__ state, int32_t* __restrict__ block_table,
    int64_t bt_stride, int32_t* __restrict__ req_blocks, const int32_t* __restrict__ req_idx,
    const int32_t* __restrict__ want_len, int len_bias, int n, int block_size, int max_blocks,
    const int32_t* __restrict__ base = nullptr) {
  __shared__ int lds[96];
  const int i = threadIdx.x;
  int req = 0, held = 0, need = 0;
  bool overflow = false;
  if (i < n) {
    req = req_idx[i];
    held = req_blocks[req];
    const int len = want_len[i] + len_bias + (base ? base[i] : 0);
    int want = len > 0 ? (len + block_size - 1) / block_size : 0;
    if (want > max_blocks) {
      want = max_blocks;
      overflow = true;
    }
    need = want > held ? want - held : 0;
  }
  int prefix, total;
  block_scan(need, lds, prefix, total);
  const int top = state[0];
  __syncthreads();  // everyone has read the top before it moves
  if (total > top) {
    if (i == 0) atomicOr(&state[1], 1);
    return;
  }
  if (overflow) atomicOr(&state[1], 2);
  for (int j = 0; j < need; ++j) block_table[(int64_t)req * bt_stride + held + j] = free_stack[top - 1 - prefix - j];
  if (need > 0) req_blocks[req] = held + need;
  if (i == 0) state[0] = top - total;
}

// Caller contract (not checked on the device: the entry points carry no request-table size): request indices are inside
// the tables and no request is listed twice in one call.
// Rows of positions [p_lo, p_hi) of every request on a [n][grid_len] grid: token_table[req][p] = row and
// select_out[i * grid_len + (p - p_base)] = row; positions the request holds no block for (pads, refused requests)
// get junk-block rows in select_out and leave the token table alone.  base (extend_at): the grid holds positions
// base[i] .. base[i] + grid_len - 1 of request i, of which the first lens[i] are valid (a chunk that starts at base[i]).
__global__ void paged_rows_kernel(const int32_t* __restrict__ block_table, int64_t bt_stride,
                                  const int32_t* __restrict__ req_blocks, const int32_t* __restrict__ req_idx,
                                  const int32_t* __restrict__ lens, int len_bias, int n, int block_size, int grid_len,
                                  int from_end, int32_t* __restrict__ token_table, int64_t tt_stride,
                                  int32_t* __restrict__ select_out, int64_t num_blocks, int32_t* __restrict__ state,
                                  const int32_t* __restrict__ base = nullptr) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * grid_len) return;
  const int i = (int)(idx / grid_len), g = (int)(idx - (int64_t)i * grid_len);
  const int req = req_idx[i];
  const int len = lens[i] + len_bias + (base ? base[i] : 0);
  // from_end: the grid holds the LAST grid_len positions of the request (the decode step: grid_len = 1 -> position len - 1)
  const int p = base ? base[i] + g : from_end ? len - grid_len + g : g;
  const int64_t junk = (num_blocks - 1) * block_size + (p >= 0 ? p % block_size : 0);
  int64_t row = junk;
  if (p >= 0 && p < len && p >= tt_stride) {
    atomicOr(&state[1], 2);  // beyond the request's token-table row (max_seq_len not a multiple of block_size): junk row, flagged
  } else if (p >= 0 && p < len) {
    const int b = p / block_size;
    if (b < req_blocks[req]) {
      row = (int64_t)block_table[(int64_t)req * bt_stride + b] * block_size + p % block_size;
      token_table[(int64_t)req * tt_stride + p] = (int32_t)row;
    }
  }
  select_out[idx] = (int32_t)row;
}

// Return every block of the listed requests to the stack (request order, block order); req_blocks -> 0.
__global__ __launch_bounds__(kMaxBatch) void paged_release_kernel(int32_t* __restrict__ free_stack, int32_t* __restrict__ state,
                                                                  const int32_t* __restrict__ block_table, int64_t bt_stride,
                                                                  int32_t* __restrict__ req_blocks,
                                                                  const int32_t* __restrict__ req_idx, int n) {
  __shared__ int lds[96];
  const int i = threadIdx.x;
  int req = 0, held = 0;
  if (i < n) {
    req = req_idx[i];
    held = req_blocks[req];
  }
  int prefix, total;
  block_scan(held, lds, prefix, total);
  const int top = state[0];
  __syncthreads();
  for (int j = 0; j < held; ++j) free_stack[top + prefix + j] = block_table[(int64_t)req * bt_stride + j];
  if (i < n) req_blocks[req] = 0;
  if (i == 0) state[0] = top + total;
}

// A value another thread of the workgroup (or an earlier launch) wrote with an atomic or a plain store: read at the L2.
__device__ __forceinline__ int load_l2(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Fork i: request dst[i] names the first lens[i] / block_size blocks of src[i] (share + 1) and gets a fresh block for
// the lens[i] % block_size rows after them (pops in call order, like paged_reserve_kernel).  All-or-nothing per call:
// bit 4 for a dst that holds blocks, a length < 1 or beyond src's blocks / the token-table row; bit 1 when the stack is
// short; so is a dst listed twice or a dst that is a source of the same call (bit 4).  An accepted call sets ctrl[0] for
// the launch that follows (the partial blocks' rows, the token table); a refused one writes it 0.
__global__ __launch_bounds__(kMaxBatch) void paged_fork_kernel(
    const int32_t* __restrict__ free_stack, int32_t* __restrict__ state, int32_t* __restrict__ block_table,
    int64_t bt_stride, int32_t* __restrict__ req_blocks, int32_t* __restrict__ block_share, int32_t* __restrict__ ctrl,
    const int32_t* __restrict__ src_req, const int32_t* __restrict__ dst_req, const int32_t* __restrict__ lens, int n,
    int block_size, int64_t tt_stride) {
  __shared__ int lds[96];
  __shared__ int s_src[kMaxBatch], s_dst[kMaxBatch], s_full[kMaxBatch];
  const int i = threadIdx.x;
  int src = 0, dst = 0, full = 0, need = 0;
  bool bad = false, claimed = false;
  if (i < n) {
    src = src_req[i];
    dst = dst_req[i];
    const int len = lens[i];
    full = len / block_size;
    need = len % block_size ? 1 : 0;
    // a dst that holds nothing is claimed (req_blocks 0 -> -1): a dst listed twice loses the second claim, and a source
    // that is a dst of this call reads -1 blocks below -- both are refused instead of leaking a block
    claimed = atomicCAS(&req_blocks[dst], 0, -1) == 0;
    bad = !claimed || len < 1 || len > tt_stride;
  }
  __syncthreads();
  if (i < n && !bad) bad = full + need > load_l2(&req_blocks[src]);
  if (__syncthreads_or(bad)) {
    if (claimed) req_blocks[dst] = 0;
    if (i == 0) {
      atomicOr(&state[1], 4);
      ctrl[0] = 0;  // were an earlier second launch lost before it cleared the word, this call's must still do nothing
    }
    return;
  }
  int prefix, total;
  block_scan(need, lds, prefix, total);
  const int top = state[0];
  __syncthreads();  // everyone has read the top before it moves
  if (total > top) {
    if (claimed) req_blocks[dst] = 0;
    if (i == 0) {
      atomicOr(&state[1], 1);
      ctrl[0] = 0;
    }
    return;
  }
  if (i < n) {
    s_src[i] = src;
    s_dst[i] = dst;
    s_full[i] = full;
    if (need) block_table[(int64_t)dst * bt_stride + full] = free_stack[top - 1 - prefix];
    req_blocks[dst] = full + need;
  }
  if (i == 0) {
    state[0] = top - total;
    ctrl[0] = 1;
  }
  __syncthreads();
  // the shared blocks, all threads over (fork, block): no dst is a source of this call, so the rows read here are those
  // of earlier launches; the same source may be forked many times, so the count moves by atomics
  const int64_t work = (int64_t)n * bt_stride;
  for (int64_t w = i; w < work; w += kMaxBatch) {
    const int f = (int)(w / bt_stride), j = (int)(w - (int64_t)f * bt_stride);
    if (j >= s_full[f]) continue;
    const int b = block_table[(int64_t)s_src[f] * bt_stride + j];
    block_table[(int64_t)s_dst[f] * bt_stride + j] = b;
    atomicAdd(&block_share[b], 1);
  }
}

// What follows an accepted fork, grid (fork, layer, piece).  Every layer: rows [0, lens % block_size) of the source's
// partial block into the block the launch above popped, as one contiguous run of 16-byte words.  Layer 0 also fills
// token_table[dst][p] for p < lens from the block-table row the launch above wrote.  ctrl[0] = 0 (the call was
// refused): nothing is read or written.  The last workgroup to finish (ticket in ctrl[1]) puts ctrl back to 0.
__global__ __launch_bounds__(256) void paged_fork_copy_kernel(
    const int32_t* __restrict__ block_table, int64_t bt_stride, int32_t* __restrict__ ctrl,
    const int32_t* __restrict__ src_req, const int32_t* __restrict__ dst_req, const int32_t* __restrict__ lens,
    int block_size, int32_t* __restrict__ token_table, int64_t tt_stride, void* const* __restrict__ layer_base,
    int64_t row_bytes, int64_t piece_bytes, int64_t num_blocks) {
  __shared__ int accepted;
  if (threadIdx.x == 0) accepted = load_l2(&ctrl[0]);
  __syncthreads();
  if (!accepted) return;
  const int f = blockIdx.x;
  const int len = lens[f];
  const int full = len / block_size, rem = len % block_size;
  const int32_t* bt = block_table + (int64_t)dst_req[f] * bt_stride;
  if (blockIdx.y == 0) {
    int32_t* tt = token_table + (int64_t)dst_req[f] * tt_stride;  // len <= tt_stride: checked by the launch above
    for (int p = blockIdx.z * blockDim.x + threadIdx.x; p < len; p += gridDim.z * blockDim.x)
      tt[p] = bt[p / block_size] * block_size + p % block_size;
  }
  if (rem) {
    const int64_t sb = block_table[(int64_t)src_req[f] * bt_stride + full];
    const int64_t db = bt[full];
    if (sb >= 0 && sb < num_blocks && db >= 0 && db < num_blocks - 1) {  // never the junk block, never outside the pool
      const int64_t bytes = rem * row_bytes;
      const int64_t lo = (int64_t)blockIdx.z * piece_bytes;
      const int64_t hi = lo + piece_bytes < bytes ? lo + piece_bytes : bytes;
      char* base = (char*)layer_base[blockIdx.y];
      const uint4* from = (const uint4*)(base + sb * block_size * row_bytes);
      uint4* to = (uint4*)(base + db * block_size * row_bytes);
      for (int64_t w = lo / 16 + threadIdx.x; w < hi / 16; w += blockDim.x) to[w] = from[w];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int all = (int)(gridDim.x * gridDim.y * gridDim.z);
    if (atomicAdd(&ctrl[1], 1) == all - 1) {  // every other workgroup has read ctrl[0] before it took its ticket
      __hip_atomic_store(&ctrl[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&ctrl[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// paged_release_kernel with share counts: a block goes back on the stack only when its last holder lets go.  The result
// is that of releasing the requests one after the other in call order: a block several listed requests hold is pushed
// by the last of them, at its place in the scan.  Pass 1 counts the call's holders per block and records the largest
// caller index + 1; after the barrier only that caller acts on the block -- it pushes it (holders == share + 1) or takes
// the call's holders off the share count -- and puts the scratch back to zero.
__global__ __launch_bounds__(kMaxBatch) void paged_release_shared_kernel(
    int32_t* __restrict__ free_stack, int32_t* __restrict__ state, const int32_t* __restrict__ block_table,
    int64_t bt_stride, int32_t* __restrict__ req_blocks, int32_t* __restrict__ block_share, int32_t* __restrict__ holders,
    int32_t* __restrict__ last_caller, const int32_t* __restrict__ req_idx, int n, int64_t num_blocks) {
  __shared__ int lds[96];
  const int i = threadIdx.x;
  int req = 0, held = 0;
  if (i < n) {
    req = req_idx[i];
    held = req_blocks[req];
  }
  const int32_t* mine = block_table + (int64_t)req * bt_stride;
  for (int j = 0; j < held; ++j) {
    const int b = mine[j];
    atomicAdd(&holders[b], 1);
    atomicMax(&last_caller[b], i + 1);
  }
  __syncthreads();
  int pushes = 0;
  for (int j = 0; j < held; ++j) {
    const int b = mine[j];
    if (load_l2(&last_caller[b]) == i + 1 && load_l2(&holders[b]) == load_l2(&block_share[b]) + 1) ++pushes;
  }
  int prefix, total;
  block_scan(pushes, lds, prefix, total);  // ends on a barrier: every thread has counted before a share count moves
  const int top = state[0];
  __syncthreads();
  int at = top + prefix;
  for (int j = 0; j < held; ++j) {
    const int b = mine[j];
    if (load_l2(&last_caller[b]) != i + 1) continue;  // only this thread writes the three words of b from here on
    const int c = load_l2(&holders[b]), s = load_l2(&block_share[b]);
    if (c == s + 1) {
      if (at < num_blocks - 1) free_stack[at] = b;
      ++at;
      block_share[b] = 0;
    } else {
      block_share[b] = s - c;
    }
    holders[b] = 0;
    last_caller[b] = 0;
  }
  if (i < n) req_blocks[req] = 0;
  if (i == 0) state[0] = top + total;
}

}  // namespace

extern "C" int ll_kv_paged_reset(int32_t* free_stack, int32_t* state, int32_t* req_blocks, int64_t num_blocks,
                                 int64_t max_reqs, void* stream) {
  if (num_blocks < 2 || max_reqs < 1) return LL_ERR_SHAPE;
  if (!free_stack || !state || !req_blocks) return LL_ERR_ARG;
  const int64_t n = num_blocks > max_reqs ? num_blocks : max_reqs;
  paged_reset_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream>>>(free_stack, state, req_blocks,
                                                                                        num_blocks, max_reqs);
  return LL_LAUNCH_CHECK();
}

// lens + len_bias = the length every request must be able to hold after the call; rows are produced for the grid
// [n][grid_len]: from_end = 0 -> positions 0 .. grid_len - 1 (prefill, pads included), from_end = 1 -> the last
// grid_len positions (decode append: grid_len = 1).
extern "C" int ll_kv_paged_extend(int32_t* free_stack, int32_t* state, int32_t* block_table, int64_t bt_stride,
                                  int32_t* req_blocks, const int32_t* req_idx, const int32_t* lens, int len_bias,
                                  int64_t n, int block_size, int64_t grid_len, int from_end, int32_t* token_table,
                                  int64_t tt_stride, int32_t* select_out, int64_t num_blocks, void* stream) {
  if (n < 0 || n > kMaxBatch || block_size < 1 || grid_len < 1 || num_blocks < 2 || bt_stride < 1) return LL_ERR_SHAPE;
  if (n == 0) return LL_OK;
  if (!free_stack || !state || !block_table || !req_blocks || !req_idx || !lens || !token_table || !select_out)
    return LL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  paged_reserve_kernel<<<1, kMaxBatch, 0, st>>>(free_stack, state, block_table, bt_stride, req_blocks, req_idx, lens,
                                               len_bias, (int)n, block_size, (int)bt_stride);
  const int64_t total = n * grid_len;
  paged_rows_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      block_table, bt_stride, req_blocks, req_idx, lens, len_bias, (int)n, block_size, (int)grid_len, from_end,
      token_table, tt_stride, select_out, num_blocks, state);
  return LL_LAUNCH_CHECK();
}

// extend_at: request i's grid holds positions ctx_lens[i] .. ctx_lens[i] + grid_len - 1, of which the first
// chunk_lens[i] are valid; blocks are popped up to ctx_lens[i] + chunk_lens[i] only and pads get junk rows (a chunked
// prefill: from_end = 1 with a ragged grid would name the request's own prefix rows for a short chunk's pads).
extern "C" int ll_kv_paged_extend_at(int32_t* free_stack, int32_t* state, int32_t* block_table, int64_t bt_stride,
                                     int32_t* req_blocks, const int32_t* req_idx, const int32_t* ctx_lens,
                                     const int32_t* chunk_lens, int64_t n, int block_size, int64_t grid_len,
                                     int32_t* token_table, int64_t tt_stride, int32_t* select_out, int64_t num_blocks,
                                     void* stream) {
  if (n < 0 || n > kMaxBatch || block_size < 1 || grid_len < 1 || num_blocks < 2 || bt_stride < 1) return LL_ERR_SHAPE;
  if (n == 0) return LL_OK;
  if (!free_stack || !state || !block_table || !req_blocks || !req_idx || !ctx_lens || !chunk_lens || !token_table ||
      !select_out)
    return LL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  paged_reserve_kernel<<<1, kMaxBatch, 0, st>>>(free_stack, state, block_table, bt_stride, req_blocks, req_idx,
                                               chunk_lens, 0, (int)n, block_size, (int)bt_stride, ctx_lens);
  const int64_t total = n * grid_len;
  paged_rows_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      block_table, bt_stride, req_blocks, req_idx, chunk_lens, 0, (int)n, block_size, (int)grid_len, 0, token_table,
      tt_stride, select_out, num_blocks, state, ctx_lens);
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_kv_paged_release(int32_t* free_stack, int32_t* state, const int32_t* block_table, int64_t bt_stride,
                                   int32_t* req_blocks, const int32_t* req_idx, int64_t n, void* stream) {
  if (n < 0 || n > kMaxBatch || bt_stride < 1) return LL_ERR_SHAPE;
  if (n == 0) return LL_OK;
  if (!free_stack || !state || !block_table || !req_blocks || !req_idx) return LL_ERR_ARG;
  paged_release_kernel<<<1, kMaxBatch, 0, (hipStream_t)stream>>>(free_stack, state, block_table, bt_stride, req_blocks,
                                                                req_idx, (int)n);
  return LL_LAUNCH_CHECK();
}

// Fork: see paged_fork_kernel (tables, counts) / paged_fork_copy_kernel (partial blocks, token table).  layer_base: device array of num_layers pool base pointers;
// row_bytes: bytes of one pool row (all K and V heads), a multiple of 16.
extern "C" int ll_kv_paged_fork(const int32_t* free_stack, int32_t* state, int32_t* block_table, int64_t bt_stride,
                                int32_t* req_blocks, int32_t* block_share, int32_t* share_scratch, const int32_t* src_req,
                                const int32_t* dst_req, const int32_t* lens, int64_t n, int block_size,
                                int32_t* token_table, int64_t tt_stride, void* const* layer_base, int64_t num_layers,
                                int64_t row_bytes, int64_t num_blocks, void* stream) {
  if (n < 0 || n > kMaxBatch || block_size < 1 || num_blocks < 2 || bt_stride < 1 || tt_stride < 1 || num_layers < 1 ||
      num_layers > 65535 || row_bytes < 16 || row_bytes % 16)
    return LL_ERR_SHAPE;
  if (n == 0) return LL_OK;
  if (!free_stack || !state || !block_table || !req_blocks || !block_share || !share_scratch || !src_req || !dst_req ||
      !lens || !token_table || !layer_base)
    return LL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int32_t* ctrl = share_scratch + 2 * num_blocks;
  paged_fork_kernel<<<1, kMaxBatch, 0, st>>>(free_stack, state, block_table, bt_stride, req_blocks, block_share, ctrl,
                                            src_req, dst_req, lens, (int)n, block_size, tt_stride);
  // at most block_size - 1 rows per (fork, layer); pieces of >= 16 KB, at most 64 of them
  const int64_t most = (int64_t)block_size * row_bytes;
  int64_t piece = 16384;
  while ((most + piece - 1) / piece > 64) piece *= 2;
  const unsigned pieces = (unsigned)((most + piece - 1) / piece);
  paged_fork_copy_kernel<<<dim3((unsigned)n, (unsigned)num_layers, pieces), 256, 0, st>>>(
      block_table, bt_stride, ctrl, src_req, dst_req, lens, block_size, token_table, tt_stride, layer_base, row_bytes,
      piece, num_blocks);
  return LL_LAUNCH_CHECK();
}

extern "C" int ll_kv_paged_release_shared(int32_t* free_stack, int32_t* state, const int32_t* block_table,
                                          int64_t bt_stride, int32_t* req_blocks, int32_t* block_share,
                                          int32_t* share_scratch, const int32_t* req_idx, int64_t n, int64_t num_blocks,
                                          void* stream) {
  if (n < 0 || n > kMaxBatch || bt_stride < 1 || num_blocks < 2) return LL_ERR_SHAPE;
  if (n == 0) return LL_OK;
  if (!free_stack || !state || !block_table || !req_blocks || !block_share || !share_scratch || !req_idx) return LL_ERR_ARG;
  paged_release_shared_kernel<<<1, kMaxBatch, 0, (hipStream_t)stream>>>(
      free_stack, state, block_table, bt_stride, req_blocks, block_share, share_scratch, share_scratch + num_blocks,
      req_idx, (int)n, num_blocks);
  return LL_LAUNCH_CHECK();
}
