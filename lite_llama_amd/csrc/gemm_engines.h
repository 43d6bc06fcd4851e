// Host-side hooks one GEMM engine's file calls in another's (not exported through include/lite_llama_amd.h).  Shapes and pointers
// reaching a *_launch have been validated by its caller.
#pragma once
#include <stdint.h>

// ---- W4A16 decode (pre-packed layout) ----
// Which engine serves a launch of a supported shape (gemm_w4_dispatch.hip).
enum W4Engine { W4_SHORT_PARTIALS, W4_ROW_GROUPS, W4_SHORT_FULL, W4_UNIT_LOOP };
W4Engine w4a16_engine(int64_t m, int64_t n, int64_t k, int group_size, int epilogue);

// the unit loop (gemm_w4_v3.hip): stream-K over the tiles, or a split-K partial launch
bool v3_shape_ok(int64_t m, int64_t n, int64_t k);
int v3_partials_count(int64_t m, int64_t n, int64_t k, int group_size);  // planes of a partial launch; 0: not served
int v3_launch(void* out, const void* x, const void* wpacked, const void* spacked, const void* bias, int64_t m, int64_t n, int64_t k,
              int group_size, int64_t x_stride_m, float* workspace, int32_t* counters, int epilogue, void* stream);
extern "C" int ll_w4a16_v3_workspace(int64_t m, int64_t n, int64_t k, int64_t* floats, int64_t* ints);
// the row-group loop (gemm_w4_v4.hip); kslices = the k-split of a partial launch (= v3_partials_count)
int v4_wants(int64_t n, int epilogue);
int v4_launch(void* out, const void* x, const void* wpacked, const void* spacked, const void* bias, int64_t m, int64_t n, int64_t k,
              int group_size, int64_t x_stride_m, int epilogue, int kslices, void* stream);
// the short-stream engine's split-K partial launches of a few tens of KB per CU (gemm_short.hip)
int ss_partials_slices(int64_t m, int64_t n, int64_t k, int group_size);  // planes it leaves; 0: not its launch
int ss_launch(void* out, const void* x, const void* wpacked, const void* spacked, int64_t m, int64_t n, int64_t k, int group_size,
              int64_t x_stride_m, void* stream);
// ... and its all-of-K form for narrow finished outputs (gemm_short_full.hip)
int sf_wants(int64_t m, int64_t n, int64_t k, int group_size);
int sf_launch(void* out, const void* x, const void* wpacked, const void* spacked, const void* bias, int64_t m, int64_t n, int64_t k,
              int group_size, int64_t x_stride_m, int epilogue, void* stream);

// ---- 8- and 16-bit weights ----
// the decode-shaped engine (gemm_w8_skinny.hip): served shapes leave fp32 / int32 partial planes in the workspace
extern "C" int64_t ll_dense8_partial_words(int64_t m, int64_t n, int64_t k);
extern "C" int64_t ll_dense16_partial_words(int64_t m, int64_t n, int64_t k);
extern "C" int ll_dense8_try(void* out, const void* x, const void* w, const float* scales, const float* a_scale,
                             const void* bias, int32_t* acc_out, int64_t m, int64_t n, int64_t k, int group_n,
                             int64_t group_k, int wfmt, int64_t x_stride, int64_t w_stride, int64_t s_stride_n,
                             int64_t s_stride_k, void* partials, void* stream);
// ... and what ll_dense8_try asks of a call besides its pointers (ll_w8a16_engine asks too)
bool dense8_takes(int64_t m, int64_t n, int64_t k, int64_t group_k, int wfmt, int64_t x_stride, int64_t w_stride);
// its short-stream form (gemm_short_dense.hip)
int sd_partials_slices(int64_t m, int64_t n, int64_t k, int wfmt, int max_splits);
int sd_launch(float* out, const void* x, const void* w, const float* scales, int64_t m, int64_t n, int64_t k, int group_n,
              int64_t group_k, int wfmt, int64_t x_stride, int64_t w_stride_bytes, int64_t s_stride_n, int64_t s_stride_k,
              int max_splits, void* stream);
// the M-tiled prefill engine (gemm_w8_prefill.hip)
extern "C" int ll_w8_mtiled_try(void* out, const void* x, const void* w, const float* scales, const float* a_scale, const void* bias,
                                int32_t* acc_out, int64_t m, int64_t n, int64_t k, int group_n, int64_t group_k, int wfmt,
                                int64_t x_stride, int64_t w_stride, int64_t s_stride_n, int64_t s_stride_k, void* stream);
// ... and what it asks of a call besides its pointers (group_k already clamped to k; ll_w8a16_engine asks too)
bool w8_mtiled_takes(int64_t m, int64_t n, int64_t k, int64_t group_k, int wfmt, int64_t x_stride, int64_t w_stride);
