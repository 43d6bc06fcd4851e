// Host-side hooks one attention file calls in another's (not exported through include/lite_llama_amd.h).  Shapes, dtypes and
// pointers reaching a launcher have been validated by its caller.
#pragma once
#include <stdint.h>

// flash_decoding's stage 1 alone, in the two-launch form (flash_decoding.hip): plain fp32 records mid_o [batch, hq, nparts, d]
// (normalised) and mid_lse [batch, hq, nparts] with nparts = ll_flash_decoding_num_partitions(max_len); partitions at or past
// b_seq_len[b] store nothing.  No merge is launched.  d in {32, 64, 128, 256}, dtype LL_F16 / LL_BF16.
int fd_stage1_records(const void* q, const void* k_cache, const void* v_cache, const int32_t* table, const void* b_req_idx,
                      const void* b_seq_len, float* mid_o, float* mid_lse, int batch, int hq, int hkv, int d, int64_t max_len,
                      float qk_scale, int64_t q_stride_b, int64_t q_stride_h, int64_t k_stride_t, int64_t k_stride_h,
                      int64_t v_stride_t, int64_t v_stride_h, int64_t table_stride_b, int dtype, int req_width, int seq_width,
                      void* stream);
