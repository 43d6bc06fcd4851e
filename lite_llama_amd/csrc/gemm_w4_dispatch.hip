// W4A16 decode GEMM on the pre-packed layout (ll_w4a16_pack_weights): the shapes it takes, the planes a split-K partial launch
// leaves, and which of the four engines serves a launch.  The engines share the layouts and write the same outputs / planes:
//   gemm_short.hip       short-stream engine, split-K partial launches of a few tens of KB per CU
//   gemm_w4_v4.hip       row-group loop, N split across the CUs
//   gemm_short_full.hip  short-stream engine's all-of-K form for narrow finished outputs
//   gemm_w4_v3.hip       unit loop (stream-K over the tiles): every supported shape
#include "common.h"
#include "gemm_engines.h"

extern "C" int ll_w4a16_prepacked_supported(int64_t m, int64_t n, int64_t k, int group_size) {
  if (group_size <= 0 || group_size % 128 != 0 || k % group_size != 0) return 0;
  const int gdiv = group_size / 128;
  return v3_shape_ok(m, n, k) && ((gdiv & (gdiv - 1)) == 0) ? 1 : 0;
}

// bits 8-9 of the epilogue: a forced unit-loop tile width (tests / tuning) -- the launch stays on the unit loop
static bool w4_unit_loop_forced(int epilogue) { return ((epilogue >> 8) & 3) != 0; }

W4Engine w4a16_engine(int64_t m, int64_t n, int64_t k, int group_size, int epilogue) {
  if (w4_unit_loop_forced(epilogue)) return W4_UNIT_LOOP;
  const bool partials = (epilogue & 3) == 2;
  // round 6: split-K partial launches whose stream is a few tens of KB per CU
  if (partials && ss_partials_slices(m, n, k, group_size) > 0) return W4_SHORT_PARTIALS;
  // round 5: the row-group loop when its plan serves the shape
  if (v4_wants(n, epilogue)) return W4_ROW_GROUPS;
  // narrow FINISHED outputs (the reference-shaped layer's q / k|v / o calls, the fused gate|up of a TP >= 4 shard): the sums meet
  // inside the workgroup, no slabs, no counters
  if (!partials && sf_wants(m, n, k, group_size)) return W4_SHORT_FULL;
  return W4_UNIT_LOOP;
}

// Split-K partial mode (epilogue 2): the number of fp32 planes [S][M][N] the launch writes; 0 when the shape has too many tiles for
// the tile-group split (use the ordinary epilogue then).  `epilogue` = the value the launch will be given: the short-stream
// engine's k-split differs from the unit loop's (which the row-group loop shares).
extern "C" int ll_w4a16_partials_count_ex(int64_t m, int64_t n, int64_t k, int group_size, int epilogue) {
  if (!ll_w4a16_prepacked_supported(m, n, k, group_size)) return 0;
  if (!w4_unit_loop_forced(epilogue)) {
    const int s = ss_partials_slices(m, n, k, group_size);
    if (s > 0) return s;
  }
  return v3_partials_count(m, n, k, group_size);
}
extern "C" int ll_w4a16_partials_count(int64_t m, int64_t n, int64_t k, int group_size) {
  return ll_w4a16_partials_count_ex(m, n, k, group_size, 2);
}

// Host-side introspection (tests; no device work, changes no launch): the W4Engine a launch of this shape and epilogue takes, -1 when
// ll_w4a16_matmul_prepacked would refuse it (shape outside the engines, or a split-K partial launch that leaves no planes).
extern "C" int ll_w4a16_engine_id(int64_t m, int64_t n, int64_t k, int group_size, int epilogue) {
  if (!ll_w4a16_prepacked_supported(m, n, k, group_size)) return -1;
  if ((epilogue & 3) == 2 && ll_w4a16_partials_count_ex(m, n, k, group_size, epilogue) == 0) return -1;
  return (int)w4a16_engine(m, n, k, group_size, epilogue);
}

extern "C" int ll_w4a16_matmul_prepacked(void* out, const void* x, const void* wpacked, const void* spacked,
                                         const void* bias, int64_t m, int64_t n, int64_t k, int group_size,
                                         int64_t x_stride_m, float* workspace, int32_t* counters, int epilogue,
                                         void* stream) {
  if (m < 0 || n <= 0 || k <= 0 || group_size <= 0) return LL_ERR_SHAPE;
  if (m == 0) return LL_OK;
  if (!ll_w4a16_prepacked_supported(m, n, k, group_size) || x_stride_m % 8 != 0 || ((epilogue & 1) && (n & 1))) return LL_ERR_SHAPE;
  if (!out || !x || !wpacked || !spacked || !workspace || !counters) return LL_ERR_ARG;
  if (!ll_aligned16(x) || !ll_aligned16(wpacked) || !ll_aligned16(spacked)) return LL_ERR_ARG;
  if ((m - 1) * x_stride_m * 2 + k * 2 >= (1ll << 31)) return LL_ERR_SHAPE;
  const bool partials = (epilogue & 3) == 2;
  const int kslices = partials ? v3_partials_count(m, n, k, group_size) : 1;  // the unit loop's k-split, shared by the row-group loop
  if (partials && (bias || !kslices)) return LL_ERR_SHAPE;
  switch (w4a16_engine(m, n, k, group_size, epilogue)) {
    case W4_SHORT_PARTIALS:
      return ss_launch(out, x, wpacked, spacked, m, n, k, group_size, x_stride_m, stream);
    case W4_ROW_GROUPS:
      return v4_launch(out, x, wpacked, spacked, bias, m, n, k, group_size, x_stride_m, epilogue & 3, kslices, stream);
    case W4_SHORT_FULL:
      return sf_launch(out, x, wpacked, spacked, bias, m, n, k, group_size, x_stride_m, epilogue, stream);
    default:
      return v3_launch(out, x, wpacked, spacked, bias, m, n, k, group_size, x_stride_m, workspace, counters, epilogue, stream);
  }
}
