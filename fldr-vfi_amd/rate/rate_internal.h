// libfldr_rate.so, shared between the host side (rate_host.hip) and the kernels (rate_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_rate.h"
#include "luma8_device.h"

namespace fldr_rate_impl {
using namespace fldr_luma8;

// The scene state (FLDR_SCENE_STATE_BYTES of device memory): the result the caller reads, then the kernels' accumulators.
constexpr int STATE_SAD_OFFSET = 64;       // uint64: the sum of absolute differences, added to by every workgroup
constexpr int STATE_HIST_OFFSET = 1024;    // int32[256]: h0[b] - h1[b], added to by every workgroup

constexpr int SELECT_MAX_OUT = 64;         // outputs one select launch serves (its kernel argument holds their planes)

// zero `state`, accumulate sad and h0 - h1 over the two luma planes, reduce and decide: three launches on `stream`
int scene_measure(const void* y0, int64_t pitch0, const void* y1, int64_t pitch1, int H, int W, int mode, int sad_permille, int hist_permille,
                  void* state, hipStream_t stream);

// If state->cut: out[k] = copy of in[t[k] < 0.5f ? 0 : 1] for k < n (n <= SELECT_MAX_OUT), rows[p] rows of row_bytes[p] bytes of each of
// the np planes; else nothing.
int select_on_cut(const void* state, const float* t, const fldr_video_frame in[2], const fldr_video_frame* out, int n, int np,
                  const int64_t row_bytes[3], const int rows[3], hipStream_t stream);

}  // namespace fldr_rate_impl
