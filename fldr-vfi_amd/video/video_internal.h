// Internals shared by the two translation units of libfldr_video.so (hidden: -fvisibility=hidden + video/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_video.h"
#include "yuv_color.h"

namespace fldr_video_impl {
// Two YUV 4:2:0 frames in `fmt` (checked by the caller) -> the planar BGR pair [1,2,3,H,W] (plane c = BGR channel c), one launch: uint8, or
// at depth 10 uint16 code values 0 .. 1023 (16-bit words in the YUV planes: NV12 = P010, value << 6; I420 = yuv420p10le, value in the low
// bits; pitches in bytes).  k: YUV_COEFFS or YUV_COEFFS_10 of the format.
int yuv420_to_planar_pair(const fldr_video_frame in[2], const fldr_video_format& fmt, const YuvCoeffs& k, void* pair, int H, int W, hipStream_t stream);
// One planar BGR frame [1,3,H,W] -> one YUV 4:2:0 frame in `fmt`; bytes between a row's end and its pitch are not written.
int planar_to_yuv420(const void* planar, const fldr_video_frame& out, const fldr_video_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream);
#ifdef FLDR_TEST_HOOKS
// libfldr_video_test.so only: the form the most recent of the two launchers above chose (1: VEC, 0: per-sample, -1: none launched yet)
extern int g_last_path;
#endif
}  // namespace fldr_video_impl
