// Internals shared by the two translation units of libfldr_video.so (hidden: -fvisibility=hidden + video/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_video.h"
#include "yuv_color.h"

namespace fldr_video_impl {
// Two YUV 4:2:0 frames (layout: FLDR_VIDEO_NV12 / I420) -> the planar uint8 pair [1,2,3,H,W] (plane c = BGR channel c), one launch.
int yuv420_to_planar_pair(const fldr_video_frame in[2], int layout, const YuvCoeffs& k, uint8_t* pair, int H, int W, hipStream_t stream);
// One planar uint8 frame [1,3,H,W] (BGR planes) -> one YUV 4:2:0 frame; bytes between a row's end and its pitch are not written.
int planar_to_yuv420(const uint8_t* planar, const fldr_video_frame& out, int layout, const YuvCoeffs& k, int H, int W, hipStream_t stream);
// The same two at depth 10: 16-bit words in the YUV planes (NV12 = P010, value << 6; I420 = yuv420p10le, value in the low bits; pitches in
// bytes), planar uint16 BGR code values 0 .. 1023 on the model's side; k from YUV_COEFFS_10.
int yuv420_to_planar_pair10(const fldr_video_frame in[2], int layout, const YuvCoeffs& k, uint16_t* pair, int H, int W, hipStream_t stream);
int planar_to_yuv420_10(const uint16_t* planar, const fldr_video_frame& out, int layout, const YuvCoeffs& k, int H, int W, hipStream_t stream);
#ifdef FLDR_TEST_HOOKS
// libfldr_video_test.so only: the form the most recent of the four launchers above chose (1: VEC, 0: per-sample, -1: none launched yet)
extern int g_last_path;
#endif
}  // namespace fldr_video_impl
