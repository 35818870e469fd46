// Internals shared by the two translation units of libfldr_pack10.so (hidden: -fvisibility=hidden + pack10/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_pack10.h"
#include "../video/yuv_color.h"

namespace fldr_pack10_impl {

using fldr_video_impl::YuvCoeffs;

// Luma pixels a thread owns along a row.  v210: one 16-byte group = 6 pixels, 12 bytes of each BGR plane: consecutive lanes then touch
// consecutive bytes on both sides (a run of 24 pixels, four groups and three 16-byte accesses per plane, was measured 18 - 42 % slower
// than the semiplanar 4:2:2 converter: DESIGN_LOG.md).  Y210, Y410: 8 pixels (32 bytes of the container, 16 of each BGR plane; the wide
// form needs W % 8 == 0, every planar row then starts 16-byte aligned).
constexpr int RUN_V210 = 6, RUN_WORDS = 8;
constexpr int MAX_FRAMES = 2;                        // frames one input launch converts (blockIdx.z)

// n (1 .. MAX_FRAMES) frames in `fmt` (checked by the caller) -> planar BGR [n,3,H,W] of uint16 code values.
int to_planar(const fldr_pack10_frame* in, int n, const fldr_pack10_format& fmt, const YuvCoeffs& k, void* planar, int H, int W, hipStream_t stream);
// One planar BGR frame [3,H,W] -> one frame in `fmt`; bytes between a row's end and its pitch are not written.
int from_planar(const void* planar, const fldr_pack10_frame& out, const fldr_pack10_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream);

}  // namespace fldr_pack10_impl
