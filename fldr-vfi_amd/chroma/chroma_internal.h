// Internals shared by the two translation units of libfldr_chroma.so (hidden: -fvisibility=hidden + chroma/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_chroma.h"
#include "../video/yuv_color.h"

namespace fldr_chroma_impl {

using fldr_video_impl::YuvCoeffs;

// Luma pixels a thread owns along a row: 16 at depth 8, 8 at depth 10 (16 bytes of Y and of each BGR plane per lane either way; the
// narrowest plane, planar 4:2:2 chroma, is then 8 bytes per lane).  The wide form needs W to be a multiple of the run.
constexpr int RUN8 = 16, RUN16 = 8;
constexpr int MAX_FRAMES = 2;                        // frames one input launch converts (blockIdx.z)

// n (1 .. MAX_FRAMES) frames in `fmt` (checked by the caller) -> planar BGR [n,3,H,W]: uint8, or uint16 code values at depth 10.
int to_planar(const fldr_chroma_frame* in, int n, const fldr_chroma_format& fmt, const YuvCoeffs& k, void* planar, int H, int W, hipStream_t stream);
// One planar BGR frame [3,H,W] -> one frame in `fmt`; bytes between a row's end and its pitch are not written.
int from_planar(const void* planar, const fldr_chroma_frame& out, const fldr_chroma_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream);

}  // namespace fldr_chroma_impl
