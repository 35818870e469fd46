// Internals shared by the two translation units of libfldr_rgb.so (hidden: -fvisibility=hidden + rgb/exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_rgb.h"

namespace fldr_rgb_impl {

// Pixels a thread owns along a row of a word layout (the byte layouts and the two 10-bit words): 16 bytes of the frame, and 4 (uint8)
// or 8 (uint16) bytes of each BGR plane, so consecutive lanes touch consecutive bytes on both sides in every instruction.  The wide form
// needs W % 4 == 0; every planar row then starts on a whole access.
constexpr int RUN_WORDS = 4;
// Bytes a thread owns along a row of a plane of GBRP / GBRAP: 16 or 8 samples.
constexpr int RUN_PLANE_BYTES = 16;
constexpr int MAX_FRAMES = 2;                        // frames one input launch converts (blockIdx.z)
constexpr int ALPHA_MAX_OUT = 64;                    // outputs one alpha launch serves (blockIdx.y)

inline bool word_layout(const fldr_rgb_format& f) { return f.layout < FLDR_RGB_GBRP; }
inline bool words16(const fldr_rgb_format& f) { return f.depth == 10; }        // the planar BGR samples are uint16
// bits of a format's alpha: 8 (byte layouts, GBRAP at depth 8), 2 (the 10-bit words), 10 (GBRAP at depth 10), 0 (GBRP: none)
inline int alpha_bits(const fldr_rgb_format& f) {
    if (f.layout <= FLDR_RGB_ABGR) return 8;
    if (f.layout <= FLDR_RGB_X2BGR10) return 2;
    return f.layout == FLDR_RGB_GBRAP ? (words16(f) ? 10 : 8) : 0;
}

// n (1 .. MAX_FRAMES) frames in `fmt` (checked by the caller) -> planar BGR [n,3,H,W] of uint8 / uint16 code values.
int to_planar(const fldr_rgb_frame* in, int n, const fldr_rgb_format& fmt, void* planar, int H, int W, hipStream_t stream);
// One planar BGR frame [3,H,W] -> one frame in `fmt` with opaque alpha; bytes between a row's end and its pitch are not written.
int from_planar(const void* planar, const fldr_rgb_frame& out, const fldr_rgb_format& fmt, int H, int W, hipStream_t stream);
// The alpha of n (1 .. ALPHA_MAX_OUT) frames `out` in `fout` from the two frames `in` in `fin` by the policy fout.alpha (NEARER or BLEND;
// both formats have alpha of one width: checked by the caller) at the times t[0 .. n-1], read on the device.  Only alpha is written.
int write_alpha(const fldr_rgb_frame in[2], const fldr_rgb_format& fin, const fldr_rgb_frame* out, int n, const fldr_rgb_format& fout,
                const float* t, int H, int W, hipStream_t stream);

}  // namespace fldr_rgb_impl
