// The 8-bit luma reader of the measure kernels (fldr_rate.h's y8): how the value sits in a sample of each format, the reduced samples of a
// dword, their sum of absolute differences, and the host's side of it (the mode of a format, the bytes of a row, whether the 16-byte loads
// may be used).  The 16 bytes of a row as four dwords (load16) and the launch of a kernel template by mode (SAMPLE16_LAUNCH) are those of
// ../video/sample16_device.h.  Included through rate_internal.h and, by way of tile_reduce_device.h, the cadence, pulldown and probe
// libraries' internal headers: scene_accumulate_kernel and the three tiles kernels read luma with the same text, inlined into each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/sample16_device.h"
#include "fldr_video.h"

namespace fldr_luma8 {

// how the 8-bit luma value sits in a sample
enum { Y8_BYTE = fldr_sample16::FORM_BYTE,       // depth 8: the byte
       Y8_P010 = fldr_sample16::FORM_P010,       // word >> 8
       Y8_LOW10 = fldr_sample16::FORM_LOW10 };   // (word & 0x3ff) >> 2

using fldr_sample16::load16;           // 16 bytes of a row -> four dwords, as load16<MODE != Y8_BYTE, VEC>

template <int MODE> __device__ __forceinline__ uint32_t reduce8(uint32_t w) {           // a dword of samples -> y8 in each sample's low byte
    return MODE == Y8_BYTE ? w : MODE == Y8_P010 ? ((w >> 8) & 0x00ff00ffu) : ((w >> 2) & 0x00ff00ffu);
}
template <int MODE> __device__ __forceinline__ int sample8(const uint8_t* p) {
    if (MODE == Y8_BYTE) return *p;
    const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
    return MODE == Y8_P010 ? (int)(w >> 8) : (int)((w >> 2) & 0xffu);
}

// acc + the sum of absolute differences of the samples of two reduced dwords: v_sad_u8 on four bytes, v_sad_u16 on two words
template <int MODE> __device__ __forceinline__ uint32_t sad_dword(uint32_t a, uint32_t b, uint32_t acc) {
    return MODE == Y8_BYTE ? __builtin_amdgcn_sad_u8(a, b, acc) : __builtin_amdgcn_sad_u16(a, b, acc);
}

// the host's side
static inline int luma_mode(bool deep, int layout) { return !deep ? Y8_BYTE : layout == FLDR_VIDEO_NV12 ? Y8_P010 : Y8_LOW10; }

static inline int64_t luma_row_bytes(int W, int mode) { return (int64_t)W * (mode == Y8_BYTE ? 1 : 2); }

// both plane addresses and pitches 16-byte aligned: the 16-byte loads (VEC) may be used
static inline bool luma_vec_ok(const void* y0, int64_t pitch0, const void* y1, int64_t pitch1) {
    return (((uintptr_t)y0 | (uintptr_t)y1 | (uintptr_t)pitch0 | (uintptr_t)pitch1) & 15) == 0;
}

}  // namespace fldr_luma8
