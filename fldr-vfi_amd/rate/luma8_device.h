// The 8-bit luma reader of the measure kernels (fldr_rate.h's y8): how the value sits in a sample of each format, 16 bytes of a row as
// four dwords of reduced samples, their sum of absolute differences, and the host's side of it (the mode of a format, the bytes of a
// row, whether the 16-byte loads may be used, the launch of a kernel template by mode).  Included through rate_internal.h and
// ../cadence/cadence_internal.h: scene_accumulate_kernel and repeat_tiles_kernel read luma with the same text, inlined into each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fldr_video.h"

namespace fldr_luma8 {

// how the 8-bit luma value sits in a sample
enum { Y8_BYTE = 0,                    // depth 8: the byte
       Y8_P010 = 1,                    // word >> 8
       Y8_LOW10 = 2 };                 // (word & 0x3ff) >> 2

template <int MODE> __device__ __forceinline__ uint32_t reduce8(uint32_t w) {           // a dword of samples -> y8 in each sample's low byte
    return MODE == Y8_BYTE ? w : MODE == Y8_P010 ? ((w >> 8) & 0x00ff00ffu) : ((w >> 2) & 0x00ff00ffu);
}
template <int MODE> __device__ __forceinline__ int sample8(const uint8_t* p) {
    if (MODE == Y8_BYTE) return *p;
    const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
    return MODE == Y8_P010 ? (int)(w >> 8) : (int)((w >> 2) & 0xffu);
}

// 16 bytes at p -> four dwords; !VEC: from loads of one sample each (p is then only sample-aligned)
template <int MODE, bool VEC> __device__ __forceinline__ void load16(const uint8_t* p, uint32_t d[4]) {
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else if (MODE == Y8_BYTE) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            d[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    } else {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = (uint32_t)q[2 * i] | ((uint32_t)q[2 * i + 1] << 16);
    }
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

// KERNEL<MODE, VEC><<<grid, threads, 0, stream>>>(args) for the mode and vec of a call
#define LUMA8_LAUNCH_VEC(KERNEL, M, vec, grid, threads, stream, ...) do { \
        if (vec) KERNEL<M, true><<<grid, threads, 0, stream>>>(__VA_ARGS__); \
        else KERNEL<M, false><<<grid, threads, 0, stream>>>(__VA_ARGS__); } while (0)
#define LUMA8_LAUNCH(KERNEL, mode, vec, grid, threads, stream, ...) do { \
        if ((mode) == fldr_luma8::Y8_BYTE) LUMA8_LAUNCH_VEC(KERNEL, fldr_luma8::Y8_BYTE, vec, grid, threads, stream, __VA_ARGS__); \
        else if ((mode) == fldr_luma8::Y8_P010) LUMA8_LAUNCH_VEC(KERNEL, fldr_luma8::Y8_P010, vec, grid, threads, stream, __VA_ARGS__); \
        else LUMA8_LAUNCH_VEC(KERNEL, fldr_luma8::Y8_LOW10, vec, grid, threads, stream, __VA_ARGS__); } while (0)
