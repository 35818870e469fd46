// The 16-byte sample-row reader of the bandwidth kernels above the video library, device side, inlined into each kernel that uses it:
// 16 bytes of samples as four dwords (load16), the weighted add of their values (add16), the same over the frames of a launch with four
// frames' loads in flight (gather16), the uint32 accumulator of such a group as aligned uint4 (load_acc, store_acc), and the launch of a
// <MODE, VEC> kernel template by the sample form of a call.  Included by ../shutter/shutter_kernels.hip and ../light/light_kernels.hip
// (all of it) and by ../rate/luma8_device.h, and through it the rate, cadence and pipe libraries (load16 and the launch) and the weave
// kernels of ../field/field_kernels.hip and ../interlace/interlace_kernels.hip (a group sample by sample: Sample, value_of, canonical,
// raw_at, put_at, load_group, store_group, and the launch of a <FORM, ...> kernel template) and the resize kernel of
// ../scale/scale_kernels.hip (Sample, value_of, canonical, load_raw, store_group).  Where a lane's 16 bytes lie and what is done with the samples stay with the including kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fldr_sample16 {

// how the value sits in a sample: the numbers a library's own mode names (S_*, Y8_*) carry
enum { FORM_BYTE = 0,                  // depth 8: a byte
       FORM_P010 = 1,                  // a 16-bit word, the value in its high bits
       FORM_LOW10 = 2 };               // a 16-bit word, the value in its low bits

// 16 bytes at p -> four dwords; !VEC: from loads of one sample each (p is then only sample-aligned).  WORDS: the samples are 16-bit words
template <bool WORDS, bool VEC> __device__ __forceinline__ void load16(const uint8_t* p, uint32_t d[4]) {
    if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else if (!WORDS) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            d[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    } else {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = (uint32_t)q[2 * i] | ((uint32_t)q[2 * i + 1] << 16);
    }
}

// ---- a group sample by sample: what the weave kernels of the deinterlacing and interlacing libraries share ------------------------------
template <int FORM> struct Sample {
    static constexpr bool WORDS = FORM != FORM_BYTE;
    static constexpr int BPS = WORDS ? 2 : 1;                         // bytes per sample
    static constexpr int NS = 16 / BPS;                               // samples per group
    static constexpr int MX = WORDS ? 1023 : 255;
};

template <int FORM> __device__ __forceinline__ int value_of(uint32_t raw) {
    return FORM == FORM_BYTE ? (int)raw : FORM == FORM_P010 ? (int)(raw >> 6) : (int)(raw & 0x3ffu);
}

template <int FORM> __device__ __forceinline__ uint32_t canonical(int o) { return FORM == FORM_P010 ? (uint32_t)o << 6 : (uint32_t)o; }

// sample i of a group, as it sits in memory
template <int FORM> __device__ __forceinline__ uint32_t raw_at(const uint32_t d[4], int i) {
    return Sample<FORM>::WORDS ? (d[i >> 1] >> (16 * (i & 1))) & 0xffffu : (d[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

template <int FORM> __device__ __forceinline__ void put_at(uint32_t d[4], int i, uint32_t raw) {
    if (Sample<FORM>::WORDS) d[i >> 1] |= raw << (16 * (i & 1));
    else d[i >> 2] |= raw << (8 * (i & 3));
}

template <int FORM> __device__ __forceinline__ uint32_t load_raw(const uint8_t* p) {
    return Sample<FORM>::WORDS ? (uint32_t)*reinterpret_cast<const uint16_t*>(p) : (uint32_t)*p;
}

// the nv samples at p -> four dwords (the others zero); a whole group with load16
template <int FORM, bool VEC> __device__ __forceinline__ void load_group(const uint8_t* p, int nv, uint32_t d[4]) {
    using S = Sample<FORM>;
    if (nv == S::NS) { load16<S::WORDS, VEC>(p, d); return; }
    d[0] = d[1] = d[2] = d[3] = 0u;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) if (i < nv) put_at<FORM>(d, i, load_raw<FORM>(p + i * S::BPS));
}

template <int FORM, bool VEC> __device__ __forceinline__ void store_group(uint8_t* p, int nv, const uint32_t d[4]) {
    using S = Sample<FORM>;
    if (VEC && nv == S::NS) { *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]); return; }
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
        if (i >= nv) continue;
        if (S::WORDS) reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)raw_at<FORM>(d, i);
        else p[i] = (uint8_t)raw_at<FORM>(d, i);
    }
}

// s += w * map(code) for the samples in four dwords: a byte each, or the 10 bits from bit SHIFT of each word
template <bool WORDS, int SHIFT, class Map>
__device__ __forceinline__ void add16(uint32_t* s, const uint32_t d[4], uint32_t w, Map map) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!WORDS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[4 * i + j] += w * map((d[i] >> (8 * j)) & 0xffu);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) s[2 * i + j] += w * map((d[i] >> (16 * j + SHIFT)) & 0x3ffu);
        }
    }
}

// the weighted sum of the 16 bytes at at(k) of frames k = 0 .. n - 1, added to s; four frames' loads in flight
template <bool WORDS, int SHIFT, bool VEC, class At, class Map>
__device__ __forceinline__ void gather16(int n, const uint32_t* weight, At at, Map map, uint32_t* s) {
    int k0 = 0;
    for (; k0 + 4 <= n; k0 += 4) {
        uint32_t d[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) load16<WORDS, VEC>(at(k0 + u), d[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) add16<WORDS, SHIFT>(s, d[u], weight[k0 + u], map);
    }
    for (; k0 < n; ++k0) {
        uint32_t d[4];
        load16<WORDS, VEC>(at(k0), d);
        add16<WORDS, SHIFT>(s, d, weight[k0], map);
    }
}

// the SPC sums of one group, SPC / 4 aligned uint4 at ap
template <int SPC> __device__ __forceinline__ void load_acc(const uint32_t* ap, uint32_t* s) {
#pragma unroll
    for (int i = 0; i < SPC / 4; ++i) {
        const uint4 v = reinterpret_cast<const uint4*>(ap)[i];
        s[4 * i] = v.x; s[4 * i + 1] = v.y; s[4 * i + 2] = v.z; s[4 * i + 3] = v.w;
    }
}

template <int SPC> __device__ __forceinline__ void store_acc(uint32_t* ap, const uint32_t* s) {
#pragma unroll
    for (int i = 0; i < SPC / 4; ++i) reinterpret_cast<uint4*>(ap)[i] = make_uint4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
}

}  // namespace fldr_sample16

// KERNEL<M, VEC><<<grid, threads, 0, stream>>>(args) for the vec of a call, and for its mode (a FORM_* number) as well
#define SAMPLE16_LAUNCH_VEC(KERNEL, M, vec, grid, threads, stream, ...) do { \
        if (vec) KERNEL<M, true><<<grid, threads, 0, stream>>>(__VA_ARGS__); \
        else KERNEL<M, false><<<grid, threads, 0, stream>>>(__VA_ARGS__); } while (0)
#define SAMPLE16_LAUNCH(KERNEL, mode, vec, grid, threads, stream, ...) do { \
        if ((mode) == fldr_sample16::FORM_BYTE) SAMPLE16_LAUNCH_VEC(KERNEL, fldr_sample16::FORM_BYTE, vec, grid, threads, stream, __VA_ARGS__); \
        else if ((mode) == fldr_sample16::FORM_P010) SAMPLE16_LAUNCH_VEC(KERNEL, fldr_sample16::FORM_P010, vec, grid, threads, stream, __VA_ARGS__); \
        else SAMPLE16_LAUNCH_VEC(KERNEL, fldr_sample16::FORM_LOW10, vec, grid, threads, stream, __VA_ARGS__); } while (0)
// KERNEL<FORM, ...><<<grid, threads, 0, stream>>> ARGS for the form of a call: ARGS the kernel's arguments in their parentheses, ... the
// template arguments after the form, if there are any
#define SAMPLE16_LAUNCH_FORM(KERNEL, form, grid, threads, stream, ARGS, ...) do { \
        if ((form) == fldr_sample16::FORM_BYTE) KERNEL<fldr_sample16::FORM_BYTE, ##__VA_ARGS__><<<grid, threads, 0, stream>>> ARGS; \
        else if ((form) == fldr_sample16::FORM_P010) KERNEL<fldr_sample16::FORM_P010, ##__VA_ARGS__><<<grid, threads, 0, stream>>> ARGS; \
        else KERNEL<fldr_sample16::FORM_LOW10, ##__VA_ARGS__><<<grid, threads, 0, stream>>> ARGS; } while (0)
