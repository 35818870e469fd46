// The two kernels of libfldr_video.so: YUV 4:2:0 (NV12 / I420, pitched planes) on either side of the model's 8-bit planar forward.
// Both are bandwidth kernels.  A thread owns 4 luma pixels along a row (the input kernel: one row; the output kernel: the two rows
// of one chroma row), so rows are read and written 4 bytes per lane when every plane pointer and pitch is 4-byte aligned and W is a
// multiple of 4 (VEC); otherwise the same arithmetic runs on byte accesses with the indices clamped to the row.  The arithmetic is
// the colour definition of yuv_color.h, in int32, exactly as tests/yuv_oracle.py states it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "video_internal.h"

namespace fldr_video_impl {

#define VK_TX 64                 // threads along a row (x 4 pixels = 256 luma columns per block)
#define VK_TY 4                  // rows per block

// The test build (libfldr_video_test.so, include/fldr_video_test_hooks.h) records which form a launcher chose; the product compiles
// VK_NOTE_PATH to nothing.
#ifdef FLDR_TEST_HOOKS
int g_last_path = -1;
#define VK_NOTE_PATH(vec) (g_last_path = (vec) ? 1 : 0)
#else
#define VK_NOTE_PATH(vec) ((void)0)
#endif

__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return *reinterpret_cast<const uint16_t*>(p); }
__device__ __forceinline__ int byte_of(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xffu); }
// Four values in 0..255 -> one dword (a in the low byte), through v_perm_b32.  Packed with shifts and ORs, hipcc turns the input
// kernel's "clamp (x >> 19) to 0..255, pack two" into v_ashr_pk_u8_i32 and ORs its result with the upper bytes, which assumes the
// instruction clears bits 16..31; on gfx950 pixels 2 and 3 of every dword then came out ORed with stale bits (measured).  The library
// is checked for the instruction (tests/test_video_cpu.py).
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x0c0c0400u);     // bytes: a, b, 0, 0
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x0c0c0400u);     // bytes: c, d, 0, 0
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);                                    // a, b, c, d
}

// ---- (a) two YUV 4:2:0 frames -> planar BGR pair ---------------------------------------------------------------------------------
struct InArgs {
    const uint8_t* plane[2][3];
    int64_t pitch[2][3];
    uint8_t* dst;                // [2][3][H][W]
    int H, W;
    YuvCoeffs k;
};

// Chroma samples c0 = x0/2, c1, c2 (clamped into the row) of one chroma row: u[0..2], v[0..2].
template <int LAYOUT, bool VEC>
__device__ __forceinline__ void load_chroma(const InArgs& a, int f, int r, int c0, int cw, int* u, int* v) {
    const int c1 = min(c0 + 1, cw - 1), c2 = min(c0 + 2, cw - 1);
    if (LAYOUT == FLDR_VIDEO_NV12) {
        const uint8_t* row = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        if (VEC) {                                                   // c1 = c0 + 1 here (W % 4 == 0): one dword, then U, V of c2
            const uint32_t w = ld32(row + 2 * c0);
            const uint32_t w2 = c2 > c1 ? ld16(row + 2 * c2) : (w >> 16);
            u[0] = byte_of(w, 0); v[0] = byte_of(w, 1); u[1] = byte_of(w, 2); v[1] = byte_of(w, 3);
            u[2] = byte_of(w2, 0); v[2] = byte_of(w2, 1);
        } else {
            u[0] = row[2 * c0]; v[0] = row[2 * c0 + 1];
            u[1] = row[2 * c1]; v[1] = row[2 * c1 + 1];
            u[2] = row[2 * c2]; v[2] = row[2 * c2 + 1];
        }
    } else {
        const uint8_t* ru = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        const uint8_t* rv = a.plane[f][2] + (int64_t)r * a.pitch[f][2];
        if (VEC) {                                                   // c0 even: a 2-byte load of (c0, c0 + 1), then c2
            const uint32_t wu = ld16(ru + c0), wv = ld16(rv + c0);
            u[0] = byte_of(wu, 0); u[1] = byte_of(wu, 1); v[0] = byte_of(wv, 0); v[1] = byte_of(wv, 1);
        } else {
            u[0] = ru[c0]; u[1] = ru[c1]; v[0] = rv[c0]; v[1] = rv[c1];
        }
        u[2] = ru[c2]; v[2] = rv[c2];
    }
}

template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void yuv420_to_planar_pair_kernel(InArgs a) {
    const int x0 = 4 * (blockIdx.x * VK_TX + threadIdx.x);
    const int y = blockIdx.y * VK_TY + threadIdx.y;
    const int f = blockIdx.z;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    // vertical taps: even y -> rows y/2 - 1, y/2 with weights 1, 3; odd y -> rows (y-1)/2, (y+1)/2 with 3, 1 (clamped)
    const bool ev = (y & 1) == 0;
    const int ra = ev ? max((y >> 1) - 1, 0) : (y >> 1);
    const int rb = ev ? (y >> 1) : min((y >> 1) + 1, ch - 1);
    const int wa = ev ? 1 : 3, wb = 4 - wa;
    int ua[3], va[3], ub[3], vb[3];
    load_chroma<LAYOUT, VEC>(a, f, ra, x0 >> 1, cw, ua, va);
    load_chroma<LAYOUT, VEC>(a, f, rb, x0 >> 1, cw, ub, vb);
    int yy[4];
    const uint8_t* yrow = a.plane[f][0] + (int64_t)y * a.pitch[f][0];
    if (VEC) {
        const uint32_t w = ld32(yrow + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) yy[j] = byte_of(w, j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) yy[j] = yrow[min(x0 + j, W - 1)];
    }
    const YuvCoeffs& k = a.k;
    int bb[4], gg[4], rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // horizontal taps of pixel x0 + j: 2 on column c0 + j/2 (even), 1 + 1 on c0 + (j-1)/2 and c0 + (j+1)/2 (odd; clamped)
        const int ia = j >> 1, ib = (j + 1) >> 1;
        const int hu_a = ua[ia] + ua[ib], hu_b = ub[ia] + ub[ib];
        const int hv_a = va[ia] + va[ib], hv_b = vb[ia] + vb[ib];
        const int cu = wa * hu_a + wb * hu_b - 1024;
        const int cv = wa * hv_a + wb * hv_b - 1024;
        const int yv = (yy[j] - k.yoff) * 8 * k.ky;
        rr[j] = clamp8((yv + k.krv * cv + (1 << 18)) >> 19);
        gg[j] = clamp8((yv - k.kgu * cu - k.kgv * cv + (1 << 18)) >> 19);
        bb[j] = clamp8((yv + k.kbu * cu + (1 << 18)) >> 19);
    }
    const int64_t HW = (int64_t)H * W;
    uint8_t* d = a.dst + (int64_t)f * 3 * HW + (int64_t)y * W + x0;
    if (VEC) {
        *reinterpret_cast<uint32_t*>(d) = pack4(bb[0], bb[1], bb[2], bb[3]);
        *reinterpret_cast<uint32_t*>(d + HW) = pack4(gg[0], gg[1], gg[2], gg[3]);
        *reinterpret_cast<uint32_t*>(d + 2 * HW) = pack4(rr[0], rr[1], rr[2], rr[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) { d[j] = (uint8_t)bb[j]; d[HW + j] = (uint8_t)gg[j]; d[2 * HW + j] = (uint8_t)rr[j]; }
    }
}

static bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int yuv420_to_planar_pair(const fldr_video_frame in[2], int layout, const YuvCoeffs& k, uint8_t* pair, int H, int W, hipStream_t stream) {
    InArgs a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    bool vec = (W & 3) == 0;
    for (int f = 0; f < 2; ++f)
        for (int p = 0; p < 3; ++p) {
            a.plane[f][p] = p < np ? (const uint8_t*)in[f].plane[p] : nullptr;
            a.pitch[f][p] = p < np ? in[f].pitch[p] : 0;
            if (p < np) vec = vec && al4(in[f].plane[p]) && (in[f].pitch[p] & 3) == 0;
        }
    a.dst = pair; a.H = H; a.W = W; a.k = k;
    VK_NOTE_PATH(vec);
    const dim3 grid((((W + 3) >> 2) + VK_TX - 1) / VK_TX, (H + VK_TY - 1) / VK_TY, 2), block(VK_TX, VK_TY);
    if (layout == FLDR_VIDEO_NV12) {
        if (vec) hipLaunchKernelGGL((yuv420_to_planar_pair_kernel<FLDR_VIDEO_NV12, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((yuv420_to_planar_pair_kernel<FLDR_VIDEO_NV12, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((yuv420_to_planar_pair_kernel<FLDR_VIDEO_I420, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((yuv420_to_planar_pair_kernel<FLDR_VIDEO_I420, false>), grid, block, 0, stream, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// ---- (b) planar BGR frame -> YUV 4:2:0 -----------------------------------------------------------------------------------------
struct OutArgs {
    const uint8_t* src;          // [3][H][W]
    uint8_t* plane[3];
    int64_t pitch[3];
    int H, W;
    YuvCoeffs k;
};

// Pixels x0 - 1 .. x0 + 3 (clamped into the row) of row y of plane c: px[0..4].
template <bool VEC>
__device__ __forceinline__ void load_px(const uint8_t* row, int x0, int W, int* px) {
    px[0] = row[max(x0 - 1, 0)];
    if (VEC) {
        const uint32_t w = ld32(row + x0);
#pragma unroll
        for (int j = 0; j < 4; ++j) px[1 + j] = byte_of(w, j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[1 + j] = row[min(x0 + j, W - 1)];
    }
}

template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void planar_to_yuv420_kernel(OutArgs a) {
    const int x0 = 4 * (blockIdx.x * VK_TX + threadIdx.x);
    const int cj = blockIdx.y * VK_TY + threadIdx.y;                 // chroma row: luma rows 2 cj, 2 cj + 1 (clamped)
    const int H = a.H, W = a.W;
    if (x0 >= W || 2 * cj >= H) return;
    const int cw = (W + 1) >> 1;
    const int64_t HW = (int64_t)H * W;
    const YuvCoeffs& k = a.k;
    int up[5], vp[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) up[m] = vp[m] = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int y = min(2 * cj + h, H - 1);
        int b[5], g[5], r[5];
        const uint8_t* s = a.src + (int64_t)y * W;
        load_px<VEC>(s, x0, W, b);
        load_px<VEC>(s + HW, x0, W, g);
        load_px<VEC>(s + 2 * HW, x0, W, r);
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            up[m] += k.kur * r[m] + k.kug * g[m] + k.kub * b[m];
            vp[m] += k.kvr * r[m] + k.kvg * g[m] + k.kvb * b[m];
        }
        if (2 * cj + h >= H) continue;                               // odd H: the last chroma row has one luma row
        int yb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            yb[j] = min(((k.kyr * r[1 + j] + k.kyg * g[1 + j] + k.kyb * b[1 + j] + (1 << 15)) >> 16) + k.yoff, 255);
        uint8_t* yrow = a.plane[0] + (int64_t)y * a.pitch[0] + x0;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(yrow) = pack4(yb[0], yb[1], yb[2], yb[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) yrow[j] = (uint8_t)yb[j];
        }
    }
    // chroma columns i0 = x0/2 (luma x0 - 1, x0, x0 + 1 weighted 1, 2, 1) and i0 + 1 (x0 + 1, x0 + 2, x0 + 3)
    const int i0 = x0 >> 1;
    const int u0 = clamp8(((up[0] + 2 * up[1] + up[2] + (1 << 18)) >> 19) + 128);
    const int v0 = clamp8(((vp[0] + 2 * vp[1] + vp[2] + (1 << 18)) >> 19) + 128);
    const int u1 = clamp8(((up[2] + 2 * up[3] + up[4] + (1 << 18)) >> 19) + 128);
    const int v1 = clamp8(((vp[2] + 2 * vp[3] + vp[4] + (1 << 18)) >> 19) + 128);
    const bool has1 = i0 + 1 < cw;
    if (LAYOUT == FLDR_VIDEO_NV12) {
        uint8_t* row = a.plane[1] + (int64_t)cj * a.pitch[1] + 2 * i0;
        if (VEC) {                                                   // W % 4 == 0: both columns exist
            *reinterpret_cast<uint32_t*>(row) = pack4(u0, v0, u1, v1);
        } else {
            row[0] = (uint8_t)u0; row[1] = (uint8_t)v0;
            if (has1) { row[2] = (uint8_t)u1; row[3] = (uint8_t)v1; }
        }
    } else {
        uint8_t* ru = a.plane[1] + (int64_t)cj * a.pitch[1] + i0;
        uint8_t* rv = a.plane[2] + (int64_t)cj * a.pitch[2] + i0;
        if (VEC) {                                                   // i0 even: 2-byte aligned
            *reinterpret_cast<uint16_t*>(ru) = (uint16_t)(u0 | (u1 << 8));
            *reinterpret_cast<uint16_t*>(rv) = (uint16_t)(v0 | (v1 << 8));
        } else {
            ru[0] = (uint8_t)u0; rv[0] = (uint8_t)v0;
            if (has1) { ru[1] = (uint8_t)u1; rv[1] = (uint8_t)v1; }
        }
    }
}

int planar_to_yuv420(const uint8_t* planar, const fldr_video_frame& out, int layout, const YuvCoeffs& k, int H, int W, hipStream_t stream) {
    OutArgs a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    bool vec = (W & 3) == 0;
    for (int p = 0; p < 3; ++p) {
        a.plane[p] = p < np ? (uint8_t*)out.plane[p] : nullptr;
        a.pitch[p] = p < np ? out.pitch[p] : 0;
        if (p < np) vec = vec && al4(out.plane[p]) && (out.pitch[p] & 3) == 0;
    }
    a.src = planar; a.H = H; a.W = W; a.k = k;
    VK_NOTE_PATH(vec);
    const int ch = (H + 1) >> 1;
    const dim3 grid((((W + 3) >> 2) + VK_TX - 1) / VK_TX, (ch + VK_TY - 1) / VK_TY, 1), block(VK_TX, VK_TY);
    if (layout == FLDR_VIDEO_NV12) {
        if (vec) hipLaunchKernelGGL((planar_to_yuv420_kernel<FLDR_VIDEO_NV12, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((planar_to_yuv420_kernel<FLDR_VIDEO_NV12, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((planar_to_yuv420_kernel<FLDR_VIDEO_I420, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((planar_to_yuv420_kernel<FLDR_VIDEO_I420, false>), grid, block, 0, stream, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// ---- the same two converters at depth 10 -------------------------------------------------------------------------------------------
// Samples are little-endian 16-bit words, pitches stay in bytes.  FLDR_VIDEO_NV12 is P010 (the value in the high 10 bits: read as
// word >> 6, written as value << 6), FLDR_VIDEO_I420 is yuv420p10le (the value in the low 10 bits: read as word & 0x3ff).  The model's
// side is planar uint16 BGR, code values 0 .. 1023.  Same taps, same 16 fraction bits and the same shifts as the 8-bit kernels; the
// chroma centre is 512 (8 x 512 where those subtract 1024), the clamps are 0 .. 1023, the coefficients are YUV_COEFFS_10.  A thread owns
// 4 luma pixels again: 8 bytes per access when every plane pointer and pitch is 8-byte aligned and W is a multiple of 4 (VEC).
// Two values in 0 .. 1023 -> one dword through v_perm_b32, for the reason given at pack4: "shift, clamp, pack two" must not become a
// v_ashr_pk_* / v_cvt_pk_u16_* whose upper half the compiler then trusts (tests/test_video10_cpu.py looks at the listing).
#define VK_MAX10 1023
#define VK_MID10 512
__device__ __forceinline__ int clamp10(int v) { return min(max(v, 0), VK_MAX10); }
__device__ __forceinline__ uint32_t pack2h(int a, int b) { return __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x05040100u); }   // halves: a, b
__device__ __forceinline__ uint2 ld64(const uint8_t* p) { return *reinterpret_cast<const uint2*>(p); }
template <int LAYOUT>
__device__ __forceinline__ int smp10(uint32_t w16) { return LAYOUT == FLDR_VIDEO_NV12 ? (int)((w16 & 0xffffu) >> 6) : (int)(w16 & 0x3ffu); }
template <int LAYOUT>
__device__ __forceinline__ int word10(int v) { return LAYOUT == FLDR_VIDEO_NV12 ? v << 6 : v; }
__device__ __forceinline__ uint32_t ldh(const uint8_t* row, int i) { return reinterpret_cast<const uint16_t*>(row)[i]; }

struct InArgs16 {
    const uint8_t* plane[2][3];
    int64_t pitch[2][3];         // bytes
    uint16_t* dst;               // [2][3][H][W]
    int H, W;
    YuvCoeffs k;
};

template <int LAYOUT, bool VEC>
__device__ __forceinline__ void load_chroma10(const InArgs16& a, int f, int r, int c0, int cw, int* u, int* v) {
    const int c1 = min(c0 + 1, cw - 1), c2 = min(c0 + 2, cw - 1);
    if (LAYOUT == FLDR_VIDEO_NV12) {
        const uint8_t* row = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        if (VEC) {                                                   // c0 even, c1 = c0 + 1 (W % 4 == 0): U, V, U, V in 8 bytes, then c2
            const uint2 w = ld64(row + 4 * c0);
            const uint32_t w2 = c2 > c1 ? ld32(row + 4 * c2) : w.y;
            u[0] = smp10<LAYOUT>(w.x); v[0] = smp10<LAYOUT>(w.x >> 16); u[1] = smp10<LAYOUT>(w.y); v[1] = smp10<LAYOUT>(w.y >> 16);
            u[2] = smp10<LAYOUT>(w2); v[2] = smp10<LAYOUT>(w2 >> 16);
        } else {
            u[0] = smp10<LAYOUT>(ldh(row, 2 * c0)); v[0] = smp10<LAYOUT>(ldh(row, 2 * c0 + 1));
            u[1] = smp10<LAYOUT>(ldh(row, 2 * c1)); v[1] = smp10<LAYOUT>(ldh(row, 2 * c1 + 1));
            u[2] = smp10<LAYOUT>(ldh(row, 2 * c2)); v[2] = smp10<LAYOUT>(ldh(row, 2 * c2 + 1));
        }
    } else {
        const uint8_t* ru = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        const uint8_t* rv = a.plane[f][2] + (int64_t)r * a.pitch[f][2];
        if (VEC) {                                                   // c0 even: a 4-byte load of (c0, c0 + 1), then c2
            const uint32_t wu = ld32(ru + 2 * c0), wv = ld32(rv + 2 * c0);
            u[0] = smp10<LAYOUT>(wu); u[1] = smp10<LAYOUT>(wu >> 16); v[0] = smp10<LAYOUT>(wv); v[1] = smp10<LAYOUT>(wv >> 16);
        } else {
            u[0] = smp10<LAYOUT>(ldh(ru, c0)); u[1] = smp10<LAYOUT>(ldh(ru, c1)); v[0] = smp10<LAYOUT>(ldh(rv, c0)); v[1] = smp10<LAYOUT>(ldh(rv, c1));
        }
        u[2] = smp10<LAYOUT>(ldh(ru, c2)); v[2] = smp10<LAYOUT>(ldh(rv, c2));
    }
}

template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void yuv420_to_planar_pair10_kernel(InArgs16 a) {
    const int x0 = 4 * (blockIdx.x * VK_TX + threadIdx.x);
    const int y = blockIdx.y * VK_TY + threadIdx.y;
    const int f = blockIdx.z;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const bool ev = (y & 1) == 0;                                    // vertical taps as the 8-bit kernel
    const int ra = ev ? max((y >> 1) - 1, 0) : (y >> 1);
    const int rb = ev ? (y >> 1) : min((y >> 1) + 1, ch - 1);
    const int wa = ev ? 1 : 3, wb = 4 - wa;
    int ua[3], va[3], ub[3], vb[3];
    load_chroma10<LAYOUT, VEC>(a, f, ra, x0 >> 1, cw, ua, va);
    load_chroma10<LAYOUT, VEC>(a, f, rb, x0 >> 1, cw, ub, vb);
    int yy[4];
    const uint8_t* yrow = a.plane[f][0] + (int64_t)y * a.pitch[f][0];
    if (VEC) {
        const uint2 w = ld64(yrow + 2 * x0);
        yy[0] = smp10<LAYOUT>(w.x); yy[1] = smp10<LAYOUT>(w.x >> 16); yy[2] = smp10<LAYOUT>(w.y); yy[3] = smp10<LAYOUT>(w.y >> 16);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) yy[j] = smp10<LAYOUT>(ldh(yrow, min(x0 + j, W - 1)));
    }
    const YuvCoeffs& k = a.k;
    int bb[4], gg[4], rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ia = j >> 1, ib = (j + 1) >> 1;
        const int hu_a = ua[ia] + ua[ib], hu_b = ub[ia] + ub[ib];
        const int hv_a = va[ia] + va[ib], hv_b = vb[ia] + vb[ib];
        const int cu = wa * hu_a + wb * hu_b - 8 * VK_MID10;
        const int cv = wa * hv_a + wb * hv_b - 8 * VK_MID10;
        const int yv = (yy[j] - k.yoff) * 8 * k.ky;
        rr[j] = clamp10((yv + k.krv * cv + (1 << 18)) >> 19);
        gg[j] = clamp10((yv - k.kgu * cu - k.kgv * cv + (1 << 18)) >> 19);
        bb[j] = clamp10((yv + k.kbu * cu + (1 << 18)) >> 19);
    }
    const int64_t HW = (int64_t)H * W;
    uint16_t* d = a.dst + (int64_t)f * 3 * HW + (int64_t)y * W + x0;
    if (VEC) {
        *reinterpret_cast<uint2*>(d) = make_uint2(pack2h(bb[0], bb[1]), pack2h(bb[2], bb[3]));
        *reinterpret_cast<uint2*>(d + HW) = make_uint2(pack2h(gg[0], gg[1]), pack2h(gg[2], gg[3]));
        *reinterpret_cast<uint2*>(d + 2 * HW) = make_uint2(pack2h(rr[0], rr[1]), pack2h(rr[2], rr[3]));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) { d[j] = (uint16_t)bb[j]; d[HW + j] = (uint16_t)gg[j]; d[2 * HW + j] = (uint16_t)rr[j]; }
    }
}

static bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

int yuv420_to_planar_pair10(const fldr_video_frame in[2], int layout, const YuvCoeffs& k, uint16_t* pair, int H, int W, hipStream_t stream) {
    InArgs16 a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    bool vec = (W & 3) == 0 && al8(pair);
    for (int f = 0; f < 2; ++f)
        for (int p = 0; p < 3; ++p) {
            a.plane[f][p] = p < np ? (const uint8_t*)in[f].plane[p] : nullptr;
            a.pitch[f][p] = p < np ? in[f].pitch[p] : 0;
            if (p < np) vec = vec && al8(in[f].plane[p]) && (in[f].pitch[p] & 7) == 0;
        }
    a.dst = pair; a.H = H; a.W = W; a.k = k;
    VK_NOTE_PATH(vec);
    const dim3 grid((((W + 3) >> 2) + VK_TX - 1) / VK_TX, (H + VK_TY - 1) / VK_TY, 2), block(VK_TX, VK_TY);
    if (layout == FLDR_VIDEO_NV12) {
        if (vec) hipLaunchKernelGGL((yuv420_to_planar_pair10_kernel<FLDR_VIDEO_NV12, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((yuv420_to_planar_pair10_kernel<FLDR_VIDEO_NV12, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((yuv420_to_planar_pair10_kernel<FLDR_VIDEO_I420, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((yuv420_to_planar_pair10_kernel<FLDR_VIDEO_I420, false>), grid, block, 0, stream, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

struct OutArgs16 {
    const uint16_t* src;         // [3][H][W], code values 0 .. 1023
    uint8_t* plane[3];
    int64_t pitch[3];            // bytes
    int H, W;
    YuvCoeffs k;
};

// Pixels x0 - 1 .. x0 + 3 (clamped into the row) of one row of one plane: px[0..4].
template <bool VEC>
__device__ __forceinline__ void load_px10(const uint16_t* row, int x0, int W, int* px) {
    px[0] = row[max(x0 - 1, 0)];
    if (VEC) {
        const uint2 w = *reinterpret_cast<const uint2*>(row + x0);
        px[1] = (int)(w.x & 0xffffu); px[2] = (int)(w.x >> 16); px[3] = (int)(w.y & 0xffffu); px[4] = (int)(w.y >> 16);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[1 + j] = row[min(x0 + j, W - 1)];
    }
}

template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void planar_to_yuv420_10_kernel(OutArgs16 a) {
    const int x0 = 4 * (blockIdx.x * VK_TX + threadIdx.x);
    const int cj = blockIdx.y * VK_TY + threadIdx.y;                 // chroma row: luma rows 2 cj, 2 cj + 1 (clamped)
    const int H = a.H, W = a.W;
    if (x0 >= W || 2 * cj >= H) return;
    const int cw = (W + 1) >> 1;
    const int64_t HW = (int64_t)H * W;
    const YuvCoeffs& k = a.k;
    int up[5], vp[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) up[m] = vp[m] = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int y = min(2 * cj + h, H - 1);
        int b[5], g[5], r[5];
        const uint16_t* s = a.src + (int64_t)y * W;
        load_px10<VEC>(s, x0, W, b);
        load_px10<VEC>(s + HW, x0, W, g);
        load_px10<VEC>(s + 2 * HW, x0, W, r);
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            up[m] += k.kur * r[m] + k.kug * g[m] + k.kub * b[m];
            vp[m] += k.kvr * r[m] + k.kvg * g[m] + k.kvb * b[m];
        }
        if (2 * cj + h >= H) continue;                               // odd H: the last chroma row has one luma row
        int yb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            yb[j] = word10<LAYOUT>(min(((k.kyr * r[1 + j] + k.kyg * g[1 + j] + k.kyb * b[1 + j] + (1 << 15)) >> 16) + k.yoff, VK_MAX10));
        uint8_t* yrow = a.plane[0] + (int64_t)y * a.pitch[0] + 2 * x0;
        if (VEC) {
            *reinterpret_cast<uint2*>(yrow) = make_uint2(pack2h(yb[0], yb[1]), pack2h(yb[2], yb[3]));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) reinterpret_cast<uint16_t*>(yrow)[j] = (uint16_t)yb[j];
        }
    }
    const int i0 = x0 >> 1;
    const int u0 = word10<LAYOUT>(clamp10(((up[0] + 2 * up[1] + up[2] + (1 << 18)) >> 19) + VK_MID10));
    const int v0 = word10<LAYOUT>(clamp10(((vp[0] + 2 * vp[1] + vp[2] + (1 << 18)) >> 19) + VK_MID10));
    const int u1 = word10<LAYOUT>(clamp10(((up[2] + 2 * up[3] + up[4] + (1 << 18)) >> 19) + VK_MID10));
    const int v1 = word10<LAYOUT>(clamp10(((vp[2] + 2 * vp[3] + vp[4] + (1 << 18)) >> 19) + VK_MID10));
    const bool has1 = i0 + 1 < cw;
    if (LAYOUT == FLDR_VIDEO_NV12) {
        uint16_t* row = reinterpret_cast<uint16_t*>(a.plane[1] + (int64_t)cj * a.pitch[1]) + 2 * i0;
        if (VEC) {                                                   // W % 4 == 0: both columns exist; i0 even: 8-byte aligned
            *reinterpret_cast<uint2*>(row) = make_uint2(pack2h(u0, v0), pack2h(u1, v1));
        } else {
            row[0] = (uint16_t)u0; row[1] = (uint16_t)v0;
            if (has1) { row[2] = (uint16_t)u1; row[3] = (uint16_t)v1; }
        }
    } else {
        uint16_t* ru = reinterpret_cast<uint16_t*>(a.plane[1] + (int64_t)cj * a.pitch[1]) + i0;
        uint16_t* rv = reinterpret_cast<uint16_t*>(a.plane[2] + (int64_t)cj * a.pitch[2]) + i0;
        if (VEC) {                                                   // i0 even: 4-byte aligned
            *reinterpret_cast<uint32_t*>(ru) = pack2h(u0, u1);
            *reinterpret_cast<uint32_t*>(rv) = pack2h(v0, v1);
        } else {
            ru[0] = (uint16_t)u0; rv[0] = (uint16_t)v0;
            if (has1) { ru[1] = (uint16_t)u1; rv[1] = (uint16_t)v1; }
        }
    }
}

int planar_to_yuv420_10(const uint16_t* planar, const fldr_video_frame& out, int layout, const YuvCoeffs& k, int H, int W, hipStream_t stream) {
    OutArgs16 a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    bool vec = (W & 3) == 0 && al8(planar);
    for (int p = 0; p < 3; ++p) {
        a.plane[p] = p < np ? (uint8_t*)out.plane[p] : nullptr;
        a.pitch[p] = p < np ? out.pitch[p] : 0;
        if (p < np) vec = vec && al8(out.plane[p]) && (out.pitch[p] & 7) == 0;
    }
    a.src = planar; a.H = H; a.W = W; a.k = k;
    VK_NOTE_PATH(vec);
    const int ch = (H + 1) >> 1;
    const dim3 grid((((W + 3) >> 2) + VK_TX - 1) / VK_TX, (ch + VK_TY - 1) / VK_TY, 1), block(VK_TX, VK_TY);
    if (layout == FLDR_VIDEO_NV12) {
        if (vec) hipLaunchKernelGGL((planar_to_yuv420_10_kernel<FLDR_VIDEO_NV12, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((planar_to_yuv420_10_kernel<FLDR_VIDEO_NV12, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((planar_to_yuv420_10_kernel<FLDR_VIDEO_I420, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((planar_to_yuv420_10_kernel<FLDR_VIDEO_I420, false>), grid, block, 0, stream, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace fldr_video_impl
