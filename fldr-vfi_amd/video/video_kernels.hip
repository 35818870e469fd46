// The two kernels of libfldr_video.so: YUV 4:2:0 (NV12 / I420, pitched planes) on either side of the model's planar BGR forward, templated
// on the sample type: bytes at depth 8; at depth 10 little-endian 16-bit words (pitches stay in bytes), where FLDR_VIDEO_NV12 is P010 (the
// value in the high 10 bits) and FLDR_VIDEO_I420 is yuv420p10le (the value in the low 10 bits), and the model's side is planar uint16 BGR,
// code values 0 .. 1023.  Both are bandwidth kernels.  A thread owns 4 luma pixels along a row (the input kernel: one row; the output
// kernel: the two rows of one chroma row), so rows are read and written with one 4-sample access per lane (4 bytes at depth 8, 8 at
// depth 10) when every plane pointer and pitch is aligned to that and W is a multiple of 4 (VEC); otherwise the same arithmetic runs on
// single-sample accesses with the indices clamped to the row.  The arithmetic is the colour definition of yuv_color.h, in int32, exactly
// as tests/yuv_oracle.py states it: the same taps, 16 fraction bits and shifts at both depths; the chroma centre and the clamps are those
// of the sample type (Smp), the coefficients YUV_COEFFS or YUV_COEFFS_10.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "video_internal.h"
#include "yuv_run_device.h"

namespace fldr_video_impl {

using namespace fldr_yuv_run;    // Smp, load_run / store_run, dec / enc

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

template <typename T> __device__ __forceinline__ int clamp_smp(int v) { return min(max(v, 0), Smp<T>::MAXV); }

// ---- (a) two YUV 4:2:0 frames -> planar BGR pair ---------------------------------------------------------------------------------
struct InArgs {
    const uint8_t* plane[2][3];
    int64_t pitch[2][3];         // bytes
    uint8_t* dst;                // [2][3][H][W] of T
    int H, W;
    YuvCoeffs k;
};

// Chroma samples c0 = x0/2, c1, c2 (clamped into the row) of one chroma row: u[0..2], v[0..2].
template <typename T, int LAYOUT, bool VEC>
__device__ __forceinline__ void load_chroma(const InArgs& a, int f, int r, int c0, int cw, int* u, int* v) {
    constexpr bool HI = LAYOUT == FLDR_VIDEO_NV12;
    const int c1 = min(c0 + 1, cw - 1), c2 = min(c0 + 2, cw - 1);
    if (LAYOUT == FLDR_VIDEO_NV12) {
        const uint8_t* row = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        int m[6];
        if (VEC) {                                                   // c1 = c0 + 1 (W % 4 == 0): U, V, U, V in one access, then U, V of c2
            constexpr int PB = 2 * (int)sizeof(T), ND = 2 * PB / 4;  // bytes of a U, V pair; dwords of two pairs
            uint32_t w[ND + 1];
            ld_wide<2 * PB>(row + c0 * PB, w);
            if (c2 > c1) ld_wide<PB>(row + c0 * PB + 2 * PB, w + ND);  // c2 = c0 + 2
            else w[ND] = w[ND - 1] >> (32 - 8 * PB);                 // the row ends with this run: c2 is c1 again
            // the pair of c2 fills the low end of its own dword: samples 4, 5.  Unpacked after the merge, not on either side of it, so
            // that the samples' range is still known where they are multiplied (24-bit multiplies)
            unpack<T, 6>(w, m);
        } else {
            load_run<T, 3, 2, false>(row, c0, cw, m);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { u[i] = dec<T, HI>(m[2 * i]); v[i] = dec<T, HI>(m[2 * i + 1]); }
    } else {
        const uint8_t* ru = a.plane[f][1] + (int64_t)r * a.pitch[f][1];
        const uint8_t* rv = a.plane[f][2] + (int64_t)r * a.pitch[f][2];
        load_run<T, 2, 1, VEC>(ru, c0, cw, u);                       // VEC: c0 even: one half-width access of (c0, c0 + 1)
        load_run<T, 2, 1, VEC>(rv, c0, cw, v);
        u[2] = reinterpret_cast<const T*>(ru)[c2]; v[2] = reinterpret_cast<const T*>(rv)[c2];
#pragma unroll
        for (int i = 0; i < 3; ++i) { u[i] = dec<T, HI>(u[i]); v[i] = dec<T, HI>(v[i]); }
    }
}

template <typename T, int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void yuv420_to_planar_pair_kernel(InArgs a) {
    constexpr int MID = Smp<T>::MID;
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
    load_chroma<T, LAYOUT, VEC>(a, f, ra, x0 >> 1, cw, ua, va);
    load_chroma<T, LAYOUT, VEC>(a, f, rb, x0 >> 1, cw, ub, vb);
    int yy[4];
    load_run<T, 4, 1, VEC>(a.plane[f][0] + (int64_t)y * a.pitch[f][0], x0, W, yy);
    const YuvCoeffs& k = a.k;
    int bb[4], gg[4], rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // horizontal taps of pixel x0 + j: 2 on column c0 + j/2 (even), 1 + 1 on c0 + (j-1)/2 and c0 + (j+1)/2 (odd; clamped)
        const int ia = j >> 1, ib = (j + 1) >> 1;
        const int hu_a = ua[ia] + ua[ib], hu_b = ub[ia] + ub[ib];
        const int hv_a = va[ia] + va[ib], hv_b = vb[ia] + vb[ib];
        const int cu = wa * hu_a + wb * hu_b - 8 * MID;
        const int cv = wa * hv_a + wb * hv_b - 8 * MID;
        const int yv = (dec<T, LAYOUT == FLDR_VIDEO_NV12>(yy[j]) - k.yoff) * 8 * k.ky;
        rr[j] = clamp_smp<T>((yv + k.krv * cv + (1 << 18)) >> 19);
        gg[j] = clamp_smp<T>((yv - k.kgu * cu - k.kgv * cv + (1 << 18)) >> 19);
        bb[j] = clamp_smp<T>((yv + k.kbu * cu + (1 << 18)) >> 19);
    }
    const int64_t HW = (int64_t)H * W;
    T* d = reinterpret_cast<T*>(a.dst) + (int64_t)f * 3 * HW + (int64_t)y * W + x0;     // the run's first sample: group 0 of W - x0
    store_run<T, 4, 1, VEC>(reinterpret_cast<uint8_t*>(d), 0, W - x0, bb);
    store_run<T, 4, 1, VEC>(reinterpret_cast<uint8_t*>(d + HW), 0, W - x0, gg);
    store_run<T, 4, 1, VEC>(reinterpret_cast<uint8_t*>(d + 2 * HW), 0, W - x0, rr);
}

// ---- (b) planar BGR frame -> YUV 4:2:0 -----------------------------------------------------------------------------------------
struct OutArgs {
    const uint8_t* src;          // [3][H][W] of T
    uint8_t* plane[3];
    int64_t pitch[3];            // bytes
    int H, W;
    YuvCoeffs k;
};

template <typename T, int LAYOUT, bool VEC>
__global__ __launch_bounds__(VK_TX * VK_TY) void planar_to_yuv420_kernel(OutArgs a) {
    constexpr int MID = Smp<T>::MID, MAXV = Smp<T>::MAXV;
    constexpr bool HI = LAYOUT == FLDR_VIDEO_NV12;
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
        // pixels x0 - 1 .. x0 + 3 (clamped into the row) of row y of the three planes: px[c][0..4]
        int px[3][5];
        const T* s = reinterpret_cast<const T*>(a.src) + (int64_t)y * W + x0;         // the run's first sample: group 0 of W - x0
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            px[c][0] = s[c * HW - (x0 > 0)];                         // the left neighbour; at the row's start the pixel itself
            load_run<T, 4, 1, VEC>(reinterpret_cast<const uint8_t*>(s + c * HW), 0, W - x0, px[c] + 1);
        }
        const int *b = px[0], *g = px[1], *r = px[2];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            up[m] += k.kur * r[m] + k.kug * g[m] + k.kub * b[m];
            vp[m] += k.kvr * r[m] + k.kvg * g[m] + k.kvb * b[m];
        }
        if (2 * cj + h >= H) continue;                               // odd H: the last chroma row has one luma row
        int yb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            yb[j] = enc<T, HI>(min(((k.kyr * r[1 + j] + k.kyg * g[1 + j] + k.kyb * b[1 + j] + (1 << 15)) >> 16) + k.yoff, MAXV));
        store_run<T, 4, 1, VEC>(a.plane[0] + (int64_t)y * a.pitch[0], x0, W, yb);
    }
    // chroma columns i0 = x0/2 (luma x0 - 1, x0, x0 + 1 weighted 1, 2, 1) and i0 + 1 (x0 + 1, x0 + 2, x0 + 3): uo[0..1], vo[0..1]
    const int i0 = x0 >> 1;
    int uo[2], vo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        uo[i] = enc<T, HI>(clamp_smp<T>(((up[2 * i] + 2 * up[2 * i + 1] + up[2 * i + 2] + (1 << 18)) >> 19) + MID));
        vo[i] = enc<T, HI>(clamp_smp<T>(((vp[2 * i] + 2 * vp[2 * i + 1] + vp[2 * i + 2] + (1 << 18)) >> 19) + MID));
    }
    // VEC: W % 4 == 0, so both columns exist, and i0 is even, so the access is aligned; !VEC: column i0 + 1 only when it is below cw
    if (LAYOUT == FLDR_VIDEO_NV12) {
        const int m[4] = { uo[0], vo[0], uo[1], vo[1] };
        store_run<T, 2, 2, VEC>(a.plane[1] + (int64_t)cj * a.pitch[1], i0, cw, m);
    } else {
        store_run<T, 2, 1, VEC>(a.plane[1] + (int64_t)cj * a.pitch[1], i0, cw, uo);
        store_run<T, 2, 1, VEC>(a.plane[2] + (int64_t)cj * a.pitch[2], i0, cw, vo);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// KERNEL<T, layout, vec><<<grid, block, 0, stream>>>(a)
#define VK_LAUNCH(KERNEL, T, layout, vec, grid, block, stream, a)                                          \
    do {                                                                                                   \
        if ((layout) == FLDR_VIDEO_NV12) YUV_LAUNCH_VEC(KERNEL, vec, grid, block, stream, a, T, FLDR_VIDEO_NV12); \
        else YUV_LAUNCH_VEC(KERNEL, vec, grid, block, stream, a, T, FLDR_VIDEO_I420);                      \
    } while (0)

// VEC needs every pointer and pitch aligned to a lane's 4 samples.  That includes the planar buffer: every caller passes one aligned to
// the workspace alignment (the offsets of the forward's plan; the debug hooks refuse anything else), so testing it changes no path.
template <typename T> static bool al_run(const void* p, int64_t pitch = 0) { return al(p, 4 * sizeof(T)) && al(pitch, 4 * sizeof(T)); }

// -> the launch's error; vec: the form chosen
template <typename T>
static int to_planar_t(const fldr_video_frame in[2], int layout, const YuvCoeffs& k, void* pair, int H, int W, hipStream_t stream, bool& vec) {
    InArgs a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    vec = (W & 3) == 0 && al_run<T>(pair);
    for (int f = 0; f < 2; ++f)
        for (int p = 0; p < 3; ++p) {
            a.plane[f][p] = p < np ? (const uint8_t*)in[f].plane[p] : nullptr;
            a.pitch[f][p] = p < np ? in[f].pitch[p] : 0;
            if (p < np) vec = vec && al_run<T>(in[f].plane[p], in[f].pitch[p]);
        }
    a.dst = (uint8_t*)pair; a.H = H; a.W = W; a.k = k;
    const dim3 grid = row_grid<VK_TX, VK_TY>(4, H, W, 2), block(VK_TX, VK_TY);
    VK_LAUNCH(yuv420_to_planar_pair_kernel, T, layout, vec, grid, block, stream, a);
    return launched();
}

template <typename T>
static int from_planar_t(const void* planar, const fldr_video_frame& out, int layout, const YuvCoeffs& k, int H, int W, hipStream_t stream, bool& vec) {
    OutArgs a;
    const int np = layout == FLDR_VIDEO_NV12 ? 2 : 3;
    vec = (W & 3) == 0 && al_run<T>(planar);
    for (int p = 0; p < 3; ++p) {
        a.plane[p] = p < np ? (uint8_t*)out.plane[p] : nullptr;
        a.pitch[p] = p < np ? out.pitch[p] : 0;
        if (p < np) vec = vec && al_run<T>(out.plane[p], out.pitch[p]);
    }
    a.src = (const uint8_t*)planar; a.H = H; a.W = W; a.k = k;
    const int ch = (H + 1) >> 1;
    const dim3 grid = row_grid<VK_TX, VK_TY>(4, ch, W, 1), block(VK_TX, VK_TY);
    VK_LAUNCH(planar_to_yuv420_kernel, T, layout, vec, grid, block, stream, a);
    return launched();
}

int yuv420_to_planar_pair(const fldr_video_frame in[2], const fldr_video_format& fmt, const YuvCoeffs& k, void* pair, int H, int W, hipStream_t stream) {
    bool vec;
    const int rc = fmt.depth == 10 ? to_planar_t<uint16_t>(in, fmt.layout, k, pair, H, W, stream, vec)
                                   : to_planar_t<uint8_t>(in, fmt.layout, k, pair, H, W, stream, vec);
    VK_NOTE_PATH(vec);
    return rc;
}

int planar_to_yuv420(const void* planar, const fldr_video_frame& out, const fldr_video_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream) {
    bool vec;
    const int rc = fmt.depth == 10 ? from_planar_t<uint16_t>(planar, out, fmt.layout, k, H, W, stream, vec)
                                   : from_planar_t<uint8_t>(planar, out, fmt.layout, k, H, W, stream, vec);
    VK_NOTE_PATH(vec);
    return rc;
}

}  // namespace fldr_video_impl
