// The kernels of libfldr_pack10.so: the packed 10-bit containers v210 (4:2:2, six pixels per 16-byte group), Y210 (4:2:2, 16-bit words
// Y0 U Y1 V, value high) and Y410 (4:4:4, one dword per pixel) on either side of the model's planar 10-bit BGR forward.  One input kernel
// and one output kernel, templated on the container.  All are bandwidth kernels: a thread owns a run of luma pixels along one row (one
// group = 6 for v210, 8 for Y210 / Y410); 4:2:2 has no vertical taps, so rows are independent.  Two forms of each:
//   VEC      wide accesses.  v210: the plane and its pitch are 16-byte aligned, the planar BGR pointer is 4-byte aligned and W is even: a
//            lane moves its group as 16 bytes and its six pixels of each BGR plane as 12 (three dwords), so the lanes of a wave touch
//            1024 contiguous bytes of v210 and 768 of each plane per instruction.  Y210 / Y410: the plane, its pitch and the planar BGR
//            pointer are 16-byte aligned and W % 8 == 0: two 16-byte accesses of the container and one per BGR plane;
//   !VEC     the same arithmetic on single words (dwords of v210 / Y410, 16-bit words of Y210 and BGR), indices clamped into the row and
//            the stores guarded.
// A v210 row is whole groups in memory whatever W is, so the v210 side of the VEC form is 16 bytes per group everywhere; only the planar
// side has a row end, and only the lane whose group holds it (6 g + 6 > W, one lane per row) takes the guarded per-sample accesses
// there.  W % 6 is no condition of the wide form.
// The arithmetic is the colour definition of ../video/yuv_color.h in int32 at depth 10, exactly as tests/yuv_chroma_oracle.py states it
// for yuv422p10le / yuv444p10le.  Written with h = 2 C for 4:4:4 (to BGR) and s = 8 p (from BGR), the 4:4:4 forms are the 4:2:2
// expressions: (8 p + 2^18) >> 19 = (p + 2^15) >> 16.
// The 32-bit words of v210 and Y410 are built as a | b << 10 | c << 20 from three clamped int32 values (v_lshl_or_b32 / v_or3_b32): whole
// dwords, never half-word packing, so none of the instructions ../video/yuv_run_device.h warns of can appear; 16-bit halves (Y210, BGR)
// go through its pack2h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/yuv_run_device.h"
#include "pack10_internal.h"

namespace fldr_pack10_impl {

#define PK_TX 64                 // threads along a row
#define PK_TY 4                  // rows per block

using namespace fldr_yuv_run;                      // Smp, ld_wide / st_wide, load_run / store_run, load_words / store_words, pack2h;
                                                   // al, row_grid, YUV_LAUNCH_VEC, launched

typedef uint16_t T;                                // a planar BGR sample
constexpr int MID = Smp<T>::MID, MAXV = Smp<T>::MAXV;

template <int C> constexpr int RUN = C == FLDR_PACK10_V210 ? RUN_V210 : RUN_WORDS;

__device__ __forceinline__ int f0(uint32_t w) { return (int)(w & 0x3ffu); }            // the three 10-bit fields of a dword
__device__ __forceinline__ int f1(uint32_t w) { return (int)((w >> 10) & 0x3ffu); }
__device__ __forceinline__ int f2(uint32_t w) { return (int)((w >> 20) & 0x3ffu); }
// three values 0 .. 1023 -> one dword, a lowest; bits 30-31 zero
__device__ __forceinline__ uint32_t word3(int a, int b, int c) { return (uint32_t)a | ((uint32_t)b << 10) | ((uint32_t)c << 20); }

// a 16-byte group of v210, as one access or as four dwords
template <bool VEC> __device__ __forceinline__ void ld_group(const uint8_t* p, uint32_t* w) {
    if (VEC) {
        ld_wide<16>(p, w);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    }
}
template <bool VEC> __device__ __forceinline__ void st_group(uint8_t* p, const uint32_t* w) {
    if (VEC) {
        st_wide<16>(p, w);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) reinterpret_cast<uint32_t*>(p)[i] = w[i];
    }
}

// six 16-bit samples of a planar row (the pixels of one v210 group) at a 4-byte aligned address, as one 12-byte access
struct alignas(4) Dword3 { uint32_t a, b, c; };
__device__ __forceinline__ void ld_six(const uint8_t* p, int* s) {
    const Dword3 v = *reinterpret_cast<const Dword3*>(p);
    const uint32_t w[3] = {v.a, v.b, v.c};
    unpack<T, 6>(w, s);
}
__device__ __forceinline__ void st_six(uint8_t* p, const int* s) {
    Dword3 v;
    v.a = pack2h(s[0], s[1]); v.b = pack2h(s[2], s[3]); v.c = pack2h(s[4], s[5]);
    *reinterpret_cast<Dword3*>(p) = v;
}

// ---- (a) frames -> planar BGR ----------------------------------------------------------------------------------------------------
struct InArgs {
    const uint8_t* plane[MAX_FRAMES];
    int64_t pitch[MAX_FRAMES];       // bytes
    uint8_t* dst;                    // [n][3][H][W] of T
    int H, W;
    YuvCoeffs k;
};

template <int C, bool VEC>
__global__ __launch_bounds__(PK_TX * PK_TY) void pack10_to_planar_kernel(InArgs a) {
    constexpr int R = RUN<C>;
    constexpr bool FULL = C == FLDR_PACK10_Y410;
    constexpr int NC = FULL ? R : R / 2;                             // chroma samples under the run
    const int x0 = R * (blockIdx.x * PK_TX + threadIdx.x);
    const int y = blockIdx.y * PK_TY + threadIdx.y;
    const int f = blockIdx.z;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int cw = FULL ? W : (W + 1) >> 1;
    const int c0 = FULL ? x0 : x0 >> 1;
    // the whole run lies in the row: the planar side may take the wide form (always so where VEC is a property of W: Y210, Y410)
    const bool whole = C == FLDR_PACK10_V210 ? x0 + R <= W : true;
    int yy[R], u[NC + 1], v[NC + 1];
    const uint8_t* row0 = a.plane[f] + (int64_t)y * a.pitch[f];
    if constexpr (C == FLDR_PACK10_V210) {
        const uint8_t* grp = row0 + (int64_t)(x0 / 6) * 16;          // x0 < W: the group is in the row
        uint32_t w[4];
        ld_group<VEC>(grp, w);
        u[0] = f0(w[0]);  yy[0] = f1(w[0]); v[0] = f2(w[0]);
        yy[1] = f0(w[1]); u[1] = f1(w[1]);  yy[2] = f2(w[1]);
        v[1] = f0(w[2]);  yy[3] = f1(w[2]); u[2] = f2(w[2]);
        yy[4] = f0(w[3]); v[2] = f1(w[3]);  yy[5] = f2(w[3]);
        // the chroma sample right of the group: U0, V0 of the next group, or the group's last when the row's chroma ends with it
        if (c0 + NC < cw) {
            const uint32_t n = *reinterpret_cast<const uint32_t*>(grp + 16);
            u[NC] = f0(n); v[NC] = f2(n);
        } else {
            u[NC] = u[NC - 1]; v[NC] = v[NC - 1];
        }
        if (!whole) {
            // the group holds the row's end: every chroma sample past the row's last (a spare slot) becomes the last
#pragma unroll
            for (int i = 1; i <= NC; ++i)
                if (c0 + i >= cw) { u[i] = u[i - 1]; v[i] = v[i - 1]; }
        }
    } else if constexpr (C == FLDR_PACK10_Y210) {
        int m[NC * 4];
        load_run<uint16_t, NC, 4, VEC>(row0, c0, cw, m);
#pragma unroll
        for (int i = 0; i < NC; ++i) { yy[2 * i] = m[4 * i] >> 6; u[i] = m[4 * i + 1] >> 6; yy[2 * i + 1] = m[4 * i + 2] >> 6; v[i] = m[4 * i + 3] >> 6; }
        const int ce = min(c0 + NC, cw - 1);                         // the chroma sample right of the run (clamped)
        u[NC] = reinterpret_cast<const uint16_t*>(row0)[4 * ce + 1] >> 6;
        v[NC] = reinterpret_cast<const uint16_t*>(row0)[4 * ce + 3] >> 6;
    } else {
        uint32_t w[R];
        if (VEC) {
            load_words<R, true>(row0, x0, W, w);
        } else {                                     // in the kernel: DESIGN_LOG.md ("Chroma, pack10 and rgb", device code)
#pragma unroll
            for (int j = 0; j < R; ++j) w[j] = reinterpret_cast<const uint32_t*>(row0)[min(x0 + j, W - 1)];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) { u[j] = f0(w[j]); yy[j] = f1(w[j]); v[j] = f2(w[j]); }
    }
    const YuvCoeffs& k = a.k;
    int bb[R], gg[R], rr[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        // h = C[ca] + C[cb]: even x -> both its own column, odd x -> the columns left and right of it (the right one clamped); x0 is even
        const int ia = FULL ? j : j >> 1, ib = FULL ? j : (j + 1) >> 1;
        const int cu = 4 * (u[ia] + u[ib]) - 8 * MID;
        const int cv = 4 * (v[ia] + v[ib]) - 8 * MID;
        const int yv = (yy[j] - k.yoff) * 8 * k.ky;
        rr[j] = min(max((yv + k.krv * cv + (1 << 18)) >> 19, 0), MAXV);
        gg[j] = min(max((yv - k.kgu * cu - k.kgv * cv + (1 << 18)) >> 19, 0), MAXV);
        bb[j] = min(max((yv + k.kbu * cu + (1 << 18)) >> 19, 0), MAXV);
    }
    const int64_t HW = (int64_t)H * W;
    uint8_t* d = a.dst + ((int64_t)f * 3 * HW + (int64_t)y * W) * (int64_t)sizeof(T);
    const int64_t plane_bytes = HW * (int64_t)sizeof(T);
    if constexpr (C == FLDR_PACK10_V210) {
        if (VEC && whole) {
            uint8_t* p = d + (int64_t)x0 * (int64_t)sizeof(T);
            st_six(p, bb); st_six(p + plane_bytes, gg); st_six(p + 2 * plane_bytes, rr);
        } else {
            store_run<T, R, 1, false>(d, x0, W, bb);
            store_run<T, R, 1, false>(d + plane_bytes, x0, W, gg);
            store_run<T, R, 1, false>(d + 2 * plane_bytes, x0, W, rr);
        }
    } else {
        store_run<T, R, 1, VEC>(d, x0, W, bb);
        store_run<T, R, 1, VEC>(d + plane_bytes, x0, W, gg);
        store_run<T, R, 1, VEC>(d + 2 * plane_bytes, x0, W, rr);
    }
}

// ---- (b) planar BGR frame -> frame -------------------------------------------------------------------------------------------------
struct OutArgs {
    const uint8_t* src;              // [3][H][W] of T
    uint8_t* plane;
    int64_t pitch;                   // bytes
    int H, W;
    YuvCoeffs k;
};

template <int C, bool VEC>
__global__ __launch_bounds__(PK_TX * PK_TY) void pack10_from_planar_kernel(OutArgs a) {
    constexpr int R = RUN<C>;
    constexpr bool FULL = C == FLDR_PACK10_Y410;
    constexpr int NC = FULL ? R : R / 2;
    const int x0 = R * (blockIdx.x * PK_TX + threadIdx.x);
    const int y = blockIdx.y * PK_TY + threadIdx.y;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int cw = FULL ? W : (W + 1) >> 1;
    const int c0 = FULL ? x0 : x0 >> 1;
    const bool whole = C == FLDR_PACK10_V210 ? x0 + R <= W : true;
    const int64_t HW = (int64_t)H * W;
    const YuvCoeffs& k = a.k;
    // pixels x0 - 1 .. x0 + R - 1 (clamped into the row) of the three planes: px[c][0 .. R]; the left neighbour only feeds 4:2:2 chroma
    int px[3][R + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* row = a.src + ((int64_t)c * HW + (int64_t)y * W) * (int64_t)sizeof(T);
        px[c][0] = FULL ? 0 : (int)reinterpret_cast<const T*>(row)[max(x0 - 1, 0)];
        if constexpr (C == FLDR_PACK10_V210) {
            if (VEC && whole) ld_six(row + (int64_t)x0 * (int64_t)sizeof(T), px[c] + 1);
            else load_run<T, R, 1, false>(row, x0, W, px[c] + 1);
        } else {
            load_run<T, R, 1, VEC>(row, x0, W, px[c] + 1);
        }
    }
    int yb[R], pu[R + 1], pv[R + 1];
#pragma unroll
    for (int m = 0; m <= R; ++m) {
        const int b = px[0][m], g = px[1][m], r = px[2][m];
        pu[m] = k.kur * r + k.kug * g + k.kub * b;
        pv[m] = k.kvr * r + k.kvg * g + k.kvb * b;
        if (m) yb[m - 1] = min(max(((k.kyr * r + k.kyg * g + k.kyb * b + (1 << 15)) >> 16) + k.yoff, 0), MAXV);
    }
    int uo[NC], vo[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        // 4:2:2: chroma column c0 + i takes luma x0 + 2 i - 1, x0 + 2 i, x0 + 2 i + 1 weighted 1, 2, 1 (twice: the weights sum to 8)
        const int su = FULL ? 8 * pu[i + 1] : 2 * (pu[2 * i] + 2 * pu[2 * i + 1] + pu[2 * i + 2]);
        const int sv = FULL ? 8 * pv[i + 1] : 2 * (pv[2 * i] + 2 * pv[2 * i + 1] + pv[2 * i + 2]);
        uo[i] = min(max(((su + (1 << 18)) >> 19) + MID, 0), MAXV);
        vo[i] = min(max(((sv + (1 << 18)) >> 19) + MID, 0), MAXV);
    }
    uint8_t* row0 = a.plane + (int64_t)y * a.pitch;
    if constexpr (C == FLDR_PACK10_V210) {
        // The group is written whole.  In the row's last group the spare luma slots are copies of luma W - 1 already (the pixels were read
        // clamped); the spare chroma slots become copies of the row's last chroma sample here (c0 < cw: never the group's first).
        if (!whole) {
#pragma unroll
            for (int i = 1; i < NC; ++i)
                if (c0 + i >= cw) { uo[i] = uo[i - 1]; vo[i] = vo[i - 1]; }
        }
        const uint32_t w[4] = {word3(uo[0], yb[0], vo[0]), word3(yb[1], uo[1], yb[2]), word3(vo[1], yb[3], uo[2]), word3(yb[4], vo[2], yb[5])};
        st_group<VEC>(row0 + (int64_t)(x0 / 6) * 16, w);
    } else if constexpr (C == FLDR_PACK10_Y210) {
        // odd W: the run's last pixel was read clamped, so the second luma word of the last group is a copy of the last luma sample
        int m[NC * 4];
#pragma unroll
        for (int i = 0; i < NC; ++i) { m[4 * i] = yb[2 * i] << 6; m[4 * i + 1] = uo[i] << 6; m[4 * i + 2] = yb[2 * i + 1] << 6; m[4 * i + 3] = vo[i] << 6; }
        store_run<uint16_t, NC, 4, VEC>(row0, c0, cw, m);
    } else {
        uint32_t w[R];
#pragma unroll
        for (int j = 0; j < R; ++j) w[j] = word3(uo[j], yb[j], vo[j]) | 0xc0000000u;            // alpha = 3
        if (VEC) {
            store_words<R, true>(row0, x0, W, w);
        } else {                                     // in the kernel, like the input kernel's loads
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (x0 + j < W) reinterpret_cast<uint32_t*>(row0)[x0 + j] = w[j];
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// what the wide form asks of the planar BGR side: v210 moves 12 bytes per lane (a 4-byte aligned start of every row), the others 16
static bool planar_wide(const fldr_pack10_format& fmt, const void* planar, int W) {
    return fmt.container == FLDR_PACK10_V210 ? W % 2 == 0 && al(planar, 4) : W % 8 == 0 && al(planar, 16);
}

// Call GO(C) for the container of `fmt` (the caller checked the format).
#define PK_DISPATCH(fmt)                                                   \
    do {                                                                   \
        if ((fmt).container == FLDR_PACK10_V210) GO(FLDR_PACK10_V210);     \
        else if ((fmt).container == FLDR_PACK10_Y210) GO(FLDR_PACK10_Y210); \
        else GO(FLDR_PACK10_Y410);                                         \
    } while (0)

int to_planar(const fldr_pack10_frame* in, int n, const fldr_pack10_format& fmt, const YuvCoeffs& k, void* planar, int H, int W, hipStream_t stream) {
    InArgs a;
    bool vec = planar_wide(fmt, planar, W);
    for (int f = 0; f < MAX_FRAMES; ++f) {
        a.plane[f] = f < n ? (const uint8_t*)in[f].plane[0] : nullptr;
        a.pitch[f] = f < n ? in[f].pitch[0] : 0;
        if (f < n) vec = vec && al(in[f].plane[0], 16) && al(in[f].pitch[0], 16);
    }
    a.dst = (uint8_t*)planar; a.H = H; a.W = W; a.k = k;
    const dim3 block(PK_TX, PK_TY);
#define GO(C) YUV_LAUNCH_VEC(pack10_to_planar_kernel, vec, (row_grid<PK_TX, PK_TY>(RUN<C>, H, W, n)), block, stream, a, C)
    PK_DISPATCH(fmt);
#undef GO
    return launched();
}

int from_planar(const void* planar, const fldr_pack10_frame& out, const fldr_pack10_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream) {
    OutArgs a;
    const bool vec = planar_wide(fmt, planar, W) && al(out.plane[0], 16) && al(out.pitch[0], 16);
    a.src = (const uint8_t*)planar; a.plane = (uint8_t*)out.plane[0]; a.pitch = out.pitch[0]; a.H = H; a.W = W; a.k = k;
    const dim3 block(PK_TX, PK_TY);
#define GO(C) YUV_LAUNCH_VEC(pack10_from_planar_kernel, vec, (row_grid<PK_TX, PK_TY>(RUN<C>, H, W, 1)), block, stream, a, C)
    PK_DISPATCH(fmt);
#undef GO
    return launched();
}

}  // namespace fldr_pack10_impl
