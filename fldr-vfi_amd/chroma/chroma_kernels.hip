// The kernels of libfldr_chroma.so: YUV 4:2:2 / 4:4:4 (planar, semiplanar, UYVY / YUYV; 8-bit bytes or 10-bit values in 16-bit words,
// pitched planes) on either side of the model's planar BGR forward.  One input kernel and one output kernel, templated on the sample
// type, the sampling and the layout.  All are bandwidth kernels: a thread owns a run of luma pixels along one row (16 at depth 8, 8 at
// depth 10: 16 bytes of Y and of every BGR plane per lane); 4:2:2 has no vertical taps, so rows are independent.  Two forms of each:
//   VEC      every plane pointer and pitch (and the planar BGR pointer) is 16-byte aligned and W is a multiple of the run: every plane
//            is read and written with one or two 8- or 16-byte accesses per lane (planar 4:2:2 chroma: 8 bytes; everything else 16 or 32);
//   !VEC     the same arithmetic on single samples, with the indices clamped into the row and the stores guarded.
// The arithmetic is the colour definition of ../video/yuv_color.h in int32, exactly as tests/yuv_chroma_oracle.py states it.  Written with
// h = 2 C for 4:4:4 (to BGR) and s = 8 p (from BGR), the 4:4:4 forms are the 4:2:2 expressions: (8 p + 2^18) >> 19 = (p + 2^15) >> 16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/yuv_run_device.h"
#include "chroma_internal.h"

namespace fldr_chroma_impl {

#define CK_TX 64                 // threads along a row
#define CK_TY 4                  // rows per block

using namespace fldr_yuv_run;                      // Smp, load_run / store_run, dec / enc

template <typename T> constexpr int RUN = sizeof(T) == 1 ? RUN8 : RUN16;

// ---- (a) YUV frames -> planar BGR ------------------------------------------------------------------------------------------------
struct InArgs {
    const uint8_t* plane[MAX_FRAMES][3];
    int64_t pitch[MAX_FRAMES][3];    // bytes
    uint8_t* dst;                    // [n][3][H][W] of T
    int H, W;
    YuvCoeffs k;
};

template <typename T, int S, int L, bool VEC>
__global__ __launch_bounds__(CK_TX * CK_TY) void chroma_to_planar_kernel(InArgs a) {
    constexpr int R = RUN<T>, MID = Smp<T>::MID, MAXV = Smp<T>::MAXV;
    constexpr bool FULL = S == FLDR_CHROMA_444, HI = L == FLDR_CHROMA_SEMIPLANAR;   // HI: 16-bit words keep the value high
    constexpr int NC = FULL ? R : R / 2;                             // chroma samples under the run
    const int x0 = R * (blockIdx.x * CK_TX + threadIdx.x);
    const int y = blockIdx.y * CK_TY + threadIdx.y;
    const int f = blockIdx.z;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int cw = FULL ? W : (W + 1) >> 1;
    const int c0 = FULL ? x0 : x0 >> 1;
    const int ce = min(c0 + NC, cw - 1);                             // 4:2:2: the chroma sample right of the run (clamped)
    int yy[R], u[NC + 1], v[NC + 1];
    const uint8_t* row0 = a.plane[f][0] + (int64_t)y * a.pitch[f][0];
    if constexpr (L == FLDR_CHROMA_UYVY || L == FLDR_CHROMA_YUYV) {            // 4:2:2, bytes
        constexpr int YO = L == FLDR_CHROMA_UYVY ? 1 : 0, UO = 1 - YO, VO = UO + 2;
        int m[NC * 4];
        load_run<T, NC, 4, VEC>(row0, c0, cw, m);
#pragma unroll
        for (int i = 0; i < NC; ++i) { yy[2 * i] = m[4 * i + YO]; yy[2 * i + 1] = m[4 * i + YO + 2]; u[i] = m[4 * i + UO]; v[i] = m[4 * i + VO]; }
        u[NC] = row0[4 * ce + UO]; v[NC] = row0[4 * ce + VO];
    } else {
        load_run<T, R, 1, VEC>(row0, x0, W, yy);
#pragma unroll
        for (int j = 0; j < R; ++j) yy[j] = dec<T, HI>(yy[j]);
        const uint8_t* row1 = a.plane[f][1] + (int64_t)y * a.pitch[f][1];
        if constexpr (L == FLDR_CHROMA_SEMIPLANAR) {
            int m[NC * 2];
            load_run<T, NC, 2, VEC>(row1, c0, cw, m);
#pragma unroll
            for (int i = 0; i < NC; ++i) { u[i] = dec<T, HI>(m[2 * i]); v[i] = dec<T, HI>(m[2 * i + 1]); }
            if (!FULL) { u[NC] = dec<T, HI>(reinterpret_cast<const T*>(row1)[2 * ce]); v[NC] = dec<T, HI>(reinterpret_cast<const T*>(row1)[2 * ce + 1]); }
        } else {
            const uint8_t* row2 = a.plane[f][2] + (int64_t)y * a.pitch[f][2];
            load_run<T, NC, 1, VEC>(row1, c0, cw, u);
            load_run<T, NC, 1, VEC>(row2, c0, cw, v);
#pragma unroll
            for (int i = 0; i < NC; ++i) { u[i] = dec<T, HI>(u[i]); v[i] = dec<T, HI>(v[i]); }
            if (!FULL) { u[NC] = dec<T, HI>(reinterpret_cast<const T*>(row1)[ce]); v[NC] = dec<T, HI>(reinterpret_cast<const T*>(row2)[ce]); }
        }
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
    store_run<T, R, 1, VEC>(d, x0, W, bb);
    store_run<T, R, 1, VEC>(d + HW * (int64_t)sizeof(T), x0, W, gg);
    store_run<T, R, 1, VEC>(d + 2 * HW * (int64_t)sizeof(T), x0, W, rr);
}

// ---- (b) planar BGR frame -> YUV frame -----------------------------------------------------------------------------------------
struct OutArgs {
    const uint8_t* src;              // [3][H][W] of T
    uint8_t* plane[3];
    int64_t pitch[3];                // bytes
    int H, W;
    YuvCoeffs k;
};

template <typename T, int S, int L, bool VEC>
__global__ __launch_bounds__(CK_TX * CK_TY) void chroma_from_planar_kernel(OutArgs a) {
    constexpr int R = RUN<T>, MID = Smp<T>::MID, MAXV = Smp<T>::MAXV;
    constexpr bool FULL = S == FLDR_CHROMA_444, HI = L == FLDR_CHROMA_SEMIPLANAR;   // HI: 16-bit words keep the value high
    constexpr int NC = FULL ? R : R / 2;
    const int x0 = R * (blockIdx.x * CK_TX + threadIdx.x);
    const int y = blockIdx.y * CK_TY + threadIdx.y;
    const int H = a.H, W = a.W;
    if (x0 >= W || y >= H) return;
    const int cw = FULL ? W : (W + 1) >> 1;
    const int c0 = FULL ? x0 : x0 >> 1;
    const int64_t HW = (int64_t)H * W;
    const YuvCoeffs& k = a.k;
    // pixels x0 - 1 .. x0 + R - 1 (clamped into the row) of the three planes: px[c][0 .. R]; the left neighbour only feeds 4:2:2 chroma
    int px[3][R + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* row = a.src + ((int64_t)c * HW + (int64_t)y * W) * (int64_t)sizeof(T);
        px[c][0] = FULL ? 0 : (int)reinterpret_cast<const T*>(row)[max(x0 - 1, 0)];
        load_run<T, R, 1, VEC>(row, x0, W, px[c] + 1);
    }
    int yb[R], pu[R + 1], pv[R + 1];
#pragma unroll
    for (int m = 0; m <= R; ++m) {
        const int b = px[0][m], g = px[1][m], r = px[2][m];
        pu[m] = k.kur * r + k.kug * g + k.kub * b;
        pv[m] = k.kvr * r + k.kvg * g + k.kvb * b;
        if (m) yb[m - 1] = enc<T, HI>(min(max(((k.kyr * r + k.kyg * g + k.kyb * b + (1 << 15)) >> 16) + k.yoff, 0), MAXV));
    }
    int uo[NC], vo[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        // 4:2:2: chroma column c0 + i takes luma x0 + 2 i - 1, x0 + 2 i, x0 + 2 i + 1 weighted 1, 2, 1 (twice: the weights sum to 8)
        const int su = FULL ? 8 * pu[i + 1] : 2 * (pu[2 * i] + 2 * pu[2 * i + 1] + pu[2 * i + 2]);
        const int sv = FULL ? 8 * pv[i + 1] : 2 * (pv[2 * i] + 2 * pv[2 * i + 1] + pv[2 * i + 2]);
        uo[i] = enc<T, HI>(min(max(((su + (1 << 18)) >> 19) + MID, 0), MAXV));
        vo[i] = enc<T, HI>(min(max(((sv + (1 << 18)) >> 19) + MID, 0), MAXV));
    }
    uint8_t* row0 = a.plane[0] + (int64_t)y * a.pitch[0];
    if constexpr (L == FLDR_CHROMA_UYVY || L == FLDR_CHROMA_YUYV) {
        // odd W: the run's last pixel was read clamped, so the second luma byte of the last group is a copy of the last luma sample
        constexpr int YO = L == FLDR_CHROMA_UYVY ? 1 : 0, UO = 1 - YO, VO = UO + 2;
        int m[NC * 4];
#pragma unroll
        for (int i = 0; i < NC; ++i) { m[4 * i + YO] = yb[2 * i]; m[4 * i + YO + 2] = yb[2 * i + 1]; m[4 * i + UO] = uo[i]; m[4 * i + VO] = vo[i]; }
        store_run<T, NC, 4, VEC>(row0, c0, cw, m);
    } else {
        store_run<T, R, 1, VEC>(row0, x0, W, yb);
        uint8_t* row1 = a.plane[1] + (int64_t)y * a.pitch[1];
        if constexpr (L == FLDR_CHROMA_SEMIPLANAR) {
            int m[NC * 2];
#pragma unroll
            for (int i = 0; i < NC; ++i) { m[2 * i] = uo[i]; m[2 * i + 1] = vo[i]; }
            store_run<T, NC, 2, VEC>(row1, c0, cw, m);
        } else {
            store_run<T, NC, 1, VEC>(row1, c0, cw, uo);
            store_run<T, NC, 1, VEC>(a.plane[2] + (int64_t)y * a.pitch[2], c0, cw, vo);
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
static int planes_used(int layout) { return layout == FLDR_CHROMA_PLANAR ? 3 : layout == FLDR_CHROMA_SEMIPLANAR ? 2 : 1; }

// Call GO(S, L) for the (sampling, layout) of `fmt`; the packed layouts exist for bytes at 4:2:2 only (the caller checked the format).
#define CK_DISPATCH(T, fmt)                                                                      \
    do {                                                                                         \
        if ((fmt).sampling == FLDR_CHROMA_444) {                                                 \
            if ((fmt).layout == FLDR_CHROMA_PLANAR) GO(FLDR_CHROMA_444, FLDR_CHROMA_PLANAR);     \
            else GO(FLDR_CHROMA_444, FLDR_CHROMA_SEMIPLANAR);                                    \
        } else if ((fmt).layout == FLDR_CHROMA_PLANAR) GO(FLDR_CHROMA_422, FLDR_CHROMA_PLANAR);  \
        else if ((fmt).layout == FLDR_CHROMA_SEMIPLANAR) GO(FLDR_CHROMA_422, FLDR_CHROMA_SEMIPLANAR); \
        else if constexpr (sizeof(T) == 1) {                                                     \
            if ((fmt).layout == FLDR_CHROMA_UYVY) GO(FLDR_CHROMA_422, FLDR_CHROMA_UYVY);         \
            else GO(FLDR_CHROMA_422, FLDR_CHROMA_YUYV);                                          \
        }                                                                                        \
    } while (0)

template <typename T>
static int to_planar_t(const fldr_chroma_frame* in, int n, const fldr_chroma_format& fmt, const YuvCoeffs& k, void* planar, int H, int W,
                       hipStream_t stream) {
    constexpr int R = RUN<T>;
    InArgs a;
    const int np = planes_used(fmt.layout);
    bool vec = W % R == 0 && al(planar, 16);
    for (int f = 0; f < MAX_FRAMES; ++f)
        for (int p = 0; p < 3; ++p) {
            const bool used = f < n && p < np;
            a.plane[f][p] = used ? (const uint8_t*)in[f].plane[p] : nullptr;
            a.pitch[f][p] = used ? in[f].pitch[p] : 0;
            if (used) vec = vec && al(in[f].plane[p], 16) && al(in[f].pitch[p], 16);
        }
    a.dst = (uint8_t*)planar; a.H = H; a.W = W; a.k = k;
    const dim3 grid = row_grid<CK_TX, CK_TY>(R, H, W, n), block(CK_TX, CK_TY);
#define GO(S, L) YUV_LAUNCH_VEC(chroma_to_planar_kernel, vec, grid, block, stream, a, T, S, L)
    CK_DISPATCH(T, fmt);
#undef GO
    return launched();
}

template <typename T>
static int from_planar_t(const void* planar, const fldr_chroma_frame& out, const fldr_chroma_format& fmt, const YuvCoeffs& k, int H, int W,
                         hipStream_t stream) {
    constexpr int R = RUN<T>;
    OutArgs a;
    const int np = planes_used(fmt.layout);
    bool vec = W % R == 0 && al(planar, 16);
    for (int p = 0; p < 3; ++p) {
        a.plane[p] = p < np ? (uint8_t*)out.plane[p] : nullptr;
        a.pitch[p] = p < np ? out.pitch[p] : 0;
        if (p < np) vec = vec && al(out.plane[p], 16) && al(out.pitch[p], 16);
    }
    a.src = (const uint8_t*)planar; a.H = H; a.W = W; a.k = k;
    const dim3 grid = row_grid<CK_TX, CK_TY>(R, H, W, 1), block(CK_TX, CK_TY);
#define GO(S, L) YUV_LAUNCH_VEC(chroma_from_planar_kernel, vec, grid, block, stream, a, T, S, L)
    CK_DISPATCH(T, fmt);
#undef GO
    return launched();
}

int to_planar(const fldr_chroma_frame* in, int n, const fldr_chroma_format& fmt, const YuvCoeffs& k, void* planar, int H, int W, hipStream_t stream) {
    return fmt.depth == 10 ? to_planar_t<uint16_t>(in, n, fmt, k, planar, H, W, stream) : to_planar_t<uint8_t>(in, n, fmt, k, planar, H, W, stream);
}

int from_planar(const void* planar, const fldr_chroma_frame& out, const fldr_chroma_format& fmt, const YuvCoeffs& k, int H, int W, hipStream_t stream) {
    return fmt.depth == 10 ? from_planar_t<uint16_t>(planar, out, fmt, k, H, W, stream) : from_planar_t<uint8_t>(planar, out, fmt, k, H, W, stream);
}

}  // namespace fldr_chroma_impl
