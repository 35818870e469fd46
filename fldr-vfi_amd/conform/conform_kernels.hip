// The kernel of libfldr_conform.so: the direct YUV 4:2:0 -> YUV 4:2:0 conversion of fldr_conform.h, every plane of the frame in one launch.
//
// A lane owns RUN_BYTES = 16 bytes of an output row — a run of 16 samples at depth 8, 8 at depth 10 —, converts the source samples under
// it and stores the run: one uint4 where its address is a multiple of 16, sample by sample otherwise, as a row's last, partial run always
// is.  A workgroup is CONFORM_THREADS consecutive runs of a plane, row by row, so consecutive lanes store consecutive 16 bytes.  The first
// luma_blocks workgroups are the luma plane; the others the chroma: a chroma run is 16 bytes of EVERY chroma plane of the output at the
// same columns (both planes of I420, the one of NV12), since U' and V' of a column come from the same U and V.
//   The kernel is bound by its bytes, so a run loads its source samples as one wide word (4 .. 64 bytes, ../video/yuv_run_device.h)
// where the run lies inside the picture and the address allows it, and sample by sample, indices clamped, otherwise: at the picture's
// edges, with a source plane off its alignment, or with a dst_x that moves the picture off the runs.  Both give the same values.
//   With equal matrices (MATRIX = false) the luma pass reads no chroma at all and the chroma pass has no cross terms.  With different
// matrices a luma run needs the chroma columns x/2 .. x/2 + run/2 of two chroma rows: each row is loaded ONCE per run (run/2 columns wide,
// one more sample by sample), combined vertically (1, 3 / 3, 1) once per column, and every tap of the run reads registers.
//   NV12's interleaved chroma is the same body with a component stride of 2 (PAIR).  Samples outside the picture are the destination's
// black.  All arithmetic is integer; the destination offset is folded into the sum and the value is clamped BEFORE the final shift, then
// packed with v_perm_b32 (../video/yuv_run_device.h): the other order is what hipcc turns into v_ashr_pk_u8_i32, whose upper half has
// come back non-zero on gfx950 (DESIGN_LOG.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../video/sample16_device.h"
#include "../video/yuv_run_device.h"
#include "conform_internal.h"

namespace fldr_conform_impl {
using namespace fldr_sample16;
using fldr_yuv_run::ld_wide;
using fldr_yuv_run::pack2h;
using fldr_yuv_run::pack4;
using fldr_yuv_run::unpack;

template <int LAY> struct Lay {
    static constexpr int FORM = LAY == LAY_P010 ? FORM_P010 : LAY == LAY_LOW10 ? FORM_LOW10 : FORM_BYTE;
    static constexpr bool NV = LAY == LAY_NV8 || LAY == LAY_P010;            // the chroma plane interleaves U and V
    using S = Sample<FORM>;
};

// Columns c0 .. c0 + N - 1 of a row of `lim` columns as sample values: u[N], and v[N] where the row interleaves two components (PAIR).
// One wide load where the columns lie inside the row and the address allows it; otherwise sample by sample, indices clamped to the row.
template <int FORM, int N, bool PAIR>
__device__ __forceinline__ void fetch(const uint8_t* row, int c0, int lim, int* u, int* v) {
    using S = Sample<FORM>;
    using T = typename std::conditional<S::WORDS, uint16_t, uint8_t>::type;
    constexpr int G = PAIR ? 2 : 1, NB = N * G * S::BPS, AL = NB < 16 ? NB : 16;
    const uint8_t* p = row + (int64_t)c0 * (G * S::BPS);
    if (c0 >= 0 && c0 + N <= lim && ((uintptr_t)p & (AL - 1)) == 0) {
        uint32_t w[(NB + 3) / 4];
        int s[N * G];
        ld_wide<NB>(p, w);
        unpack<T, N * G>(w, s);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            u[j] = value_of<FORM>((uint32_t)s[j * G]);
            if (PAIR) v[j] = value_of<FORM>((uint32_t)s[j * G + 1]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = min(max(c0 + j, 0), lim - 1);
            u[j] = value_of<FORM>(load_raw<FORM>(row + (int64_t)c * (G * S::BPS)));
            if (PAIR) v[j] = value_of<FORM>(load_raw<FORM>(row + (int64_t)c * (G * S::BPS) + S::BPS));
        }
    }
}

// one chroma row for a luma run: columns k0 .. k0 + N (N wide, then one more), both components
template <int LAY, int N>
__device__ __forceinline__ void fetch_chroma_row(const ConformArgs& a, int r, int k0, int cw, int* u, int* v) {
    using L = Lay<LAY>;
    constexpr int FORM = L::FORM, BPS = L::S::BPS;
    const int ke = min(max(k0 + N, 0), cw - 1);
    const uint8_t* r1 = a.src[1] + (int64_t)r * a.pitch_src[1];
    if (L::NV) {
        fetch<FORM, N, true>(r1, k0, cw, u, v);
        u[N] = value_of<FORM>(load_raw<FORM>(r1 + (int64_t)ke * (2 * BPS)));
        v[N] = value_of<FORM>(load_raw<FORM>(r1 + (int64_t)ke * (2 * BPS) + BPS));
    } else {
        const uint8_t* r2 = a.src[2] + (int64_t)r * a.pitch_src[2];
        fetch<FORM, N, false>(r1, k0, cw, u, nullptr);
        fetch<FORM, N, false>(r2, k0, cw, v, nullptr);
        u[N] = value_of<FORM>(load_raw<FORM>(r1 + (int64_t)ke * BPS));
        v[N] = value_of<FORM>(load_raw<FORM>(r2 + (int64_t)ke * BPS));
    }
}

// The Bayer matrix of fldr_conform.h as b(x, y) = (X5(x) ^ (Y4(y) << 1)) | Y4(y): X5 spreads the bits of x & 7 to bits 5, 3, 1 and Y4
// those of y & 7 to bits 4, 2, 0.  A run begins at a column whose low bits are zero below the run's length, so X5(x0 + j) = X5(x0) ^ X5(j).
__host__ __device__ constexpr int bayer_x5(int x) { return ((x & 1) << 5) | ((x & 2) << 2) | ((x & 4) >> 1); }
__device__ __forceinline__ int bayer_y4(int y) { return ((y & 1) << 4) | ((y & 2) << 1) | ((y & 4) >> 2); }

// the rounding term of sample j of a run under a shift by SH: half the divisor, or (2 b + 1) << (SH - 7) under the ordered dither
template <int SH> __device__ __forceinline__ int rounding(int dither, int base, int y4, int j) {
    return dither ? (2 * ((base ^ bayer_x5(j & 7)) | y4) + 1) << (SH - 7) : 1 << (SH - 1);
}

// n values that fit a sample -> the 16 bytes of a run, the samples in their container's canonical form
template <int FORM> __device__ __forceinline__ void pack_run(const int* o, uint32_t d[4]) {
    using S = Sample<FORM>;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        d[i] = S::WORDS ? pack2h((int)canonical<FORM>(o[2 * i]), (int)canonical<FORM>(o[2 * i + 1]))
                        : pack4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

template <int FORM> __device__ __forceinline__ void store_run16(uint8_t* p, int nv, const uint32_t d[4]) {
    if (((uintptr_t)p & (RUN_BYTES - 1)) == 0) store_group<FORM, true>(p, nv, d);
    else store_group<FORM, false>(p, nv, d);
}

template <int LIN, int LOUT, bool MATRIX>
__device__ __forceinline__ void luma_run(const ConformArgs& a, uint32_t idx) {
    using I = Lay<LIN>;
    using O = Lay<LOUT>;
    constexpr int NS = O::S::NS, MX = O::S::MX, SH = 17;
    constexpr int TOP = ((MX + 1) << SH) - 1;
    const int y = (int)(idx / a.luma_runs), x0 = (int)(idx - (uint32_t)y * a.luma_runs) * NS;
    const int ys = y - a.dst_y, xs0 = x0 - a.dst_x;
    int o[NS];
    if (ys >= 0 && ys < a.in_H && xs0 + NS > 0 && xs0 < a.in_W) {
        int Y[NS], cu[NS], cv[NS];
        fetch<I::FORM, NS, false>(a.src[0] + (int64_t)ys * a.pitch_src[0], xs0, a.in_W, Y, nullptr);
        if (MATRIX) {
            constexpr int NC = NS / 2;
            const int ch = (a.in_H + 1) >> 1, cw = (a.in_W + 1) >> 1;
            const int odd = ys & 1;
            const int ra = min(max(odd ? (ys - 1) >> 1 : (ys >> 1) - 1, 0), ch - 1), rb = min(odd ? (ys + 1) >> 1 : ys >> 1, ch - 1);
            const int wa = odd ? 3 : 1, wb = 4 - wa;
            int ua[NC + 1], va[NC + 1], ub[NC + 1], vb[NC + 1];
            fetch_chroma_row<LIN, NC>(a, ra, xs0 >> 1, cw, ua, va);
            fetch_chroma_row<LIN, NC>(a, rb, xs0 >> 1, cw, ub, vb);
#pragma unroll
            for (int k = 0; k <= NC; ++k) { ua[k] = wa * ua[k] + wb * ub[k]; va[k] = wa * va[k] + wb * vb[k]; }
#pragma unroll
            for (int i = 0; i < NS; ++i) {                              // xs0 is even: sample i is odd exactly where i is
                cu[i] = ((i & 1) ? ua[i >> 1] + ua[(i >> 1) + 1] : 2 * ua[i >> 1]) - 8 * a.cc_s;
                cv[i] = ((i & 1) ? va[i >> 1] + va[(i >> 1) + 1] : 2 * va[i >> 1]) - 8 * a.cc_s;
            }
        }
        const int y4 = bayer_y4(y), base = y4 << 1;                     // x0 & 7 == 0
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            int acc = 8 * a.kyy * (Y[i] - a.yo_s) + rounding<SH>(a.dither, base, y4, i) + (a.yo_d << SH);
            if (MATRIX) acc += a.kyu * cu[i] + a.kyv * cv[i];
            o[i] = (unsigned)(xs0 + i) < (unsigned)a.in_W ? min(max(acc, 0), TOP) >> SH : a.yo_d;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) o[i] = a.yo_d;
    }
    uint32_t d[4];
    pack_run<O::FORM>(o, d);
    store_run16<O::FORM>(a.dst[0] + (int64_t)y * a.pitch_dst[0] + (int64_t)x0 * O::S::BPS, min(NS, a.out_W - x0), d);
}

template <int LIN, int LOUT, bool MATRIX>
__device__ __forceinline__ void chroma_run(const ConformArgs& a, uint32_t idx) {
    using I = Lay<LIN>;
    using O = Lay<LOUT>;
    constexpr int NS = O::S::NS, MX = O::S::MX, SH = 14;
    constexpr int N = O::NV ? NS / 2 : NS;                              // columns of a run
    constexpr int TOP = ((MX + 1) << SH) - 1;
    const int r = (int)(idx / a.chroma_runs), c0 = (int)(idx - (uint32_t)r * a.chroma_runs) * N;
    const int cw = (a.in_W + 1) >> 1, ch = (a.in_H + 1) >> 1, ocw = (a.out_W + 1) >> 1;
    const int rs = r - (a.dst_y >> 1), cs0 = c0 - (a.dst_x >> 1);
    int ou[N], ov[N];
    if (rs >= 0 && rs < ch && cs0 + N > 0 && cs0 < cw) {
        int U[N], V[N];
        if (I::NV) {
            fetch<I::FORM, N, true>(a.src[1] + (int64_t)rs * a.pitch_src[1], cs0, cw, U, V);
        } else {
            fetch<I::FORM, N, false>(a.src[1] + (int64_t)rs * a.pitch_src[1], cs0, cw, U, nullptr);
            fetch<I::FORM, N, false>(a.src[2] + (int64_t)rs * a.pitch_src[2], cs0, cw, V, nullptr);
        }
        const int y4 = bayer_y4(r), base = (y4 << 1) ^ bayer_x5(c0 & 7);   // c0 & 7 is 0, or 4 with runs of four columns
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int du = U[j] - a.cc_s, dv = V[j] - a.cc_s;
            const int rc = rounding<SH>(a.dither, base, y4, j) + (a.cc_d << SH);
            int au = a.kuu * du + rc, av = a.kvv * dv + rc;
            if (MATRIX) { au += a.kuv * dv; av += a.kvu * du; }
            const bool in = (unsigned)(cs0 + j) < (unsigned)cw;
            ou[j] = in ? min(max(au, 0), TOP) >> SH : a.cc_d;
            ov[j] = in ? min(max(av, 0), TOP) >> SH : a.cc_d;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) ou[j] = ov[j] = a.cc_d;
    }
    const int nv = min(N, ocw - c0);
    uint32_t d[4];
    if (O::NV) {
        int o[NS];
#pragma unroll
        for (int j = 0; j < N; ++j) { o[2 * j] = ou[j]; o[2 * j + 1] = ov[j]; }
        pack_run<O::FORM>(o, d);
        store_run16<O::FORM>(a.dst[1] + (int64_t)r * a.pitch_dst[1] + (int64_t)c0 * (2 * O::S::BPS), 2 * nv, d);
    } else {
        pack_run<O::FORM>(ou, d);
        store_run16<O::FORM>(a.dst[1] + (int64_t)r * a.pitch_dst[1] + (int64_t)c0 * O::S::BPS, nv, d);
        pack_run<O::FORM>(ov, d);
        store_run16<O::FORM>(a.dst[2] + (int64_t)r * a.pitch_dst[2] + (int64_t)c0 * O::S::BPS, nv, d);
    }
}

template <int LIN, int LOUT, bool MATRIX>
__global__ __launch_bounds__(CONFORM_THREADS) void conform_kernel(ConformArgs a) {
    const uint32_t b = blockIdx.x;
    if (b < a.luma_blocks) {
        const uint32_t idx = b * CONFORM_THREADS + threadIdx.x;
        if (idx < a.luma_runs * (uint32_t)a.out_H) luma_run<LIN, LOUT, MATRIX>(a, idx);
    } else {
        const uint32_t idx = (b - a.luma_blocks) * CONFORM_THREADS + threadIdx.x;
        if (idx < a.chroma_runs * (uint32_t)((a.out_H + 1) >> 1)) chroma_run<LIN, LOUT, MATRIX>(a, idx);
    }
}

template <int LIN, int LOUT> void launch(const ConformArgs& a, bool matrix, hipStream_t stream) {
    if (matrix) conform_kernel<LIN, LOUT, true><<<a.blocks, CONFORM_THREADS, 0, stream>>>(a);
    else conform_kernel<LIN, LOUT, false><<<a.blocks, CONFORM_THREADS, 0, stream>>>(a);
}

template <int LIN> void launch_in(const ConformArgs& a, int lay_out, bool matrix, hipStream_t stream) {
    if (lay_out == LAY_NV8) launch<LIN, LAY_NV8>(a, matrix, stream);
    else if (lay_out == LAY_I8) launch<LIN, LAY_I8>(a, matrix, stream);
    else if (lay_out == LAY_P010) launch<LIN, LAY_P010>(a, matrix, stream);
    else launch<LIN, LAY_LOW10>(a, matrix, stream);
}

int conform(const ConformArgs& a, int lay_in, int lay_out, bool matrix, hipStream_t stream) {
    if (lay_in == LAY_NV8) launch_in<LAY_NV8>(a, lay_out, matrix, stream);
    else if (lay_in == LAY_I8) launch_in<LAY_I8>(a, lay_out, matrix, stream);
    else if (lay_in == LAY_P010) launch_in<LAY_P010>(a, lay_out, matrix, stream);
    else launch_in<LAY_LOW10>(a, lay_out, matrix, stream);
    return (int)hipGetLastError();
}

}  // namespace fldr_conform_impl
