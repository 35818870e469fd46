// The kernel of libfldr_scale.so: the separable integer resize of fldr_scale.h, both passes in one launch, every plane of the frame in it.
//
// A workgroup owns a tile of output samples of one plane: tile_w samples (TILE_GROUPS 16-byte groups) by tile_h rows.  It reads from the
// vertical table which source rows the tile needs (the first left_y of the tile to the last left_y + ny - 1, clamped to the plane), runs
// the horizontal pass for those rows and the tile's columns into LDS as int16 — m never goes to HBM —, and then the vertical pass out of
// LDS: one 16-byte group of one output row per thread, stored as one uint4 where the output plane allows it (ScalePlane::vec) and sample
// by sample otherwise, as a row's last, partial group always is.
//   The intermediate is row-major, a tile row of tile_w int16 (512 or 256 bytes) apart.  Horizontal pass: consecutive lanes write
// consecutive int16, two lanes to a bank, no conflict.  Vertical pass: a lane reads its group as 16-byte vectors (one at depth 10, two at
// depth 8); the sixteen lanes of an output row cover one contiguous 256- or 512-byte run, but a wave is four output rows, whose source
// rows lie a multiple of the bank span apart (or are the same row, in an enlargement): those reads can serialise.  A padded row stride
// has not been tried (DESIGN_LOG.md).
//   The horizontal pass reads its source samples in one of two ways, chosen per map by the host (ScalePlane::stage_span):
//     direct   every multiply-add has a global load of one sample in front of it; four source rows per lane at a time, so that a
//              coefficient and a clamped column are formed once for four multiply-adds; neighbouring lanes read neighbouring samples and
//              the taps of a column come out of the caches;
//     staged   the source rows go through LDS a chunk of STAGE_ROWS rows at a time: every sample between the first and the last source
//              column of the tile is loaded ONCE, consecutive lanes consecutive samples, its value stored as a 16-bit word, and the taps
//              read LDS.  Two barriers per chunk.
//   Both give the same bytes; DESIGN_LOG.md has both measured, and the rule by which the host picks.
//   NV12's interleaved chroma is the same body with a component shift of 1: sample x of a row is component x & 1 of column x >> 1.
//   All arithmetic is integer.  Values are clamped before the final shift and packed with v_perm_b32 (../video/yuv_run_device.h): the
// other order is what hipcc turns into v_ashr_pk_u8_i32, whose upper half has come back non-zero on gfx950 (DESIGN_LOG.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/yuv_run_device.h"
#include "scale_internal.h"

namespace fldr_scale_impl {
using namespace fldr_sample16;
using fldr_yuv_run::pack2h;
using fldr_yuv_run::pack4;

template <int FORM, bool VEC, bool STAGE>
__device__ __forceinline__ void scale_tile(const ScalePlane& pl, int nx, int ny, uint32_t tile, int16_t* m, uint16_t* stage) {
    using S = Sample<FORM>;
    constexpr int D = S::WORDS ? 10 : 8;
    constexpr int SH_H = D, SH_V = 28 - D;                             // 14 - e and 14 + e with e = 14 - D
    constexpr int TW = TILE_GROUPS * S::NS, TW_LOG = S::WORDS ? 7 : 8;
    const int tid = threadIdx.x;
    const int x0 = (int)(tile % pl.tiles_x) * TW, y0 = (int)(tile / pl.tiles_x) * pl.tile_h;
    const int x1 = min(x0 + TW, pl.out_w), y1 = min(y0 + pl.tile_h, pl.out_rows);
    const int R = pl.in_rows, N = pl.in_cols;
    // the source rows of the tile: every clamped row index of every output row of it lies in lo .. hi
    const int lo = min(max(pl.left_y[y0], 0), R - 1), hi = min(max(pl.left_y[y1 - 1] + ny - 1, 0), R - 1);

    if constexpr (STAGE) {
        constexpr int CR = STAGE_ROWS_BYTE * (S::WORDS ? 2 : 1);        // rows of a chunk: one column of four rows per thread
        const int SS = pl.stage_span;
        const int x = tid & (TW - 1), rg = 4 * (tid >> TW_LOG);
        const int xo = x0 + x;
        const bool mine = xo < x1;
        const int o = min(xo, x1 - 1) >> pl.cshift, comp = min(xo, x1 - 1) - (o << pl.cshift);
        const int l = pl.left_x[o];
        const int16_t* q = pl.coef_x + (int64_t)o * nx;
        // the source samples of the tile: every clamped column of every output column of it lies in s_lo .. s_lo + ns - 1
        const int s_lo = min(max(pl.left_x[x0 >> pl.cshift], 0), N - 1) << pl.cshift;
        const int ns = ((min(max(pl.left_x[(x1 - 1) >> pl.cshift] + nx - 1, 0), N - 1) + 1) << pl.cshift) - s_lo;
        for (int c0 = lo; c0 <= hi; c0 += CR) {
            __syncthreads();                                           // the chunk before has been read
#pragma unroll 1
            for (int i = 0; i < CR; ++i) {                             // rolled: eight rows' pointers at once do not fit the scalar registers
                const uint8_t* row = pl.src + (int64_t)min(c0 + i, hi) * pl.pitch_src + (int64_t)s_lo * S::BPS;
                for (int j = tid; j < ns; j += SCALE_THREADS) stage[i * SS + j] = (uint16_t)value_of<FORM>(load_raw<FORM>(row + j * S::BPS));
            }
            __syncthreads();
            if (mine) {
                const uint16_t* st = stage + rg * SS + comp - s_lo;
                int acc[4] = { 0, 0, 0, 0 };
                for (int k = 0; k < nx; ++k) {
                    const int at = min(max(l + k, 0), N - 1) << pl.cshift;
                    const int qk = q[k];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] += qk * (int)st[i * SS + at];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c0 + rg + i <= hi) m[(c0 + rg + i - lo) * TW + x] = (int16_t)((acc[i] + (1 << (SH_H - 1))) >> SH_H);
            }
        }
    } else {
        const int chunks = (hi - lo + 4) >> 2;                         // of four source rows
        for (int idx = tid; idx < chunks * TW; idx += SCALE_THREADS) {
            const int x = idx & (TW - 1), r0 = lo + 4 * (idx >> TW_LOG);
            const int xo = x0 + x;
            if (xo >= x1) continue;
            const int o = xo >> pl.cshift, comp = xo - (o << pl.cshift);
            const int l = pl.left_x[o];
            const int16_t* q = pl.coef_x + (int64_t)o * nx;
            const uint8_t* row[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) row[i] = pl.src + (int64_t)min(r0 + i, hi) * pl.pitch_src + comp * S::BPS;
            int acc[4] = { 0, 0, 0, 0 };
            for (int k = 0; k < nx; ++k) {
                const int64_t off = ((int64_t)min(max(l + k, 0), N - 1) << pl.cshift) * S::BPS;
                const int qk = q[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] += qk * value_of<FORM>(load_raw<FORM>(row[i] + off));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (r0 + i <= hi) m[(r0 + i - lo) * TW + x] = (int16_t)((acc[i] + (1 << (SH_H - 1))) >> SH_H);
        }
    }
    __syncthreads();

    const int y = y0 + (tid >> 4), g = tid & (TILE_GROUPS - 1);        // TILE_ROWS_MAX x TILE_GROUPS == SCALE_THREADS
    const int xg = x0 + g * S::NS;
    if (y >= y1 || xg >= x1) return;
    const int l = pl.left_y[y];
    const int16_t* q = pl.coef_y + (int64_t)y * ny;
    int acc[S::NS];
#pragma unroll
    for (int i = 0; i < S::NS; ++i) acc[i] = 1 << (SH_V - 1);
    for (int k = 0; k < ny; ++k) {
        const int r = min(max(l + k, 0), R - 1) - lo;
        const uint4* mp = reinterpret_cast<const uint4*>(m + r * TW + g * S::NS);
        const int qk = q[k];
#pragma unroll
        for (int v = 0; v < S::NS / 8; ++v) {
            const uint4 w = mp[v];
            const uint32_t d[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[8 * v + 2 * i] += qk * (int)(int16_t)(d[i] & 0xffffu);
                acc[8 * v + 2 * i + 1] += qk * ((int)d[i] >> 16);
            }
        }
    }
    // clamp(floor(v / 2^SH_V), 0, MX) as the clamp of v to 0 .. (MX + 1) 2^SH_V - 1 and then the shift
    constexpr int TOP = ((S::MX + 1) << SH_V) - 1;
    int o[S::NS];
#pragma unroll
    for (int i = 0; i < S::NS; ++i) o[i] = (int)canonical<FORM>(min(max(acc[i], 0), TOP) >> SH_V);
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = S::WORDS ? pack2h(o[2 * i], o[2 * i + 1]) : pack4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    store_group<FORM, VEC>(pl.dst + (int64_t)y * pl.pitch_dst + (int64_t)xg * S::BPS, min(S::NS, x1 - xg), d);
}

template <int FORM, bool STAGE>
__global__ __launch_bounds__(SCALE_THREADS) void scale_kernel(ScaleArgs a) {
    extern __shared__ __attribute__((aligned(16))) int16_t scale_lds[];
    const uint32_t b = blockIdx.x;
    const int p = a.planes > 2 && b >= a.pl[2].first ? 2 : b >= a.pl[1].first ? 1 : 0;
    const ScalePlane& pl = a.pl[p];
    uint16_t* stage = reinterpret_cast<uint16_t*>(scale_lds + a.stage_at);
    if (pl.vec) scale_tile<FORM, true, STAGE>(pl, a.nx, a.ny, b - pl.first, scale_lds, stage);
    else scale_tile<FORM, false, STAGE>(pl, a.nx, a.ny, b - pl.first, scale_lds, stage);
}

// the staged form where the map keeps a staged span (every plane of a map does, or none)
template <int FORM> void launch(const ScaleArgs& a, int lds_bytes, hipStream_t stream) {
    if (a.pl[0].stage_span) scale_kernel<FORM, true><<<a.total, SCALE_THREADS, lds_bytes, stream>>>(a);
    else scale_kernel<FORM, false><<<a.total, SCALE_THREADS, lds_bytes, stream>>>(a);
}

int scale(const ScaleArgs& a, int form, int lds_bytes, hipStream_t stream) {
    if (form == FORM_BYTE) launch<FORM_BYTE>(a, lds_bytes, stream);
    else if (form == FORM_P010) launch<FORM_P010>(a, lds_bytes, stream);
    else launch<FORM_LOW10>(a, lds_bytes, stream);
    return (int)hipGetLastError();
}

}  // namespace fldr_scale_impl
