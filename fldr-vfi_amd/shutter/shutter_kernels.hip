// The kernels of libfldr_shutter.so: the weighted integer sum of up to MAX_FRAMES frames into a uint32 accumulator (accumulate), the
// rounded quotient of an accumulator written as a frame (resolve), and the two fused with the sums kept in registers (mix).
//
// All three are bandwidth kernels over the planes of YUV 4:2:0 frames.  A lane takes 16 bytes of one row of one plane — 16 samples
// at depth 8, 8 at depth 10 — from every frame, four frames' loads in flight at a time, so the accumulator (64 or 32 bytes per lane,
// as aligned uint4) is read and written once for all the frames of a launch.  The wide form (VEC) loads and stores the 16 bytes at once
// and needs every plane address and pitch involved 16-byte aligned; the per-sample form does the same arithmetic on loads and stores of
// one sample each.  The samples of a row behind its last whole 16 bytes go one by one in either form.  The plane is the grid's y, so
// everything read from the kernel arguments is uniform.  Every quantity is an integer below 2^32 (shutter_internal.h, fldr_shutter.h),
// so the order of the frames and the shape of the launch do not show in the result.  The 16-byte reader, the weighted gather over the
// frames, the accumulator's uint4 form and the launch by sample form are ../video/sample16_device.h, one text with the light kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shutter_internal.h"

namespace fldr_shutter_impl {

using fldr_sample16::load_acc;
using fldr_sample16::store_acc;

#define TK_THREADS 256
#define TK_MAX_BLOCKS 2048       // 8 workgroups per CU of an MI355X; larger planes walk with the grid's stride

template <int MODE> struct Form {
    static constexpr int BPS = MODE == S_BYTE ? 1 : 2;         // bytes per sample
    static constexpr int SPC = 16 / BPS;                       // samples per 16 bytes
};

template <int MODE> __device__ __forceinline__ uint32_t sample_of(const uint8_t* p) {
    if (MODE == S_BYTE) return *p;
    const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
    return MODE == S_P010 ? (w >> 6) : (w & 0x3ffu);
}

template <int MODE> __device__ __forceinline__ void store_sample(uint8_t* p, uint32_t v) {
    if (MODE == S_BYTE) *p = (uint8_t)v;
    else *reinterpret_cast<uint16_t*>(p) = (uint16_t)(MODE == S_P010 ? (v << 6) : v);
}

// the weighted sum of 16 bytes at (row, off) of plane p of every frame, added to s (../video/sample16_device.h)
template <int MODE, bool VEC>
__device__ __forceinline__ void gather16(const Sources& a, int p, uint32_t row, int64_t off, uint32_t* s) {
    fldr_sample16::gather16<MODE != S_BYTE, MODE == S_P010 ? 6 : 0, VEC>(
        a.n, a.weight, [&](int k) { return a.plane[k][p] + (int64_t)row * a.pitch[k][p] + off; }, [](uint32_t v) { return v; }, s);
}

template <int MODE> __device__ __forceinline__ uint32_t gather1(const Sources& a, int p, uint32_t row, int64_t off) {
    uint32_t v = 0;
    for (int k = 0; k < a.n; ++k) v += a.weight[k] * sample_of<MODE>(a.plane[k][p] + (int64_t)row * a.pitch[k][p] + off);
    return v;
}

__device__ __forceinline__ uint32_t quotient(uint32_t acc, const Target& t) {
    return min(__umulhi(2u * acc + t.total, t.mul) >> t.shift, t.maxv);
}

// the quotients of one group's sums, as 16 bytes at p
template <int MODE, bool VEC> __device__ __forceinline__ void finish16(const uint32_t* s, const Target& t, uint8_t* p) {
    constexpr int SPC = Form<MODE>::SPC;
    uint32_t q[SPC];
#pragma unroll
    for (int i = 0; i < SPC; ++i) q[i] = quotient(s[i], t);
    if (VEC) {
        uint32_t d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            d[i] = MODE == S_BYTE  ? (q[4 * i] | (q[4 * i + 1] << 8) | (q[4 * i + 2] << 16) | (q[4 * i + 3] << 24))
                 : MODE == S_P010 ? ((q[2 * i] << 6) | (q[2 * i + 1] << 22))
                                  : (q[2 * i] | (q[2 * i + 1] << 16));
        *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
#pragma unroll
        for (int i = 0; i < SPC; ++i) store_sample<MODE>(p + i * Form<MODE>::BPS, q[i]);
    }
}

// One item is one 16-byte group of a row of plane p = blockIdx.y, the row's partial last group included.
#define TK_WALK(g)                                                                                                   \
    const int p = blockIdx.y;                                                                                        \
    const uint32_t chunks = (g).chunks[p], full = (g).full[p], n_items = (g).items[p];                               \
    const int64_t row_bytes = (g).row_bytes[p];                                                                      \
    for (uint32_t item = blockIdx.x * TK_THREADS + threadIdx.x; item < n_items; item += gridDim.x * TK_THREADS)
#define TK_ITEM()                                                                                                    \
    const uint32_t row = item / chunks, c = item - row * chunks;                                                     \
    const int64_t off = 16ll * c;                                                                                    \
    const bool whole = c < full;                                                                                     \
    const int tail = (int)((row_bytes - 16ll * full) / Form<MODE>::BPS)      /* samples of the partial group */

template <int MODE, bool VEC>
__global__ __launch_bounds__(TK_THREADS) void shutter_accumulate_kernel(Geometry g, Sources a, uint32_t* acc, int first) {
    constexpr int SPC = Form<MODE>::SPC, BPS = Form<MODE>::BPS;
    TK_WALK(g) {
        TK_ITEM();
        if (whole) {
            uint32_t* ap = acc + g.acc_full[p] + ((int64_t)row * full + c) * SPC;
            uint32_t s[SPC];
            if (first) {
#pragma unroll
                for (int i = 0; i < SPC; ++i) s[i] = 0;
            } else {
                load_acc<SPC>(ap, s);
            }
            gather16<MODE, VEC>(a, p, row, off, s);
            store_acc<SPC>(ap, s);
        } else {
            uint32_t* ap = acc + g.acc_tail[p] + (int64_t)row * tail;
            for (int i = 0; i < tail; ++i) ap[i] = (first ? 0u : ap[i]) + gather1<MODE>(a, p, row, off + i * BPS);
        }
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(TK_THREADS) void shutter_resolve_kernel(Geometry g, const uint32_t* acc, Target t) {
    constexpr int SPC = Form<MODE>::SPC, BPS = Form<MODE>::BPS;
    TK_WALK(g) {
        TK_ITEM();
        uint8_t* o = t.plane[p] + (int64_t)row * t.pitch[p] + off;
        if (whole) {
            uint32_t s[SPC];
            load_acc<SPC>(acc + g.acc_full[p] + ((int64_t)row * full + c) * SPC, s);
            finish16<MODE, VEC>(s, t, o);
        } else {
            const uint32_t* ap = acc + g.acc_tail[p] + (int64_t)row * tail;
            for (int i = 0; i < tail; ++i) store_sample<MODE>(o + i * BPS, quotient(ap[i], t));
        }
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(TK_THREADS) void shutter_mix_kernel(Geometry g, Sources a, Target t) {
    constexpr int SPC = Form<MODE>::SPC, BPS = Form<MODE>::BPS;
    TK_WALK(g) {
        TK_ITEM();
        uint8_t* o = t.plane[p] + (int64_t)row * t.pitch[p] + off;
        if (whole) {
            uint32_t s[SPC];
#pragma unroll
            for (int i = 0; i < SPC; ++i) s[i] = 0;
            gather16<MODE, VEC>(a, p, row, off, s);
            finish16<MODE, VEC>(s, t, o);
        } else {
            for (int i = 0; i < tail; ++i) store_sample<MODE>(o + i * BPS, quotient(gather1<MODE>(a, p, row, off + i * BPS), t));
        }
    }
}

bool geometry(int H, int W, const fldr_video_format& fmt, Geometry& g) {
    const bool deep = fmt.depth == 10;
    const int64_t cw = (W + 1) / 2, b = deep ? 2 : 1;
    g.np = fmt.layout == FLDR_VIDEO_NV12 ? 2 : 3;
    g.mode = !deep ? S_BYTE : fmt.layout == FLDR_VIDEO_NV12 ? S_P010 : S_LOW10;
    const int64_t spc = 16 / b;
    int64_t rows[3], full_total = 0;
    g.samples = 0;
    for (int p = 0; p < 3; ++p) {
        const bool used = p < g.np;
        const int64_t row_samples = !used ? 0 : p == 0 ? W : (fmt.layout == FLDR_VIDEO_NV12 ? 2 * cw : cw);
        rows[p] = !used ? 0 : p == 0 ? H : (H + 1) / 2;
        g.row_bytes[p] = row_samples * b;
        const int64_t chunks = (g.row_bytes[p] + 15) / 16, full = g.row_bytes[p] / 16;
        if (chunks * rows[p] > 0x7fffffffll) return false;
        g.chunks[p] = (uint32_t)chunks;
        g.full[p] = (uint32_t)full;
        g.items[p] = (uint32_t)(chunks * rows[p]);
        g.acc_full[p] = full_total;
        full_total += rows[p] * full * spc;
        g.samples += rows[p] * row_samples;
    }
    int64_t tail_total = full_total;
    for (int p = 0; p < 3; ++p) {
        g.acc_tail[p] = tail_total;
        tail_total += rows[p] * (g.row_bytes[p] / b - (int64_t)g.full[p] * spc);
    }
    return true;                                                   // tail_total == g.samples
}

void reciprocal(uint32_t total, uint32_t& mul, uint32_t& shift) {
    // d = 2 total < 2^17, 2^L <= d < 2^(L+1), shift = L - 1, mul = ceil(2^(32 + shift) / d) <= 2^31 + 1.  mul d - 2^(32 + shift) = e
    // with 0 <= e < d, and floor(x mul / 2^(32 + shift)) = floor(x / d) while x e < 2^(32 + shift): x e < 1023.5 d^2 < 2^(2 L + 12),
    // and 2 L + 12 <= 32 + L - 1 for L <= 19.
    const uint64_t d = 2ull * total;
    uint32_t L = 0;
    while ((d >> (L + 1)) != 0) ++L;
    shift = L - 1;
    mul = (uint32_t)(((1ull << (32 + shift)) + d - 1) / d);
}

namespace {

dim3 grid_of(const Geometry& g) {
    uint32_t most = 1;
    for (int p = 0; p < g.np; ++p) most = max(most, g.items[p]);
    return dim3(min((most + TK_THREADS - 1) / TK_THREADS, (uint32_t)TK_MAX_BLOCKS), (unsigned)g.np);
}

}  // namespace

int launch_accumulate(const Geometry& g, const Sources& src, bool first, uint32_t* acc, bool vec, hipStream_t stream) {
    SAMPLE16_LAUNCH(shutter_accumulate_kernel, g.mode, vec, grid_of(g), TK_THREADS, stream, g, src, acc, first ? 1 : 0);
    return (int)hipGetLastError();
}

int launch_resolve(const Geometry& g, const uint32_t* acc, const Target& dst, bool vec, hipStream_t stream) {
    SAMPLE16_LAUNCH(shutter_resolve_kernel, g.mode, vec, grid_of(g), TK_THREADS, stream, g, acc, dst);
    return (int)hipGetLastError();
}

int launch_mix(const Geometry& g, const Sources& src, const Target& dst, bool vec, hipStream_t stream) {
    SAMPLE16_LAUNCH(shutter_mix_kernel, g.mode, vec, grid_of(g), TK_THREADS, stream, g, src, dst);
    return (int)hipGetLastError();
}

}  // namespace fldr_shutter_impl
