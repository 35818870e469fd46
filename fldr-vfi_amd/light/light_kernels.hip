// The kernels of libfldr_light.so: the weighted sum of up to MAX_FRAMES frames' linear-light values into a uint32 accumulator
// (accumulate), the code nearest to an accumulator's mean (resolve), and the two fused with the sums kept in registers (mix).
//
// They work on planar BGR code values — 3 H W samples in a row, as the video library's converters (video/video_kernels.hip, compiled
// into this library as well) leave and take them — so a frame is one flat run.  A lane takes 16 bytes of it, 16 samples at depth 8, 8 at
// depth 10, from every frame, four frames' loads in flight at a time; the accumulator (64 or 32 bytes per lane, aligned uint4) is read
// and written once for all the frames of a launch.  The wide form (VEC) loads the 16 bytes at once and needs every source address
// 16-byte aligned; the per-sample form does the same arithmetic on loads of one sample each (the second frame of a planar pair of odd
// size starts anywhere).  Accumulator and output are the library's own buffers and always aligned.  The samples behind the last whole 16
// bytes go one by one in either form.  The 16-byte reader, the weighted gather over the frames (here with lin[] as the per-sample map),
// the accumulator's uint4 form and the launch by VEC are ../video/sample16_device.h, one text with the shutter kernels.
//
// Both tables of the curve live in LDS, copied by every workgroup before its first item: lin[code] (up to 4 KB) for the way in, and for
// the way back up[c] = (mid[c] + 1) >> 1 (up to 4 KB).  With T the total and X = 2 acc + T the header's q is X / (2 T), and
//     mid[c] <= 2 q   <=>   up[c] <= q   <=>   up[c] * 2 T <= X   <=>   up[c] * T <= acc + (T >> 1)
// (2 q is even; a <= x / d <=> a d <= x; the last step halves an inequality between an integer and T / 2).  Both sides stay below 2^32:
// up[c] <= 2^24 - 1 and T <= 255.  So the count of entries with mid[c] <= 2 q is a binary search on a monotone table with one
// multiplication per step and no division: 8 steps at depth 8, 10 at depth 10.  Every quantity is an integer, so the order of the frames
// and the shape of the launch do not show in the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../video/sample16_device.h"
#include "light_internal.h"

namespace fldr_light_impl {

using fldr_sample16::load_acc;
using fldr_sample16::store_acc;

#define LK_THREADS 256
#define LK_MAX_BLOCKS 2048       // 8 workgroups per CU of an MI355X; longer frames walk with the grid's stride

template <bool DEEP> struct Form {
    static constexpr int BPS = DEEP ? 2 : 1;                   // bytes per sample
    static constexpr int SPC = 16 / BPS;                       // samples per 16 bytes
    static constexpr int CODES = DEEP ? 1024 : 256;
    static constexpr uint32_t MASK = CODES - 1;
};

template <bool DEEP> __device__ __forceinline__ uint32_t code_at(const void* base, int64_t i) {
    if (DEEP) return reinterpret_cast<const uint16_t*>(base)[i] & Form<DEEP>::MASK;
    return reinterpret_cast<const uint8_t*>(base)[i];
}

// the weighted linear sum of the 16 bytes at byte offset `off` of every frame, added to s (../video/sample16_device.h)
template <bool DEEP, bool VEC>
__device__ __forceinline__ void gather16(const Sources& a, int64_t off, uint32_t* s, const uint32_t* lin) {
    fldr_sample16::gather16<DEEP, 0, VEC>(
        a.n, a.weight, [&](int k) { return reinterpret_cast<const uint8_t*>(a.codes[k]) + off; }, [&](uint32_t code) { return lin[code]; }, s);
}

template <bool DEEP> __device__ __forceinline__ uint32_t gather1(const Sources& a, int64_t i, const uint32_t* lin) {
    uint32_t v = 0;
    for (int k = 0; k < a.n; ++k) v += a.weight[k] * lin[code_at<DEEP>(a.codes[k], i)];
    return v;
}

// the number of c in 1 .. max with up[c] * total <= acc + (total >> 1): every step keeps lo + step <= max
template <bool DEEP> __device__ __forceinline__ uint32_t nearest_code(uint32_t acc, uint32_t total, const uint32_t* up) {
    const uint32_t x = acc + (total >> 1);
    uint32_t lo = 0;
#pragma unroll
    for (int step = Form<DEEP>::CODES / 2; step >= 1; step >>= 1)
        if (up[lo + step] * total <= x) lo += step;
    return lo;
}

// the codes of one group's sums, as 16 bytes at p (aligned)
template <bool DEEP> __device__ __forceinline__ void finish16(const uint32_t* s, uint32_t total, const uint32_t* up, uint8_t* p) {
    constexpr int SPC = Form<DEEP>::SPC;
    uint32_t q[SPC];
#pragma unroll
    for (int i = 0; i < SPC; ++i) q[i] = nearest_code<DEEP>(s[i], total, up);
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        d[i] = !DEEP ? (q[4 * i] | (q[4 * i + 1] << 8) | (q[4 * i + 2] << 16) | (q[4 * i + 3] << 24)) : (q[2 * i] | (q[2 * i + 1] << 16));
    *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
}

template <bool DEEP> __device__ __forceinline__ void store_code(void* base, int64_t i, uint32_t v) {
    if (DEEP) reinterpret_cast<uint16_t*>(base)[i] = (uint16_t)v;
    else reinterpret_cast<uint8_t*>(base)[i] = (uint8_t)v;
}

template <bool DEEP> __device__ __forceinline__ void stage_lin(uint32_t* lin, const Tables& t) {
    for (int i = threadIdx.x; i < Form<DEEP>::CODES; i += LK_THREADS) lin[i] = t.lin[i];
}

template <bool DEEP> __device__ __forceinline__ void stage_up(uint32_t* up, const Tables& t) {
    for (int i = threadIdx.x; i < Form<DEEP>::CODES; i += LK_THREADS) up[i] = (t.mid[i] + 1u) >> 1;
}

// One item is one whole 16-byte group of the frame; the samples behind the last whole group are the first workgroup's, one per lane.
#define LK_WALK(count)                                                                                               \
    const uint32_t full = (uint32_t)((count) / SPC);                                                                 \
    const int tail = (int)((count) - (int64_t)full * SPC);                                                           \
    for (uint32_t item = blockIdx.x * LK_THREADS + threadIdx.x; item < full; item += gridDim.x * LK_THREADS)
#define LK_TAIL() if (blockIdx.x == 0 && (int)threadIdx.x < tail)

template <bool DEEP, bool VEC>
__global__ __launch_bounds__(LK_THREADS) void light_accumulate_kernel(Tables t, Sources a, uint32_t* acc, int64_t count, int first) {
    constexpr int SPC = Form<DEEP>::SPC;
    __shared__ uint32_t lin[Form<DEEP>::CODES];
    stage_lin<DEEP>(lin, t);
    __syncthreads();
    LK_WALK(count) {
        uint32_t* ap = acc + (int64_t)item * SPC;
        uint32_t s[SPC];
        if (first) {
#pragma unroll
            for (int i = 0; i < SPC; ++i) s[i] = 0;
        } else {
            load_acc<SPC>(ap, s);
        }
        gather16<DEEP, VEC>(a, 16ll * item, s, lin);
        store_acc<SPC>(ap, s);
    }
    LK_TAIL() {
        const int64_t i = (int64_t)full * SPC + threadIdx.x;
        acc[i] = (first ? 0u : acc[i]) + gather1<DEEP>(a, i, lin);
    }
}

template <bool DEEP>
__global__ __launch_bounds__(LK_THREADS) void light_resolve_kernel(Tables t, const uint32_t* acc, uint32_t total, void* out, int64_t count) {
    constexpr int SPC = Form<DEEP>::SPC;
    __shared__ uint32_t up[Form<DEEP>::CODES];
    stage_up<DEEP>(up, t);
    __syncthreads();
    LK_WALK(count) {
        uint32_t s[SPC];
        load_acc<SPC>(acc + (int64_t)item * SPC, s);
        finish16<DEEP>(s, total, up, reinterpret_cast<uint8_t*>(out) + 16ll * item);
    }
    LK_TAIL() {
        const int64_t i = (int64_t)full * SPC + threadIdx.x;
        store_code<DEEP>(out, i, nearest_code<DEEP>(acc[i], total, up));
    }
}

template <bool DEEP, bool VEC>
__global__ __launch_bounds__(LK_THREADS) void light_mix_kernel(Tables t, Sources a, uint32_t total, void* out, int64_t count) {
    constexpr int SPC = Form<DEEP>::SPC;
    __shared__ uint32_t lin[Form<DEEP>::CODES];
    __shared__ uint32_t up[Form<DEEP>::CODES];
    stage_lin<DEEP>(lin, t);
    stage_up<DEEP>(up, t);
    __syncthreads();
    LK_WALK(count) {
        uint32_t s[SPC];
#pragma unroll
        for (int i = 0; i < SPC; ++i) s[i] = 0;
        gather16<DEEP, VEC>(a, 16ll * item, s, lin);
        finish16<DEEP>(s, total, up, reinterpret_cast<uint8_t*>(out) + 16ll * item);
    }
    LK_TAIL() {
        const int64_t i = (int64_t)full * SPC + threadIdx.x;
        store_code<DEEP>(out, i, nearest_code<DEEP>(gather1<DEEP>(a, i, lin), total, up));
    }
}

namespace {

// count < 2^35 (the host refuses more), so the groups fit 32 bits
dim3 grid_of(bool deep, int64_t count) {
    const int64_t groups = count / (deep ? 8 : 16);
    const int64_t blocks = (groups + LK_THREADS - 1) / LK_THREADS;
    return dim3((unsigned)(blocks < 1 ? 1 : blocks > LK_MAX_BLOCKS ? LK_MAX_BLOCKS : blocks));
}

}  // namespace

int launch_accumulate(bool deep, int64_t count, const Tables& t, const Sources& src, bool first, uint32_t* acc, bool vec, hipStream_t stream) {
    const dim3 grid = grid_of(deep, count);
    const int f = first ? 1 : 0;
    if (deep) SAMPLE16_LAUNCH_VEC(light_accumulate_kernel, true, vec, grid, LK_THREADS, stream, t, src, acc, count, f);
    else SAMPLE16_LAUNCH_VEC(light_accumulate_kernel, false, vec, grid, LK_THREADS, stream, t, src, acc, count, f);
    return (int)hipGetLastError();
}

int launch_resolve(bool deep, int64_t count, const Tables& t, const uint32_t* acc, uint32_t total, void* out, hipStream_t stream) {
    const dim3 grid = grid_of(deep, count);
    if (deep) light_resolve_kernel<true><<<grid, LK_THREADS, 0, stream>>>(t, acc, total, out, count);
    else light_resolve_kernel<false><<<grid, LK_THREADS, 0, stream>>>(t, acc, total, out, count);
    return (int)hipGetLastError();
}

int launch_mix(bool deep, int64_t count, const Tables& t, const Sources& src, uint32_t total, void* out, bool vec, hipStream_t stream) {
    const dim3 grid = grid_of(deep, count);
    if (deep) SAMPLE16_LAUNCH_VEC(light_mix_kernel, true, vec, grid, LK_THREADS, stream, t, src, total, out, count);
    else SAMPLE16_LAUNCH_VEC(light_mix_kernel, false, vec, grid, LK_THREADS, stream, t, src, total, out, count);
    return (int)hipGetLastError();
}

}  // namespace fldr_light_impl
