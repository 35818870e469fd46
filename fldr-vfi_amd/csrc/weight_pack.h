// What every fp16 hi/lo weight prepack of the library shares (conv_split / conv_spk / conv_ring / conv_s2_split / dec23 / final):
// the max|w| -> power-of-two scale reduction and the header it writes, the hi/lo half of a scaled weight, the A-operand prepack of the
// 3x3 16x16x32 kernels and their output-channel geometry, and the (nmt, terms) -> template instantiation dispatch of their launchers.
// The section-size functions stay with the sections (spk_common.h, the kernel files).
#pragma once
#include "common.h"
#include <type_traits>

typedef _Float16 fldr_h8 __attribute__((ext_vector_type(8)));

// ---- scale ------------------------------------------------------------------------------------------------------------------------
// Header of a pack: {1 / scale, scale, max|w|, 0 ...} (4 or 8 floats; the zeros are the block padding loads read), scale = the largest
// power of two with max|w| * scale <= 8192 (fp16 ends at 65504; the low halves of the other weights stay normal); all-zero weights: 1.
struct FldrPackScale { float mx, scale; };
__device__ __forceinline__ FldrPackScale fldr_pack_scale_of(float thread_max) {     // one block of 256 threads; every thread gets the result
    __shared__ float red[256];
    red[threadIdx.x] = thread_max;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float mx = red[0];
    float scale = 1.0f;
    if (mx > 0.0f) scale = exp2f(floorf(log2f(8192.0f / mx)));
    return {mx, scale};
}
__device__ __forceinline__ FldrPackScale fldr_pack_absmax(const float* __restrict__ w, int64_t n) {
    float m = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(w[i]));
    return fldr_pack_scale_of(m);
}
__device__ __forceinline__ void fldr_pack_write_header(float* __restrict__ hdr, int hdr_floats, FldrPackScale s) {
    const int t = threadIdx.x;
    if (t < hdr_floats) hdr[t] = t == 0 ? 1.0f / s.scale : (t == 1 ? s.scale : (t == 2 ? s.mx : 0.0f));
}
template <int HDR>
__global__ void fldr_pack_absmax_kernel(const float* __restrict__ w, int64_t n, float* __restrict__ hdr) {
    fldr_pack_write_header(hdr, HDR, fldr_pack_absmax(w, n));
}

// ---- halves -----------------------------------------------------------------------------------------------------------------------
// kind 0: hi = the nearest fp16 of the scaled weight; kind 1: lo = the nearest fp16 of what hi leaves
__device__ __forceinline__ _Float16 fldr_pack_half(float x, int kind) {
    const _Float16 h = (_Float16)x;
    return kind == 0 ? h : (_Float16)(x - (float)h);
}

// ---- the 3x3 16x16x32 kernels (conv3x3_split_kernel, conv3x3_spk_kernel, conv3x3_ring_kernel) -------------------------------------
// Output-channel geometry: 16-channel blocks per group (NMT), groups per launch.
static inline void fldr_conv3x3_geometry(int cout, int& nmt, int& groups) {
    if (cout <= 16)      { nmt = 1; groups = 1; }
    else if (cout <= 32) { nmt = 2; groups = 1; }
    else if (cout <= 48) { nmt = 3; groups = 1; }
    else if (cout <= 64) { nmt = 2; groups = 2; }
    else                 { nmt = 3; groups = (cout + 47) / 48; }
}
#define FLDR_PACK3X3_STEPS 5                    // tap pairs per 16-channel chunk (9 taps + 1 zero tap)
// A operands behind a header of HDR floats (whose scale the absmax kernel wrote): [group][chunk][step][m][kind hi|lo][lane][8 halves],
// one 8-half (16-byte) element per thread
template <int HDR>
__global__ void fldr_prepack3x3_kernel(const float* __restrict__ w, float* __restrict__ wp, int cout, int cin, int nmt, int n_chunks, int64_t total_h8) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total_h8) return;
    const float scale = wp[1];
    const int lane = (int)(i % 64);
    const int kind = (int)((i / 64) % 2);
    const int m = (int)((i / 128) % nmt);
    const int s = (int)((i / (128 * nmt)) % FLDR_PACK3X3_STEPS);
    const int ch = (int)((i / (128 * nmt * FLDR_PACK3X3_STEPS)) % n_chunks);
    const int gr = (int)(i / ((int64_t)128 * nmt * FLDR_PACK3X3_STEPS * n_chunks));
    const int li = lane & 15, lg = lane >> 4;
    const int co = gr * 16 * nmt + m * 16 + li;
    const int tap = 2 * s + (lg >> 1);
    fldr_h8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = ch * 16 + (lg & 1) * 8 + j;
        v[j] = fldr_pack_half((tap < 9 && co < cout && c < cin) ? w[((int64_t)co * cin + c) * 9 + tap] * scale : 0.0f, kind);
    }
    reinterpret_cast<fldr_h8*>(wp + HDR)[i] = v;
}
// header + first section of a 3x3 pack: the two launches of fldr_conv_split_prepack and fldr_conv_spk_prepack
template <int HDR>
static inline void fldr_prepack3x3_launch(const float* weight, float* wpack, int cout, int cin, hipStream_t s) {
    int nmt, groups;
    fldr_conv3x3_geometry(cout, nmt, groups);
    const int n_chunks = (cin + 15) / 16;
    const int64_t total_h8 = (int64_t)groups * n_chunks * FLDR_PACK3X3_STEPS * nmt * 2 * 64;
    hipLaunchKernelGGL(fldr_pack_absmax_kernel<HDR>, dim3(1), dim3(256), 0, s, weight, (int64_t)cout * cin * 9, wpack);
    hipLaunchKernelGGL(fldr_prepack3x3_kernel<HDR>, dim3(fldr_cdiv(total_h8, 256)), dim3(256), 0, s, weight, wpack, cout, cin, nmt, n_chunks, total_h8);
}

// ---- launcher dispatch ------------------------------------------------------------------------------------------------------------
// f(NMT, TERMS) with the run-time (nmt in {1, 2, 3}, terms in {1, 3}) as integral constants: f names the instantiation,
//   fldr_dispatch_nmt_terms(nmt, terms, [&](auto NMT, auto TERMS) { return x_launch<NMT(), TERMS()>(...); });
template <typename F>
static inline int fldr_dispatch_nmt_terms(int nmt, int terms, F&& f) {
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    using three = std::integral_constant<int, 3>;
    if (terms == 1) return nmt == 1 ? f(one{}, one{}) : (nmt == 2 ? f(two{}, one{}) : f(three{}, one{}));
    return nmt == 1 ? f(one{}, three{}) : (nmt == 2 ? f(two{}, three{}) : f(three{}, three{}));
}
