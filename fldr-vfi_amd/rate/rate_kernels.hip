// The kernels of libfldr_rate.so: the cut measure of a frame pair (zero, accumulate, decide) and the select that replaces the
// outputs of a cut pair by the nearer input frame.
//
// The measure is a bandwidth kernel: one pass over the two luma planes, 16 bytes per lane and frame when both plane addresses and
// pitches are 16-byte aligned (VEC), the same arithmetic on per-sample loads otherwise; the bytes of a row behind its last whole
// 16 (W not a multiple of 16 samples) go sample by sample in either form.  Per 16 bytes: v_sad_u8 on the dwords (depth 8) or
// v_sad_u16 on the words reduced to 8 bits (depth 10), and the histogram DIFFERENCE h0 - h1, one copy per wave in LDS: +1 at
// y8(I0), -1 at y8(I1), which is all hist_dist needs and halves the LDS of two histograms.  Samples that would all hit one address
// are combined before the atomic: nothing for a 16-byte group equal in both frames, one add for the whole wave when every lane's
// group is the same flat value (black, bars), one per flat group, one per flat dword.  Every sum is an integer, so the order of the
// atomics does not show in the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rate_internal.h"

namespace fldr_rate_impl {

#define SK_THREADS 256
#define SK_WAVES (SK_THREADS / 64)
#define SK_MAX_BLOCKS 2048       // 8 workgroups per CU of an MI355X; larger frames walk with the grid's stride

struct MeasureArgs {
    const uint8_t* y[2];
    int64_t pitch[2];
    int64_t row_bytes;
    uint32_t chunks;             // 16-byte groups per row, the partial last one included
    uint32_t items;              // H * chunks
    uint8_t* state;
};

// sign x (the samples of four reduced dwords) into the wave's histogram
template <int MODE> __device__ __forceinline__ void hist16(int* h, const uint32_t d[4], int sign) {
    constexpr int SPD = MODE == Y8_BYTE ? 4 : 2;                       // samples per dword
    constexpr int SH = MODE == Y8_BYTE ? 8 : 16;
    constexpr uint32_t REP = MODE == Y8_BYTE ? 0x01010101u : 0x00010001u;
    const uint32_t v = d[0] & 0xffu;
    const bool flat = d[0] == v * REP && d[1] == d[0] && d[2] == d[0] && d[3] == d[0];
    const uint32_t first = __builtin_amdgcn_readfirstlane(d[0]);
    if (__all(flat && d[0] == first)) {                                // the lanes here all hold one value: one add for them all
        const int lanes = __popcll(__ballot(1));
        const int lane = threadIdx.x & 63;
        if (lane == __builtin_amdgcn_readfirstlane(lane)) atomicAdd(&h[first & 0xffu], sign * 4 * SPD * lanes);
        return;
    }
    if (flat) { atomicAdd(&h[v], sign * 4 * SPD); return; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = d[i];
        if (w == (w & 0xffu) * REP) { atomicAdd(&h[w & 0xffu], sign * SPD); continue; }
#pragma unroll
        for (int s = 0; s < SPD; ++s) atomicAdd(&h[(w >> (SH * s)) & 0xffu], sign);
    }
}

__global__ __launch_bounds__(SK_THREADS) void scene_zero_kernel(uint8_t* state) {
    reinterpret_cast<uint4*>(state)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);          // 256 x 16 = FLDR_SCENE_STATE_BYTES
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(SK_THREADS) void scene_accumulate_kernel(MeasureArgs a) {
    constexpr int BPS = MODE == Y8_BYTE ? 1 : 2;
    __shared__ int hist[SK_WAVES][256];
    __shared__ unsigned long long wg_sad;
    const int tid = threadIdx.x;
    for (int i = tid; i < SK_WAVES * 256; i += SK_THREADS) (&hist[0][0])[i] = 0;
    if (tid == 0) wg_sad = 0;
    __syncthreads();
    int* h = hist[tid >> 6];
    uint32_t sad = 0;                                                  // <= 255 x 16 x (items / threads of the grid): far inside 32 bits
    for (uint32_t item = blockIdx.x * SK_THREADS + tid; item < a.items; item += gridDim.x * SK_THREADS) {
        const uint32_t row = item / a.chunks, c = item - row * a.chunks;
        const int64_t off = 16ll * c;
        const int nbytes = (int)min((int64_t)16, a.row_bytes - off);
        const uint8_t* p0 = a.y[0] + (int64_t)row * a.pitch[0] + off;
        const uint8_t* p1 = a.y[1] + (int64_t)row * a.pitch[1] + off;
        if (nbytes == 16) {
            uint32_t d0[4], d1[4];
            load16<MODE != Y8_BYTE, VEC>(p0, d0);
            load16<MODE != Y8_BYTE, VEC>(p1, d1);
            bool same = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d0[i] = reduce8<MODE>(d0[i]);
                d1[i] = reduce8<MODE>(d1[i]);
                sad = sad_dword<MODE>(d0[i], d1[i], sad);
                same = same && d0[i] == d1[i];
            }
            if (!same) {                                               // equal groups add +1 and -1 to the same bins: nothing
                hist16<MODE>(h, d0, 1);
                hist16<MODE>(h, d1, -1);
            }
        } else {                                                       // the row's tail: nbytes / BPS samples
            for (int b = 0; b < nbytes; b += BPS) {
                const int v0 = sample8<MODE>(p0 + b), v1 = sample8<MODE>(p1 + b);
                if (v0 != v1) {
                    sad += (uint32_t)abs(v0 - v1);
                    atomicAdd(&h[v0], 1);
                    atomicAdd(&h[v1], -1);
                }
            }
        }
    }
    atomicAdd(&wg_sad, (unsigned long long)sad);
    __syncthreads();
    int v = 0;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) v += hist[w][tid];              // SK_THREADS == 256 bins
    if (v) atomicAdd(reinterpret_cast<int*>(a.state + STATE_HIST_OFFSET) + tid, v);
    if (tid == 0 && wg_sad) atomicAdd(reinterpret_cast<unsigned long long*>(a.state + STATE_SAD_OFFSET), wg_sad);
}

__global__ __launch_bounds__(SK_THREADS) void scene_decide_kernel(uint8_t* state, int H, int W, int sad_permille, int hist_permille) {
    __shared__ uint32_t dist;
    if (threadIdx.x == 0) dist = 0;
    __syncthreads();
    const int v = reinterpret_cast<const int*>(state + STATE_HIST_OFFSET)[threadIdx.x];
    if (v) atomicAdd(&dist, (uint32_t)abs(v));
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t sad = *reinterpret_cast<const uint64_t*>(state + STATE_SAD_OFFSET);
        const uint64_t hw = (uint64_t)H * (uint64_t)W;
        fldr_scene_result* r = reinterpret_cast<fldr_scene_result*>(state);
        r->sad = sad;
        r->hist_dist = dist;
        r->cut = (sad * 1000ull >= (uint64_t)sad_permille * 255ull * hw && (uint64_t)dist * 1000ull >= (uint64_t)hist_permille * 2ull * hw) ? 1u : 0u;
        for (int i = 0; i < 4; ++i) r->reserved[i] = 0u;
    }
}

int scene_measure(const void* y0, int64_t pitch0, const void* y1, int64_t pitch1, int H, int W, int mode, int sad_permille, int hist_permille,
                  void* state, hipStream_t stream) {
    MeasureArgs a;
    a.y[0] = (const uint8_t*)y0; a.y[1] = (const uint8_t*)y1;
    a.pitch[0] = pitch0; a.pitch[1] = pitch1;
    a.row_bytes = luma_row_bytes(W, mode);
    a.chunks = (uint32_t)((a.row_bytes + 15) / 16);
    a.items = (uint32_t)H * a.chunks;
    a.state = (uint8_t*)state;
    const bool vec = luma_vec_ok(y0, pitch0, y1, pitch1);
    const uint32_t blocks = min((a.items + SK_THREADS - 1) / SK_THREADS, (uint32_t)SK_MAX_BLOCKS);
    scene_zero_kernel<<<1, SK_THREADS, 0, stream>>>(a.state);
    SAMPLE16_LAUNCH(scene_accumulate_kernel, mode, vec, blocks, SK_THREADS, stream, a);
    scene_decide_kernel<<<1, SK_THREADS, 0, stream>>>(a.state, H, W, sad_permille, hist_permille);
    return (int)hipGetLastError();
}

// ---- the select --------------------------------------------------------------------------------------------------------------------
struct SelectArgs {
    const uint8_t* in[2][3];
    int64_t in_pitch[2][3];
    uint8_t* out[SELECT_MAX_OUT][3];
    int64_t out_pitch[SELECT_MAX_OUT][3];
    int64_t row_bytes[3];
    int rows[3];
    int np;
    const float* t;
    const fldr_scene_result* result;
};

// grid: (row walkers, outputs).  A workgroup copies whole rows; 16 bytes per lane where the row's two addresses allow.
__global__ __launch_bounds__(SK_THREADS) void select_on_cut_kernel(SelectArgs a) {
    if (a.result->cut == 0u) return;
    const int k = blockIdx.y;
    const int src = a.t[k] < 0.5f ? 0 : 1;
    const int total = a.rows[0] + a.rows[1] + (a.np > 2 ? a.rows[2] : 0);
    for (int row = blockIdx.x; row < total; row += gridDim.x) {
        int p = 0, r = row;
        if (r >= a.rows[0]) { r -= a.rows[0]; p = 1; if (r >= a.rows[1]) { r -= a.rows[1]; p = 2; } }
        const uint8_t* s = a.in[src][p] + (int64_t)r * a.in_pitch[src][p];
        uint8_t* d = a.out[k][p] + (int64_t)r * a.out_pitch[k][p];
        const int64_t rb = a.row_bytes[p];
        int64_t done = 0;
        if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
            done = rb & ~(int64_t)15;
            for (int64_t x = 16ll * threadIdx.x; x < done; x += 16ll * SK_THREADS)
                *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(s + x);
        }
        for (int64_t x = done + threadIdx.x; x < rb; x += SK_THREADS) d[x] = s[x];
    }
}

int select_on_cut(const void* state, const float* t, const fldr_video_frame in[2], const fldr_video_frame* out, int n, int np,
                  const int64_t row_bytes[3], const int rows[3], hipStream_t stream) {
    SelectArgs a;
    for (int f = 0; f < 2; ++f)
        for (int p = 0; p < 3; ++p) {
            a.in[f][p] = p < np ? (const uint8_t*)in[f].plane[p] : nullptr;
            a.in_pitch[f][p] = p < np ? in[f].pitch[p] : 0;
        }
    for (int k = 0; k < SELECT_MAX_OUT; ++k)
        for (int p = 0; p < 3; ++p) {
            a.out[k][p] = (k < n && p < np) ? (uint8_t*)out[k].plane[p] : nullptr;
            a.out_pitch[k][p] = (k < n && p < np) ? out[k].pitch[p] : 0;
        }
    int total = 0;
    for (int p = 0; p < 3; ++p) { a.row_bytes[p] = p < np ? row_bytes[p] : 0; a.rows[p] = p < np ? rows[p] : 0; total += a.rows[p]; }
    a.np = np;
    a.t = t;
    a.result = (const fldr_scene_result*)state;
    select_on_cut_kernel<<<dim3((unsigned)min(total, 1024), (unsigned)n), SK_THREADS, 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace fldr_rate_impl
