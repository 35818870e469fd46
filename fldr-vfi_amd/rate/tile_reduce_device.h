// The tile reduce of the luma measure kernels above the rate library (repeat_tiles_kernel, pulldown_tiles_kernel, probe_tiles_kernel and
// their zero and result kernels), written once and inlined into each: a measure counts something per tile of 32 x 32 luma samples and
// wants, over the frame, integer sums, maxima with the tile they occur in, and counts of tiles over a threshold.
//
// A workgroup is THREADS lanes, WAVES waves that walk the tiles with the grid's strides (tile_grid); each lane keeps sums, maximum keys
// and counts of its tiles in registers (arrays of NS, NK and NC words).  A key is (value << 32) | (0xffffffff - index), so the maximum
// of the keys is the largest value and, among equal values, the lowest index; a wave without a tile holds key 0, below every tile's key
// (the low word of a key is never 0: index < 2^31, which the host checks).  At the end the waves of a workgroup meet in LDS and one
// lane adds the workgroup's words to memory with integer atomics (slot_add, slot_max).  Not to one address for the whole grid (2040
// workgroups at 3840 x 2160): the state is SLOTS + 1 lines of SLOT_BYTES each, line 0 begins with the result the caller reads, workgroup
// b adds to line 1 + b % SLOTS (slot_of), and the one-wave result kernel reads line l in lane l (slot_load) and combines the lanes
// (wave_combine).  Every word is an integer sum, maximum or count, so the order of the atomics does not show in the result.
// INTEGRATION.md section 3h has the measurement of one address against the slots.  What is counted, where a lane's bytes lie and what the
// result struct holds stay with the including kernel — and so do two short pieces of each tiles kernel, the meeting of a wave's two tile
// columns (one xor step over lane bit 1) and the meeting of the waves in LDS: written as calls of functions that change the lanes'
// arrays in place they compile to the same instructions in another order (DESIGN_LOG.md has the listings), and the tiles kernels are
// held to their instruction streams.  For the same reason slot_load and wave_combine serve pulldown_result_kernel alone: the repeat and
// probe result kernels measured 0.1 and 0.4 µs slower with them and keep their own loops (DESIGN_LOG.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "luma8_device.h"

namespace fldr_tile_reduce {
using namespace fldr_luma8;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 2048;       // 8 workgroups per CU of an MI355X; larger frames walk with the grid's strides
constexpr int SLOTS = 63;              // one per lane of the result kernel but lane 0

// y8 of the 16 bytes at p, each in its sample's low byte, of which `left` (> 0) lie in the row; the others read as 0
template <int MODE, bool VEC> __device__ __forceinline__ void fetch(const uint8_t* p, int64_t left, uint32_t r[4]) {
    constexpr int BPS = MODE == Y8_BYTE ? 1 : 2;
    if (left >= 16) {
        uint32_t d[4];
        load16<MODE != Y8_BYTE, VEC>(p, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = reduce8<MODE>(d[i]);
    } else {                                                           // the row's tail: left / BPS samples
        const int last = (int)left - BPS;                              // a sample past the end reads the row's last one instead, and counts as 0
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = 0u;
#pragma unroll
        for (int b = 0; b < 16; b += BPS) {
            const uint32_t v = (uint32_t)sample8<MODE>(p + (b < last ? b : last));
            r[b >> 2] |= (b <= last ? v : 0u) << (8 * (b & 3));
        }
    }
}

// the sum over the lanes of a wave that share a tile, where a lane is 4 * row pair + 16-byte group of a 64-byte row: all 64 lanes at
// depth 10, the 32 with the same bit 1 at depth 8
template <bool WHOLE> __device__ __forceinline__ uint32_t tile_sum(uint32_t v) {
    v += (uint32_t)__shfl_xor((int)v, 32, 64);
    v += (uint32_t)__shfl_xor((int)v, 16, 64);
    v += (uint32_t)__shfl_xor((int)v, 8, 64);
    v += (uint32_t)__shfl_xor((int)v, 4, 64);
    v += (uint32_t)__shfl_xor((int)v, 1, 64);
    if (WHOLE) v += (uint32_t)__shfl_xor((int)v, 2, 64);
    return v;
}

__device__ __forceinline__ unsigned long long max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---- keys ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long key_low(uint32_t index) { return (unsigned long long)(0xffffffffu - index); }
__device__ __forceinline__ unsigned long long pack_key(uint32_t value, unsigned long long low) { return ((unsigned long long)value << 32) | low; }
__device__ __forceinline__ uint32_t key_value(unsigned long long key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ uint32_t key_index(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// ---- lanes, waves, workgroups ------------------------------------------------------------------------------------------------------------
// one step of a butterfly over the lanes: every word meets that of lane ^ m
template <int NS, int NK, int NC>
__device__ __forceinline__ void xor_step(unsigned long long* sum, unsigned long long* key, uint32_t* count, int m) {
#pragma unroll
    for (int j = 0; j < (NS > NK ? NS : NK); ++j) {
        if (j < NS) sum[j] += __shfl_xor(sum[j], m, 64);
        if (j < NK) key[j] = max64(key[j], __shfl_xor(key[j], m, 64));
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) count[j] += (uint32_t)__shfl_xor((int)count[j], m, 64);
}

// all 64 lanes: the result kernels' combine of the slots
template <int NS, int NK, int NC> __device__ __forceinline__ void wave_combine(unsigned long long* sum, unsigned long long* key, uint32_t* count) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) xor_step<NS, NK, NC>(sum, key, count, m);
}

// ---- the state -------------------------------------------------------------------------------------------------------------------------
// the whole state of BYTES, by one workgroup of THREADS
template <int BYTES> __device__ __forceinline__ void zero_state(uint8_t* state) {
    static_assert(BYTES % (16 * THREADS) == 0, "whole uint4 per thread");
    uint4* p = reinterpret_cast<uint4*>(state);
#pragma unroll
    for (int i = 0; i < BYTES / (16 * THREADS); ++i) p[threadIdx.x + i * THREADS] = make_uint4(0u, 0u, 0u, 0u);
}

// the accumulator line of this workgroup
template <int SLOT_BYTES> __device__ __forceinline__ uint8_t* slot_of(uint8_t* state) {
    return state + SLOT_BYTES * (1 + (blockIdx.y * gridDim.x + blockIdx.x) % SLOTS);
}

__device__ __forceinline__ unsigned long long* slot_u64(uint8_t* slot, int offset) { return reinterpret_cast<unsigned long long*>(slot + offset); }

// a workgroup's sum or count -> its word of the slot (a word of 0 adds nothing and is not sent), its key -> the slot's maximum
template <class T> __device__ __forceinline__ void slot_add(T* word, T v) { if (v) atomicAdd(word, v); }
__device__ __forceinline__ void slot_max(unsigned long long* word, unsigned long long key) { atomicMax(word, key); }

// NS sums, NK keys and NC counts of a workgroup -> the words of its slot, where each kind lies in a row
template <int NS, int NK, int NC>
__device__ __forceinline__ void slot_add_all(unsigned long long* ssum, unsigned long long* skey, uint32_t* scount, const unsigned long long* sum,
                                             const unsigned long long* key, const uint32_t* count) {
#pragma unroll
    for (int j = 0; j < NS; ++j) slot_add(ssum + j, sum[j]);
#pragma unroll
    for (int j = 0; j < NK; ++j) slot_max(skey + j, key[j]);
#pragma unroll
    for (int j = 0; j < NC; ++j) slot_add(scount + j, count[j]);
}

// the result kernel's lane l >= 1 reads line l; lane 0, whose line is the result, holds zeros
template <class T, int N> __device__ __forceinline__ void slot_load(const uint8_t* words, int lane, T* v) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = lane ? reinterpret_cast<const T*>(words)[j] : (T)0;
}

// ---- the host's side ---------------------------------------------------------------------------------------------------------------------
// `cols` columns of work, one per wave, by tiles_y tile rows: every workgroup's wave 0 has a column (blockIdx.x * WAVES < cols) and a tile
// row (blockIdx.y < tiles_y)
static inline dim3 tile_grid(uint32_t cols, uint32_t tiles_y) {
    const uint32_t bx = min((cols + WAVES - 1) / WAVES, (uint32_t)MAX_BLOCKS);
    return dim3(bx, min(tiles_y, (uint32_t)MAX_BLOCKS / bx));
}

static inline uint32_t tiles_of(int n, int tile) { return (uint32_t)((n + tile - 1) / tile); }

// cur against prev and next: a missing frame decides nothing about the loads, null and pitch 0 are 16-byte aligned
static inline bool luma_vec_ok3(const void* cur, int64_t pitch_cur, const void* prev, int64_t pitch_prev, const void* next, int64_t pitch_next) {
    return luma_vec_ok(cur, pitch_cur, prev, pitch_prev) && luma_vec_ok(cur, pitch_cur, next, pitch_next);
}

}  // namespace fldr_tile_reduce
