// The kernels of libfldr_cadence.so: the repeat measure of a frame pair (zero, reduce every tile, write the result).
//
// The measure is a bandwidth kernel: one pass over the two luma planes, one 64-lane wave per tile of 32 x 32 samples.  At depth 8 a
// tile is 32 rows of 32 bytes = 64 groups of 16 bytes: one group, one 16-byte load per frame, for every lane.  At depth 10 a tile is
// 32 rows of 64 bytes: two groups per lane.  The four waves of a workgroup take four tiles that lie side by side, so together they
// read whole 128-byte lines of each row.  The 16-byte loads need both plane addresses and pitches 16-byte aligned (VEC); the same
// arithmetic runs on per-sample loads otherwise, and the bytes of a row behind its last whole 16 go sample by sample in either form.
// Per 16 bytes: v_sad_u8 on the dwords (depth 8) or v_sad_u16 on the words reduced to 8 bits (depth 10).  A tile's sum is reduced
// inside its wave; each wave keeps the sum, the maximum key and the count of its tiles in registers.  What becomes of those three
// words — the key, the workgroup's slot of the state, the atomics, the grid — is the tile reduce of ../rate/tile_reduce_device.h,
// here with one sum, one key and one count; the meeting of the waves in LDS and the result kernel's gather, which it describes, are
// written out below.  No float anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cadence_internal.h"

namespace fldr_cadence_impl {

#define RK_THREADS THREADS
#define RK_WAVES WAVES
#define RK_TILE FLDR_REPEAT_TILE

struct RepeatArgs {
    const uint8_t* y[2];
    int64_t pitch[2];
    int64_t row_bytes;
    int H;
    uint32_t tiles_x, tiles_y;   // ceil(W / 32), ceil(H / 32)
    uint32_t tile_sad_min;
    uint8_t* state;
};

__global__ __launch_bounds__(RK_THREADS) void repeat_zero_kernel(uint8_t* state) { zero_state<FLDR_REPEAT_STATE_BYTES>(state); }

template <int MODE, bool VEC>
__global__ __launch_bounds__(RK_THREADS) void repeat_tiles_kernel(RepeatArgs a) {
    constexpr int BPS = MODE == Y8_BYTE ? 1 : 2;
    constexpr int GROUPS = BPS;                                        // 16-byte groups per lane and tile: 64 x GROUPS x 16 = 32 x 32 x BPS
    constexpr int GROUPS_PER_ROW = 2 * BPS;
    __shared__ unsigned long long w_sad[RK_WAVES], w_key[RK_WAVES];
    __shared__ uint32_t w_moving[RK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long sum = 0, key = 0;                               // of this wave's tiles; the same in every lane
    uint32_t moving = 0;
    // grid: (walkers of a tile row, each four tiles wide; walkers of the tile rows).  ty, tx and the trip counts are wave-uniform.
    for (uint32_t ty = blockIdx.y; ty < a.tiles_y; ty += gridDim.y)
    for (uint32_t tx = blockIdx.x * RK_WAVES + wave; tx < a.tiles_x; tx += gridDim.x * RK_WAVES) {
        const uint32_t tile = ty * a.tiles_x + tx;
        uint32_t sad = 0;                                              // <= 255 x 16 x GROUPS
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int idx = lane + 64 * g;
            const int row = (int)ty * RK_TILE + idx / GROUPS_PER_ROW;
            const int64_t off = (int64_t)tx * (RK_TILE * BPS) + 16 * (idx % GROUPS_PER_ROW);
            const int64_t left = a.row_bytes - off;                    // bytes of the row from this group on
            if (row >= a.H || left <= 0) continue;
            const uint8_t* p0 = a.y[0] + (int64_t)row * a.pitch[0] + off;
            const uint8_t* p1 = a.y[1] + (int64_t)row * a.pitch[1] + off;
            if (left >= 16) {
                uint32_t d0[4], d1[4];
                load16<MODE != Y8_BYTE, VEC>(p0, d0);
                load16<MODE != Y8_BYTE, VEC>(p1, d1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t u = reduce8<MODE>(d0[i]), v = reduce8<MODE>(d1[i]);
                    sad = sad_dword<MODE>(u, v, sad);
                }
            } else {                                                   // the row's tail: left / BPS samples
                for (int b = 0; b < (int)left; b += BPS) sad += (uint32_t)abs(sample8<MODE>(p0 + b) - sample8<MODE>(p1 + b));
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sad += (uint32_t)__shfl_xor((int)sad, m, 64);      // the tile's sum, in every lane
        sum += sad;
        key = max64(pack_key(sad, key_low(tile)), key);
        moving += sad >= a.tile_sad_min ? 1u : 0u;
    }
    if (lane == 0) { w_sad[wave] = sum; w_key[wave] = key; w_moving[wave] = moving; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < RK_WAVES; ++w) {
            sum += w_sad[w];
            key = max64(w_key[w], key);
            moving += w_moving[w];
        }
        uint8_t* slot = slot_of<STATE_SLOT_BYTES>(a.state);
        slot_add(slot_u64(slot, SLOT_SAD_OFFSET), sum);
        slot_max(slot_u64(slot, SLOT_KEY_OFFSET), key);
        slot_add(reinterpret_cast<uint32_t*>(slot + SLOT_MOVING_OFFSET), moving);
    }
}

// one wave: lane l >= 1 takes slot l (line 0 of the state is the result), the wave combines them, lane 0 writes
__global__ __launch_bounds__(64) void repeat_result_kernel(uint8_t* state) {
    static_assert(STATE_SLOT_BYTES * (SLOTS + 1) == FLDR_REPEAT_STATE_BYTES, "one slot per lane but lane 0");
    const int lane = threadIdx.x;
    const uint8_t* slot = state + STATE_SLOT_BYTES * lane;
    unsigned long long sad = lane ? *reinterpret_cast<const unsigned long long*>(slot + SLOT_SAD_OFFSET) : 0ull;
    unsigned long long key = lane ? *reinterpret_cast<const unsigned long long*>(slot + SLOT_KEY_OFFSET) : 0ull;
    uint32_t moving = lane ? *reinterpret_cast<const uint32_t*>(slot + SLOT_MOVING_OFFSET) : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sad += __shfl_xor(sad, m, 64);
        key = max64(__shfl_xor(key, m, 64), key);
        moving += (uint32_t)__shfl_xor((int)moving, m, 64);
    }
    if (lane != 0) return;
    fldr_repeat_result* r = reinterpret_cast<fldr_repeat_result*>(state);
    r->sad = sad;
    r->max_tile_sad = key_value(key);
    r->max_tile = key_index(key);
    r->moving_tiles = moving;
    r->repeat = moving == 0u ? 1u : 0u;
    r->reserved[0] = r->reserved[1] = 0u;
}

int repeat_measure(const void* y0, int64_t pitch0, const void* y1, int64_t pitch1, int H, int W, int mode, int tile_sad_min, void* state,
                   hipStream_t stream) {
    RepeatArgs a;
    a.y[0] = (const uint8_t*)y0; a.y[1] = (const uint8_t*)y1;
    a.pitch[0] = pitch0; a.pitch[1] = pitch1;
    a.row_bytes = luma_row_bytes(W, mode);
    a.H = H;
    a.tiles_x = tiles_of(W, RK_TILE);
    a.tiles_y = tiles_of(H, RK_TILE);
    a.tile_sad_min = (uint32_t)tile_sad_min;
    a.state = (uint8_t*)state;
    const bool vec = luma_vec_ok(y0, pitch0, y1, pitch1);
    const dim3 blocks = tile_grid(a.tiles_x, a.tiles_y);                // a wave's column is a tile
    repeat_zero_kernel<<<1, RK_THREADS, 0, stream>>>(a.state);
    SAMPLE16_LAUNCH(repeat_tiles_kernel, mode, vec, blocks, RK_THREADS, stream, a);
    repeat_result_kernel<<<1, 64, 0, stream>>>(a.state);
    return (int)hipGetLastError();
}

}  // namespace fldr_cadence_impl
