// The kernels of libfldr_probe.so: the probe measure (zero, reduce every tile, write the result).
//
// A bandwidth kernel in the manner of ../pulldown/pulldown_kernels.hip, with the same lane layout: one pass, one 64-lane wave per
// 32 rows x 64 bytes of luma — two tiles side by side at depth 8, one tile at depth 10.  A lane takes one row PAIR (an even row and the
// odd row below it) and one 16-byte group of it: lane = 4 * pair + group, so four lanes read 64 contiguous bytes of a row and the four
// waves of a workgroup 256.  Per lane six 16-byte loads: the pair's two rows of cur, prev and next; every byte of the three planes is
// loaded once.  The line of cur above the pair and the line below it — a and b of the comb and order measures — are the neighbouring
// pairs' rows and come from their lanes' registers (lane -+ 4); only the first and the last pair of a tile load theirs, the halo rows
// that belong to the tiles above and below.  From those registers every word comes out: an even row is an "other" row for the anchor
// parity 1 and a row of field 0, an odd row the reverse, so both anchors' comb counts, both fields' SADs and the six order sums cost no
// further load.  The 16-byte loads need every plane address and pitch 16-byte aligned (VEC); the same arithmetic runs on per-sample
// loads otherwise, and on the bytes of a row behind its last whole 16 in either form; bytes past a row's end, and the rows of a frame
// that is not given, enter as 0 in every plane, where no sample is combed and nothing differs (a missing frame's words are zeroed by the
// result kernel).
// A tile's counts are reduced inside its wave (over the lane bits that do not tell its two tiles apart), the three comb counts of one
// anchor packed ten bits each into one word (a tile's count is at most 512); each lane keeps the sums, the maximum keys and the moving
// counts of its tiles in registers, and its own share of the order sums, which need no tile.  What becomes of those words — the keys,
// the workgroup's slot of the state, the atomics, the grid — is the tile reduce of ../rate/tile_reduce_device.h, here with N_SUMS sums,
// N_KEYS keys and N_COUNTS counts; the meeting of the waves in LDS and the result kernel's gather, which it describes, are written out
// below.  No float anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "probe_internal.h"

namespace fldr_probe_impl {

#define PB_THREADS THREADS
#define PB_WAVES WAVES
#define PB_TILE FLDR_PROBE_TILE
#define PB_WAVE_BYTES 64         // of a row, per wave

struct ProbeArgs {
    const uint8_t* cur; const uint8_t* prev; const uint8_t* next;
    int64_t pitch_cur, pitch_prev, pitch_next;
    int64_t row_bytes;
    int H;
    uint32_t tiles_x, tiles_y, cols;   // ceil(W / 32), ceil(H / 32), ceil(row_bytes / 64)
    int thresh2;                       // comb_thresh squared
    uint32_t tile_sad_min, frame_tile_sad_min;
    uint8_t* state;
};

__global__ __launch_bounds__(PB_THREADS) void probe_zero_kernel(uint8_t* state) { zero_state<FLDR_PROBE_STATE_BYTES>(state); }

// One row of one group: a and b the lines of cur above and below it, m0 / m1 / m2 the row itself in cur, prev and next.  Returns the
// three candidates' combed samples, ten bits each, and adds |a + b - 2 m| of each candidate to l0 / l1 / l2.
template <int MODE> __device__ __forceinline__ uint32_t row16(const uint32_t a[4], const uint32_t b[4], const uint32_t m0[4], const uint32_t m1[4],
                                                              const uint32_t m2[4], int thresh2, uint32_t& l0, uint32_t& l1, uint32_t& l2) {
    constexpr int STEP = MODE == Y8_BYTE ? 8 : 16;
    uint32_t n0 = 0, n1 = 0, n2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int sh = 0; sh < 32; sh += STEP) {
            const int va = (int)((a[i] >> sh) & 0xffu), vb = (int)((b[i] >> sh) & 0xffu);
            const int a0 = va - (int)((m0[i] >> sh) & 0xffu), b0 = vb - (int)((m0[i] >> sh) & 0xffu);
            const int a1 = va - (int)((m1[i] >> sh) & 0xffu), b1 = vb - (int)((m1[i] >> sh) & 0xffu);
            const int a2 = va - (int)((m2[i] >> sh) & 0xffu), b2 = vb - (int)((m2[i] >> sh) & 0xffu);
            n0 += a0 * b0 > thresh2 ? 1u : 0u;
            n1 += a1 * b1 > thresh2 ? 1u : 0u;
            n2 += a2 * b2 > thresh2 ? 1u : 0u;
            l0 += (uint32_t)(a0 + b0 < 0 ? -(a0 + b0) : a0 + b0);
            l1 += (uint32_t)(a1 + b1 < 0 ? -(a1 + b1) : a1 + b1);
            l2 += (uint32_t)(a2 + b2 < 0 ? -(a2 + b2) : a2 + b2);
        }
    return n0 | (n1 << 10) | (n2 << 20);
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(PB_THREADS) void probe_tiles_kernel(ProbeArgs a) {
    constexpr int TPW = MODE == Y8_BYTE ? 2 : 1;                       // tiles per wave: 64 bytes of a row are 64 or 32 samples
    constexpr bool WORDS = MODE != Y8_BYTE;
    __shared__ unsigned long long w_sum[PB_WAVES][N_SUMS], w_key[PB_WAVES][N_KEYS];
    __shared__ uint32_t w_count[PB_WAVES][N_COUNTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = lane & 3, pair = lane >> 2;
    unsigned long long sum[N_SUMS], key[N_KEYS];
    uint32_t count[N_COUNTS] = { 0u, 0u, 0u };
#pragma unroll
    for (int j = 0; j < N_SUMS; ++j) sum[j] = 0ull;
#pragma unroll
    for (int j = 0; j < N_KEYS; ++j) key[j] = 0ull;
    // grid: (walkers of a tile row, each four waves wide; walkers of the tile rows).  ty, col and the trip counts are wave-uniform.
    for (uint32_t ty = blockIdx.y; ty < a.tiles_y; ty += gridDim.y)
    for (uint32_t col = blockIdx.x * PB_WAVES + wave; col < a.cols; col += gridDim.x * PB_WAVES) {
        const int64_t off = (int64_t)col * PB_WAVE_BYTES + 16 * group;
        const int64_t left = a.row_bytes - off;                        // bytes of the row from this group on
        const int row0 = (int)ty * PB_TILE + 2 * pair;                 // even; H is even: a pair is inside the frame or outside it
        const bool live = row0 < a.H && left > 0;
        uint32_t C0[4], C1[4], P0[4], P1[4], N0[4], N1[4];             // y8 of the pair's even and odd row in cur, prev, next
        if (live && left >= 16 && a.prev && a.next) {
            // the common case — a whole group, all three frames given —: the six loads go out together
            load16<WORDS, VEC>(a.cur + (int64_t)row0 * a.pitch_cur + off, C0);
            load16<WORDS, VEC>(a.cur + (int64_t)(row0 + 1) * a.pitch_cur + off, C1);
            load16<WORDS, VEC>(a.prev + (int64_t)row0 * a.pitch_prev + off, P0);
            load16<WORDS, VEC>(a.prev + (int64_t)(row0 + 1) * a.pitch_prev + off, P1);
            load16<WORDS, VEC>(a.next + (int64_t)row0 * a.pitch_next + off, N0);
            load16<WORDS, VEC>(a.next + (int64_t)(row0 + 1) * a.pitch_next + off, N1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                C0[i] = reduce8<MODE>(C0[i]); C1[i] = reduce8<MODE>(C1[i]); P0[i] = reduce8<MODE>(P0[i]);
                P1[i] = reduce8<MODE>(P1[i]); N0[i] = reduce8<MODE>(N0[i]); N1[i] = reduce8<MODE>(N1[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) C0[i] = C1[i] = P0[i] = P1[i] = N0[i] = N1[i] = 0u;
            if (live) {
                fetch<MODE, VEC>(a.cur + (int64_t)row0 * a.pitch_cur + off, left, C0);
                fetch<MODE, VEC>(a.cur + (int64_t)(row0 + 1) * a.pitch_cur + off, left, C1);
                if (a.prev) {
                    fetch<MODE, VEC>(a.prev + (int64_t)row0 * a.pitch_prev + off, left, P0);
                    fetch<MODE, VEC>(a.prev + (int64_t)(row0 + 1) * a.pitch_prev + off, left, P1);
                }
                if (a.next) {
                    fetch<MODE, VEC>(a.next + (int64_t)row0 * a.pitch_next + off, left, N0);
                    fetch<MODE, VEC>(a.next + (int64_t)(row0 + 1) * a.pitch_next + off, left, N1);
                }
            }
        }
        // the line above the even row and the line below the odd row: the neighbouring pairs' (every lane takes part), but for the
        // tile's first and last pair, which load the halo row where the frame has one
        uint32_t up[4], dn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            up[i] = (uint32_t)__shfl_up((int)C1[i], 4, 64);
            dn[i] = (uint32_t)__shfl_down((int)C0[i], 4, 64);
        }
        if (pair == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) up[i] = 0u;
            if (live && row0 >= 1) fetch<MODE, VEC>(a.cur + (int64_t)(row0 - 1) * a.pitch_cur + off, left, up);
        }
        if (pair == PB_TILE / 2 - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dn[i] = 0u;
            if (live && row0 + 2 < a.H) fetch<MODE, VEC>(a.cur + (int64_t)(row0 + 2) * a.pitch_cur + off, left, dn);
        }
        // cnt[0]: the odd row's combed samples (anchor parity 0), cnt[1]: the even row's (anchor parity 1), cnt[2], cnt[3]: the SAD of
        // the even and the odd row; lp[2 k + p]: the order sums.  Rows 0 and H - 1 have no line on one side: SAD only.
        uint32_t cnt[4] = { 0u, 0u, 0u, 0u }, lp[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
        if (live && row0 >= 1) cnt[1] = row16<MODE>(up, C1, C0, P0, N0, a.thresh2, lp[0], lp[2], lp[4]);
        if (live && row0 + 2 < a.H) cnt[0] = row16<MODE>(C0, dn, C1, P1, N1, a.thresh2, lp[1], lp[3], lp[5]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cnt[2] = sad_dword<MODE>(C0[i], P0[i], cnt[2]);
            cnt[3] = sad_dword<MODE>(C1[i], P1[i], cnt[3]);
        }
        const uint32_t tx = col * TPW + (TPW == 2 ? (uint32_t)(group >> 1) : 0u);
        const bool exists = tx < a.tiles_x;                            // the second tile of the last wave column may lie past the frame
        const unsigned long long low = key_low(ty * a.tiles_x + tx);
        uint32_t t[4], v[N_KEYS];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = tile_sum<TPW == 1>(cnt[k]);    // the tile's counts, in every lane of the tile
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 * q + k] = (t[q] >> (10 * k)) & 0x3ffu;
        v[6] = t[2]; v[7] = t[3];
#pragma unroll
        for (int j = 0; j < N_KEYS; ++j) {
            sum[j] += v[j];
            key[j] = max64(key[j], exists ? pack_key(v[j], low) : 0ull);
        }
        count[0] += exists && v[6] >= a.tile_sad_min ? 1u : 0u;
        count[1] += exists && v[7] >= a.tile_sad_min ? 1u : 0u;
        count[2] += exists && v[6] + v[7] >= a.frame_tile_sad_min ? 1u : 0u;
#pragma unroll
        for (int j = 0; j < 6; ++j) sum[N_KEYS + j] += lp[j];          // the lane's own share: summed over the wave at the end
    }
    if (TPW == 2) {                                                    // lanes 0 and 2 hold the two tile columns of the wave
#pragma unroll
        for (int j = 0; j < N_KEYS; ++j) {
            sum[j] += __shfl_xor(sum[j], 2, 64);
            key[j] = max64(key[j], __shfl_xor(key[j], 2, 64));
        }
#pragma unroll
        for (int j = 0; j < N_COUNTS; ++j) count[j] += (uint32_t)__shfl_xor((int)count[j], 2, 64);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int j = N_KEYS; j < N_SUMS; ++j) sum[j] += __shfl_xor(sum[j], m, 64);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < N_SUMS; ++j) w_sum[wave][j] = sum[j];
#pragma unroll
        for (int j = 0; j < N_KEYS; ++j) w_key[wave][j] = key[j];
#pragma unroll
        for (int j = 0; j < N_COUNTS; ++j) w_count[wave][j] = count[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < PB_WAVES; ++w) {
#pragma unroll
            for (int j = 0; j < N_SUMS; ++j) sum[j] += w_sum[w][j];
#pragma unroll
            for (int j = 0; j < N_KEYS; ++j) key[j] = max64(key[j], w_key[w][j]);
#pragma unroll
            for (int j = 0; j < N_COUNTS; ++j) count[j] += w_count[w][j];
        }
        uint8_t* slot = slot_of<STATE_SLOT_BYTES>(a.state);
        slot_add_all<N_SUMS, N_KEYS, N_COUNTS>(slot_u64(slot, SLOT_SUM_OFFSET), slot_u64(slot, SLOT_KEY_OFFSET),
                                               reinterpret_cast<uint32_t*>(slot + SLOT_COUNT_OFFSET), sum, key, count);
    }
}

// one wave: lane l >= 1 takes slot l (line 0 of the state is the result), the wave combines them, lane 0 writes
__global__ __launch_bounds__(64) void probe_result_kernel(uint8_t* state, int has_prev, int has_next) {
    static_assert(STATE_SLOT_BYTES * (SLOTS + 1) == FLDR_PROBE_STATE_BYTES, "one slot per lane but lane 0");
    const int lane = threadIdx.x;
    const uint8_t* slot = state + STATE_SLOT_BYTES * lane;
    unsigned long long sum[N_SUMS], key[N_KEYS];
    uint32_t count[N_COUNTS];
#pragma unroll
    for (int j = 0; j < N_SUMS; ++j) sum[j] = lane ? reinterpret_cast<const unsigned long long*>(slot + SLOT_SUM_OFFSET)[j] : 0ull;
#pragma unroll
    for (int j = 0; j < N_KEYS; ++j) key[j] = lane ? reinterpret_cast<const unsigned long long*>(slot + SLOT_KEY_OFFSET)[j] : 0ull;
#pragma unroll
    for (int j = 0; j < N_COUNTS; ++j) count[j] = lane ? reinterpret_cast<const uint32_t*>(slot + SLOT_COUNT_OFFSET)[j] : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int j = 0; j < N_SUMS; ++j) sum[j] += __shfl_xor(sum[j], m, 64);
#pragma unroll
        for (int j = 0; j < N_KEYS; ++j) key[j] = max64(key[j], __shfl_xor(key[j], m, 64));
#pragma unroll
        for (int j = 0; j < N_COUNTS; ++j) count[j] += (uint32_t)__shfl_xor((int)count[j], m, 64);
    }
    if (lane != 0) return;
    fldr_probe_result* r = reinterpret_cast<fldr_probe_result*>(state);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool given = k == FLDR_PROBE_C || (k == FLDR_PROBE_P ? has_prev : has_next);
            const int j = 3 * q + k;
            r->comb[q][k] = given ? sum[j] : 0ull;
            r->max_tile_comb[q][k] = given ? key_value(key[j]) : 0u;
            r->max_tile[q][k] = given ? key_index(key[j]) : 0u;
        }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        r->field_sad[p] = has_prev ? sum[6 + p] : 0ull;
        r->field_max_tile_sad[p] = has_prev ? key_value(key[6 + p]) : 0u;
        r->field_max_tile[p] = has_prev ? key_index(key[6 + p]) : 0u;
        r->field_moving_tiles[p] = has_prev ? count[p] : 0u;
    }
    r->frame_moving_tiles = has_prev ? count[2] : 0u;
    r->repeat = has_prev && count[2] == 0u ? 1u : 0u;
    unsigned long long lap[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool given = k == FLDR_PROBE_C || (k == FLDR_PROBE_P ? has_prev : has_next);
            lap[k][p] = given ? sum[N_KEYS + 2 * k + p] : 0ull;
            r->lap[k][p] = lap[k][p];
        }
    const bool both = has_prev && has_next;
    r->tff_sum = both ? lap[FLDR_PROBE_P][1] + lap[FLDR_PROBE_N][0] : 0ull;
    r->bff_sum = both ? lap[FLDR_PROBE_P][0] + lap[FLDR_PROBE_N][1] : 0ull;
#pragma unroll
    for (int i = 0; i < 12; ++i) r->reserved[i] = 0u;
}

int probe_measure(const MeasureCall& c, void* state, hipStream_t stream) {
    ProbeArgs a;
    a.cur = (const uint8_t*)c.cur; a.prev = (const uint8_t*)c.prev; a.next = (const uint8_t*)c.next;
    a.pitch_cur = c.pitch_cur; a.pitch_prev = c.prev ? c.pitch_prev : 0; a.pitch_next = c.next ? c.pitch_next : 0;
    a.row_bytes = luma_row_bytes(c.W, c.mode);
    a.H = c.H;
    a.tiles_x = tiles_of(c.W, PB_TILE);
    a.tiles_y = tiles_of(c.H, PB_TILE);
    a.cols = (uint32_t)((a.row_bytes + PB_WAVE_BYTES - 1) / PB_WAVE_BYTES);
    a.thresh2 = c.comb_thresh * c.comb_thresh;
    a.tile_sad_min = (uint32_t)c.tile_sad_min;
    a.frame_tile_sad_min = (uint32_t)c.frame_tile_sad_min;
    a.state = (uint8_t*)state;
    const bool vec = luma_vec_ok3(c.cur, a.pitch_cur, c.prev, a.pitch_prev, c.next, a.pitch_next);
    const dim3 blocks = tile_grid(a.cols, a.tiles_y);
    probe_zero_kernel<<<1, PB_THREADS, 0, stream>>>(a.state);
    SAMPLE16_LAUNCH(probe_tiles_kernel, c.mode, vec, blocks, PB_THREADS, stream, a);
    probe_result_kernel<<<1, 64, 0, stream>>>(a.state, c.prev ? 1 : 0, c.next ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace fldr_probe_impl
