// The kernels of libfldr_pulldown.so: the field-matching measure (zero, reduce every tile, write the result and the decision) and the
// assembly of the matched frame.
//
// The measure is a bandwidth kernel in the manner of ../cadence/cadence_kernels.hip: one pass, one 64-lane wave per 32 rows x 64 bytes
// of luma — two tiles side by side at depth 8, one tile at depth 10.  A lane takes one row PAIR (an anchor row and the other row next
// to it) and one 16-byte group of it: lane = 4 * pair + group, so four lanes read 64 contiguous bytes of a row and the four waves of a
// workgroup 256.  Per lane: the anchor row of cur and of prev (the repeat sum, v_sad_u8 / v_sad_u16 as in the repeat measure), the
// other row of cur, prev and next (the three candidates' m) and the anchor row on the far side of the other row (a and b; for the
// pair at a tile's edge that row belongs to the tile above or below).  From HBM that is cur whole, prev whole and the other rows of
// next: 2.5 luma planes; the far anchor row is a second read of bytes a neighbouring lane reads too.  The 16-byte loads need every
// plane address and pitch 16-byte aligned (VEC); the same arithmetic runs on per-sample loads otherwise, and on the bytes of a row behind
// its last whole 16 in either form; bytes past a row's end enter as 0 in every plane, where no sample is combed and nothing differs.
// The common case — a whole group of an inner pair with all three frames given — issues its six loads together; the general path
// serves the frame's first and last pair, the row tails and the calls without prev or next.
// A tile's four counts are reduced inside its wave (over the lane bits that do not tell its two tiles apart); each lane keeps the
// sums, the maximum keys and the moving count of its tiles in registers.  What becomes of those words — the keys, the workgroup's slot
// of the state, the atomics, the result kernel's gather, the grid — is the tile reduce of ../rate/tile_reduce_device.h, here with four
// sums, four keys and one count; the result kernel also takes the decision.  No float anywhere.
//
// The assembly is a copy kernel, one launch per plane: a wave takes 1024 bytes of one row, so the choice of the row's source — cur on
// the anchor rows, S_match on the others, or the line average of cur — is wave-uniform; match and combed come from the arguments or,
// for a graph that follows a rewritten measure, from two words of device memory every lane reads alike.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pulldown_internal.h"

namespace fldr_pulldown_impl {

#define PK_THREADS THREADS
#define PK_WAVES WAVES
#define PK_TILE FLDR_PULLDOWN_TILE
#define PK_WAVE_BYTES 64         // of a row, per wave

struct MeasureArgs {
    const uint8_t* cur; const uint8_t* prev; const uint8_t* next;
    int64_t pitch_cur, pitch_prev, pitch_next;
    int64_t row_bytes;
    int H, q;
    uint32_t tiles_x, tiles_y, cols;   // ceil(W / 32), ceil(H / 32), ceil(row_bytes / 64)
    int thresh2;                       // comb_thresh squared
    uint32_t tile_sad_min;
    uint8_t* state;
};

__global__ __launch_bounds__(PK_THREADS) void pulldown_zero_kernel(uint8_t* state) { zero_state<FLDR_PULLDOWN_STATE_BYTES>(state); }

// the samples of m that lie outside the span of a and b by more than the threshold on both sides
template <int MODE> __device__ __forceinline__ uint32_t combed16(const uint32_t a[4], const uint32_t b[4], const uint32_t m[4], int thresh2) {
    constexpr int STEP = MODE == Y8_BYTE ? 8 : 16;
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int sh = 0; sh < 32; sh += STEP) {
            const int va = (int)((a[i] >> sh) & 0xffu), vb = (int)((b[i] >> sh) & 0xffu), vm = (int)((m[i] >> sh) & 0xffu);
            n += (va - vm) * (vb - vm) > thresh2 ? 1u : 0u;
        }
    return n;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(PK_THREADS) void pulldown_tiles_kernel(MeasureArgs a) {
    constexpr int TPW = MODE == Y8_BYTE ? 2 : 1;                       // tiles per wave: 64 bytes of a row are 64 or 32 samples
    __shared__ unsigned long long w_sum[PK_WAVES][4], w_key[PK_WAVES][4];
    __shared__ uint32_t w_moving[PK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = lane & 3, pair = lane >> 2;
    unsigned long long sum[4] = { 0, 0, 0, 0 }, key[4] = { 0, 0, 0, 0 };   // [0..2]: the candidates' combing, [3]: the anchor rows' difference
    uint32_t moving = 0;
    // grid: (walkers of a tile row, each four waves wide; walkers of the tile rows).  ty, col and the trip counts are wave-uniform.
    for (uint32_t ty = blockIdx.y; ty < a.tiles_y; ty += gridDim.y)
    for (uint32_t col = blockIdx.x * PK_WAVES + wave; col < a.cols; col += gridDim.x * PK_WAVES) {
        const int64_t off = (int64_t)col * PK_WAVE_BYTES + 16 * group;
        const int64_t left = a.row_bytes - off;                        // bytes of the row from this group on
        const int row0 = (int)ty * PK_TILE + 2 * pair;                 // H is even: a pair is inside the frame or outside it
        uint32_t cnt[4] = { 0u, 0u, 0u, 0u };
        const int ya = row0 + a.q, y = row0 + 1 - a.q;                 // the pair's anchor row and its other row
        if (row0 < a.H && left >= 16 && y >= 1 && y <= a.H - 2 && a.prev && a.next) {
            // the common case — a whole group of an inner pair, all three frames given —: the six loads go out together
            const int yb = a.q ? y - 1 : y + 1;
            uint32_t A[4], B[4], PA[4], M0[4], M1[4], M2[4];
            load16<MODE != Y8_BYTE, VEC>(a.cur + (int64_t)ya * a.pitch_cur + off, A);
            load16<MODE != Y8_BYTE, VEC>(a.cur + (int64_t)yb * a.pitch_cur + off, B);
            load16<MODE != Y8_BYTE, VEC>(a.cur + (int64_t)y * a.pitch_cur + off, M0);
            load16<MODE != Y8_BYTE, VEC>(a.prev + (int64_t)ya * a.pitch_prev + off, PA);
            load16<MODE != Y8_BYTE, VEC>(a.prev + (int64_t)y * a.pitch_prev + off, M1);
            load16<MODE != Y8_BYTE, VEC>(a.next + (int64_t)y * a.pitch_next + off, M2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                A[i] = reduce8<MODE>(A[i]); B[i] = reduce8<MODE>(B[i]); PA[i] = reduce8<MODE>(PA[i]);
                M0[i] = reduce8<MODE>(M0[i]); M1[i] = reduce8<MODE>(M1[i]); M2[i] = reduce8<MODE>(M2[i]);
                cnt[3] = sad_dword<MODE>(A[i], PA[i], cnt[3]);
            }
            cnt[0] = combed16<MODE>(A, B, M0, a.thresh2);
            cnt[1] = combed16<MODE>(A, B, M1, a.thresh2);
            cnt[2] = combed16<MODE>(A, B, M2, a.thresh2);
        } else if (row0 < a.H && left > 0) {
            uint32_t A[4];
            fetch<MODE, VEC>(a.cur + (int64_t)ya * a.pitch_cur + off, left, A);
            if (a.prev) {
                uint32_t PA[4];
                fetch<MODE, VEC>(a.prev + (int64_t)ya * a.pitch_prev + off, left, PA);
#pragma unroll
                for (int i = 0; i < 4; ++i) cnt[3] = sad_dword<MODE>(A[i], PA[i], cnt[3]);
            }
            if (y >= 1 && y <= a.H - 2) {
                const int yb = a.q ? y - 1 : y + 1;                    // the anchor row on the other row's far side
                uint32_t B[4], M[4];
                fetch<MODE, VEC>(a.cur + (int64_t)yb * a.pitch_cur + off, left, B);
                fetch<MODE, VEC>(a.cur + (int64_t)y * a.pitch_cur + off, left, M);
                cnt[0] = combed16<MODE>(A, B, M, a.thresh2);
                if (a.prev) {
                    fetch<MODE, VEC>(a.prev + (int64_t)y * a.pitch_prev + off, left, M);
                    cnt[1] = combed16<MODE>(A, B, M, a.thresh2);
                }
                if (a.next) {
                    fetch<MODE, VEC>(a.next + (int64_t)y * a.pitch_next + off, left, M);
                    cnt[2] = combed16<MODE>(A, B, M, a.thresh2);
                }
            }
        }
        const uint32_t tx = col * TPW + (TPW == 2 ? (uint32_t)(group >> 1) : 0u);
        const bool exists = tx < a.tiles_x;                            // the second tile of the last wave column may lie past the frame
        const unsigned long long low = key_low(ty * a.tiles_x + tx);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t t = tile_sum<TPW == 1>(cnt[k]);             // the tile's count, in every lane of the tile
            sum[k] += t;
            key[k] = max64(key[k], exists ? pack_key(t, low) : 0ull);
            if (k == 3) moving += exists && t >= a.tile_sad_min ? 1u : 0u;
        }
    }
    if (TPW == 2) {                                                    // lanes 0 and 2 hold the two tile columns of the wave
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sum[k] += __shfl_xor(sum[k], 2, 64);
            key[k] = max64(key[k], __shfl_xor(key[k], 2, 64));
        }
        moving += (uint32_t)__shfl_xor((int)moving, 2, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { w_sum[wave][k] = sum[k]; w_key[wave][k] = key[k]; }
        w_moving[wave] = moving;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < PK_WAVES; ++w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { sum[k] += w_sum[w][k]; key[k] = max64(key[k], w_key[w][k]); }
            moving += w_moving[w];
        }
        // the words of a slot lie candidate by candidate, then the anchor rows': they are sent in that order
        uint8_t* slot = slot_of<STATE_SLOT_BYTES>(a.state);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            slot_add(slot_u64(slot, SLOT_COMB_OFFSET) + k, sum[k]);
            slot_max(slot_u64(slot, SLOT_KEY_OFFSET) + k, key[k]);
        }
        slot_add(slot_u64(slot, SLOT_DSAD_OFFSET), sum[3]);
        slot_max(slot_u64(slot, SLOT_DKEY_OFFSET), key[3]);
        slot_add(reinterpret_cast<uint32_t*>(slot + SLOT_DMOVING_OFFSET), moving);
    }
}

// one wave: lane l >= 1 takes slot l (line 0 of the state is the result), the wave combines them, lane 0 decides and writes
__global__ __launch_bounds__(64) void pulldown_result_kernel(uint8_t* state, int allowed, uint32_t comb_tile_min, int has_prev) {
    static_assert(STATE_SLOT_BYTES * (SLOTS + 1) == FLDR_PULLDOWN_STATE_BYTES, "one slot per lane but lane 0");
    const int lane = threadIdx.x;
    const uint8_t* slot = state + STATE_SLOT_BYTES * lane;
    unsigned long long sum[4], key[4];
    uint32_t moving;
    slot_load<unsigned long long, 3>(slot + SLOT_COMB_OFFSET, lane, sum);
    slot_load<unsigned long long, 3>(slot + SLOT_KEY_OFFSET, lane, key);
    slot_load<unsigned long long, 1>(slot + SLOT_DSAD_OFFSET, lane, sum + 3);
    slot_load<unsigned long long, 1>(slot + SLOT_DKEY_OFFSET, lane, key + 3);
    slot_load<uint32_t, 1>(slot + SLOT_DMOVING_OFFSET, lane, &moving);
    wave_combine<4, 4, 1>(sum, key, &moving);
    if (lane != 0) return;
    fldr_pulldown_result* r = reinterpret_cast<fldr_pulldown_result*>(state);
    int match = -1;
    unsigned long long best_tile = 0, best_sum = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long tile = key_value(key[k]);
        r->comb[k] = sum[k];
        r->max_tile_comb[k] = (uint32_t)tile;
        r->max_tile[k] = key_index(key[k]);
        if (!(allowed >> k & 1)) continue;
        if (match < 0 || tile < best_tile || (tile == best_tile && sum[k] < best_sum)) { match = k; best_tile = tile; best_sum = sum[k]; }   // strict: ties stay with the earlier candidate
    }
    r->match = match;
    r->combed = best_tile >= comb_tile_min ? 1u : 0u;
    r->dup_sad = sum[3];
    r->dup_max_tile_sad = key_value(key[3]);
    r->dup_max_tile = has_prev ? key_index(key[3]) : 0u;
    r->dup_moving_tiles = moving;
#pragma unroll
    for (int i = 0; i < 5; ++i) r->reserved[i] = 0u;
}

int pulldown_measure(const MeasureCall& c, void* state, hipStream_t stream) {
    MeasureArgs a;
    a.cur = (const uint8_t*)c.cur; a.prev = (const uint8_t*)c.prev; a.next = (const uint8_t*)c.next;
    a.pitch_cur = c.pitch_cur; a.pitch_prev = c.prev ? c.pitch_prev : 0; a.pitch_next = c.next ? c.pitch_next : 0;
    a.row_bytes = luma_row_bytes(c.W, c.mode);
    a.H = c.H; a.q = c.anchor;
    a.tiles_x = tiles_of(c.W, PK_TILE);
    a.tiles_y = tiles_of(c.H, PK_TILE);
    a.cols = (uint32_t)((a.row_bytes + PK_WAVE_BYTES - 1) / PK_WAVE_BYTES);
    a.thresh2 = c.comb_thresh * c.comb_thresh;
    a.tile_sad_min = (uint32_t)c.tile_sad_min;
    a.state = (uint8_t*)state;
    const bool vec = luma_vec_ok3(c.cur, a.pitch_cur, c.prev, a.pitch_prev, c.next, a.pitch_next);
    const dim3 blocks = tile_grid(a.cols, a.tiles_y);
    pulldown_zero_kernel<<<1, PK_THREADS, 0, stream>>>(a.state);
    SAMPLE16_LAUNCH(pulldown_tiles_kernel, c.mode, vec, blocks, PK_THREADS, stream, a);
    pulldown_result_kernel<<<1, 64, 0, stream>>>(a.state, c.allowed, (uint32_t)c.comb_tile_min, c.prev ? 1 : 0);
    return (int)hipGetLastError();
}

// ---- the assembly ----------------------------------------------------------------------------------------------------------------------
#define AK_ROWS 4                // waves of a workgroup, one row each
#define AK_WAVE_BYTES 1024       // 64 lanes x 16 bytes
#define AK_MAX_X 64
#define AK_MAX_Y 512

struct AssembleArgs {
    AssemblePlane p;
    int q, match, combed, post;
    const int32_t* decision;
};

// the line average of two dwords of samples, sample by sample, in the container's canonical form
template <int MODE> __device__ __forceinline__ uint32_t average_dword(uint32_t a, uint32_t b) {
    if (MODE == Y8_BYTE) {
        uint32_t o = 0;
#pragma unroll
        for (int sh = 0; sh < 32; sh += 8) o |= ((((a >> sh) & 0xffu) + ((b >> sh) & 0xffu) + 1u) >> 1) << sh;
        return o;
    }
    uint32_t o = 0;
#pragma unroll
    for (int sh = 0; sh < 32; sh += 16) {
        const uint32_t wa = (a >> sh) & 0xffffu, wb = (b >> sh) & 0xffffu;
        const uint32_t va = MODE == Y8_P010 ? wa >> 6 : wa & 0x3ffu, vb = MODE == Y8_P010 ? wb >> 6 : wb & 0x3ffu;
        const uint32_t v = (va + vb + 1u) >> 1;
        o |= (MODE == Y8_P010 ? v << 6 : v) << sh;
    }
    return o;
}

template <int MODE> __device__ __forceinline__ uint32_t average_sample(uint32_t a, uint32_t b) {   // one byte, or one word
    if (MODE == Y8_BYTE) return (a + b + 1u) >> 1;
    const uint32_t va = MODE == Y8_P010 ? a >> 6 : a & 0x3ffu, vb = MODE == Y8_P010 ? b >> 6 : b & 0x3ffu;
    const uint32_t v = (va + vb + 1u) >> 1;
    return MODE == Y8_P010 ? v << 6 : v;
}

template <int MODE> __device__ __forceinline__ uint32_t load_sample(const uint8_t* p) {
    return MODE == Y8_BYTE ? (uint32_t)*p : (uint32_t)*reinterpret_cast<const uint16_t*>(p);
}
template <int MODE> __device__ __forceinline__ void store_sample(uint8_t* p, uint32_t v) {
    if (MODE == Y8_BYTE) *p = (uint8_t)v; else *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
}

template <int MODE>
__global__ __launch_bounds__(64 * AK_ROWS) void pulldown_assemble_kernel(AssembleArgs a) {
    constexpr int BPS = MODE == Y8_BYTE ? 1 : 2;
    const AssemblePlane& P = a.p;
    int match = a.match, combed = a.combed;
    if (match < 0) {                                                   // the same two words for every lane of the grid
        match = a.decision[0];
        combed = a.decision[1];
        if ((unsigned)match > 2u) match = 0;
    }
    const bool average = a.post == FLDR_PULLDOWN_POST_AVERAGE && combed != 0;
    const uint8_t* other = match == FLDR_PULLDOWN_P ? P.prev : match == FLDR_PULLDOWN_N ? P.next : P.cur;
    const int64_t other_pitch = match == FLDR_PULLDOWN_P ? P.pitch_prev : match == FLDR_PULLDOWN_N ? P.pitch_next : P.pitch_cur;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // grid: (walkers of a row, each 1024 bytes wide; walkers of the rows, four at a time).  The row and its source are wave-uniform.
    for (int y = (int)blockIdx.y * AK_ROWS + wave; y < P.rows; y += (int)gridDim.y * AK_ROWS) {
        const bool anchor = (y & 1) == a.q;
        uint8_t* dst = P.out + (int64_t)y * P.pitch_out;
        if (anchor || !average) {
            const uint8_t* src = anchor ? P.cur + (int64_t)y * P.pitch_cur : other + (int64_t)y * other_pitch;
            for (int64_t off = (int64_t)blockIdx.x * AK_WAVE_BYTES + 16 * lane; off < P.row_bytes; off += (int64_t)gridDim.x * AK_WAVE_BYTES) {
                const int64_t left = P.row_bytes - off;
                if (P.vec && left >= 16) {
                    *reinterpret_cast<uint4*>(dst + off) = *reinterpret_cast<const uint4*>(src + off);
                } else {
                    const int n = left < 16 ? (int)left : 16;
                    for (int b = 0; b < n; b += BPS) store_sample<MODE>(dst + off + b, load_sample<MODE>(src + off + b));
                }
            }
        } else {
            const int ya = y == 0 ? 1 : y - 1, yb = y == P.rows - 1 ? y - 1 : y + 1;   // the row's own neighbour twice at an edge
            const uint8_t* sa = P.cur + (int64_t)ya * P.pitch_cur;
            const uint8_t* sb = P.cur + (int64_t)yb * P.pitch_cur;
            for (int64_t off = (int64_t)blockIdx.x * AK_WAVE_BYTES + 16 * lane; off < P.row_bytes; off += (int64_t)gridDim.x * AK_WAVE_BYTES) {
                const int64_t left = P.row_bytes - off;
                if (P.vec && left >= 16) {
                    const uint4 va = *reinterpret_cast<const uint4*>(sa + off), vb = *reinterpret_cast<const uint4*>(sb + off);
                    *reinterpret_cast<uint4*>(dst + off) = make_uint4(average_dword<MODE>(va.x, vb.x), average_dword<MODE>(va.y, vb.y),
                                                                      average_dword<MODE>(va.z, vb.z), average_dword<MODE>(va.w, vb.w));
                } else {
                    const int n = left < 16 ? (int)left : 16;
                    for (int b = 0; b < n; b += BPS)
                        store_sample<MODE>(dst + off + b, average_sample<MODE>(load_sample<MODE>(sa + off + b), load_sample<MODE>(sb + off + b)));
                }
            }
        }
    }
}

int pulldown_assemble(const AssembleCall& c, hipStream_t stream) {
    for (int p = 0; p < c.n_planes; ++p) {
        AssembleArgs a;
        a.p = c.plane[p];
        a.q = c.anchor; a.match = c.match; a.combed = c.combed; a.post = c.post;
        a.decision = c.decision;
        const int64_t gx = (a.p.row_bytes + AK_WAVE_BYTES - 1) / AK_WAVE_BYTES;
        const int64_t gy = ((int64_t)a.p.rows + AK_ROWS - 1) / AK_ROWS;
        const dim3 blocks((uint32_t)(gx < AK_MAX_X ? gx : AK_MAX_X), (uint32_t)(gy < AK_MAX_Y ? gy : AK_MAX_Y));
        if (c.mode == Y8_BYTE) pulldown_assemble_kernel<Y8_BYTE><<<blocks, 64 * AK_ROWS, 0, stream>>>(a);
        else if (c.mode == Y8_P010) pulldown_assemble_kernel<Y8_P010><<<blocks, 64 * AK_ROWS, 0, stream>>>(a);
        else pulldown_assemble_kernel<Y8_LOW10><<<blocks, 64 * AK_ROWS, 0, stream>>>(a);
    }
    return (int)hipGetLastError();
}

}  // namespace fldr_pulldown_impl
