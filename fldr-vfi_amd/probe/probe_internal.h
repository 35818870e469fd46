// libfldr_probe.so, shared between the host side (probe_host.hip) and the kernels (probe_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/tile_reduce_device.h"
#include "fldr_probe.h"

namespace fldr_probe_impl {
using namespace fldr_tile_reduce;

// The measure state (FLDR_PROBE_STATE_BYTES of device memory) in lines of 256 bytes: line 0 is the result the caller reads, lines
// 1 .. SLOTS are the kernels' accumulator slots; workgroup b adds to slot 1 + b % SLOTS (../rate/tile_reduce_device.h).
constexpr int STATE_SLOT_BYTES = 256;
// A slot: N_SUMS uint64 sums, N_KEYS uint64 keys (max over the tiles of (value << 32) | (0xffffffff - index)), N_COUNTS uint32 counts.
// Sums and keys 0 .. 5: comb[q][k] at 3 q + k; 6, 7: the field SAD of parity 0, 1.  Sums 8 .. 13: lap[k][p] at 8 + 2 k + p.
// Counts: field_moving_tiles[0], [1], frame_moving_tiles.
constexpr int N_KEYS = 8, N_SUMS = 14, N_COUNTS = 3;
constexpr int SLOT_SUM_OFFSET = 0;
constexpr int SLOT_KEY_OFFSET = 8 * N_SUMS;
constexpr int SLOT_COUNT_OFFSET = 8 * (N_SUMS + N_KEYS);
static_assert(SLOT_COUNT_OFFSET + 4 * N_COUNTS <= STATE_SLOT_BYTES, "a slot holds its words");
static_assert(sizeof(fldr_probe_result) == STATE_SLOT_BYTES, "the result is line 0");

struct MeasureCall {
    const void* cur; const void* prev; const void* next;   // plane 0; prev / next may be null: not measured
    int64_t pitch_cur, pitch_prev, pitch_next;
    int H, W, mode;
    int comb_thresh, tile_sad_min, frame_tile_sad_min;
};

// zero `state`, reduce every tile, write the result: three launches on `stream`
int probe_measure(const MeasureCall& c, void* state, hipStream_t stream);

}  // namespace fldr_probe_impl
