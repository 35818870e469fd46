// libfldr_pulldown.so, shared between the host side (pulldown_host.hip) and the kernels (pulldown_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../rate/tile_reduce_device.h"
#include "fldr_pulldown.h"

namespace fldr_pulldown_impl {
using namespace fldr_tile_reduce;

// The measure state (FLDR_PULLDOWN_STATE_BYTES of device memory) in lines of 128 bytes: line 0 begins with the result the caller reads,
// lines 1 .. SLOTS are the kernels' accumulator slots; workgroup b adds to slot 1 + b % SLOTS (../rate/tile_reduce_device.h).
constexpr int STATE_SLOT_BYTES = 128;
constexpr int SLOT_COMB_OFFSET = 0;        // uint64 x 3: the combed samples of each candidate in the slot's workgroups
constexpr int SLOT_KEY_OFFSET = 24;        // uint64 x 3: max over their tiles of (tile_comb << 32) | (0xffffffff - index)
constexpr int SLOT_DSAD_OFFSET = 48;       // uint64: the sum of the anchor rows' tile sums
constexpr int SLOT_DKEY_OFFSET = 56;       // uint64: max of (tile_sad << 32) | (0xffffffff - index)
constexpr int SLOT_DMOVING_OFFSET = 64;    // uint32: tiles with tile_sad >= tile_sad_min

struct MeasureCall {
    const void* cur; const void* prev; const void* next;   // plane 0; prev / next may be null: not measured
    int64_t pitch_cur, pitch_prev, pitch_next;
    int H, W, mode, anchor;
    int comb_thresh, comb_tile_min, tile_sad_min, allowed;
};

// zero `state`, reduce every tile, write the result and the decision: three launches on `stream`
int pulldown_measure(const MeasureCall& c, void* state, hipStream_t stream);

struct AssemblePlane {
    const uint8_t* cur; const uint8_t* prev; const uint8_t* next;   // never null: the host puts cur where a frame is missing
    uint8_t* out;
    int64_t pitch_cur, pitch_prev, pitch_next, pitch_out;
    int64_t row_bytes;
    int rows;
    int vec;                               // every address and pitch of the plane is 16-byte aligned
};

struct AssembleCall {
    AssemblePlane plane[3];
    int n_planes, mode, anchor;
    int match, combed;                     // match -1: both from `decision`
    const int32_t* decision;
    int post;
};

// one launch on `stream`
int pulldown_assemble(const AssembleCall& c, hipStream_t stream);

}  // namespace fldr_pulldown_impl
