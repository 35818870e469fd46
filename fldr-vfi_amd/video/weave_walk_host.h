// The host side of weave_walk_device.h: the frame heights a weave takes, the alignment its 16-byte form needs, and the fill of a plane's
// walk with the limits of the kernel's 32-bit index arithmetic.  Included by ../field/field_host.hip and ../interlace/interlace_host.hip
// after frame_host.h's rules (through ../rate/rate_plan.h); the two libraries judge the limit on different rows, and each says so in its
// public header.  Everything is in the unnamed namespace; no HIP call is made here.
#pragma once
#include "frame_host.h"

namespace {

bool size_ok(int H) { return H >= 4 && (H & 3) == 0; }

bool aligned16(const void* p, int64_t pitch) { return (((uintptr_t)p | (uintptr_t)pitch) & 15) == 0; }

// Everything weave_walk_device.h lists of plane p but `vec`, for an H x W frame in `f` written to `out`.  One work item per group and walked row, numbered
// from `total`, which is advanced; the kernel's item / groups is exact while item x groups < 2^32, and the library says on how many
// rows that is judged.  False beyond the index arithmetic: groups x groups x judged_rows >= 2^32, or more than 2^31 - 1 items by now.
template <class Plane>
bool fill_walk(Plane& q, const fldr_video_format& f, int p, int H, int W, const fldr_video_frame& out, int64_t walked_rows,
               int64_t judged_rows, int64_t& total) {
    q.out = (uint8_t*)out.plane[p]; q.pitch_out = out.pitch[p];
    q.row_bytes = row_bytes(f, p, W);
    q.rows = rows_of(p, H);
    const int64_t groups = (q.row_bytes + 15) / 16;                    // < 2^28: its square is no overflow, nor is a square < 2^32 x rows
    if (groups * groups >= (1ll << 32) || groups * groups * judged_rows >= (1ll << 32)) return false;
    q.groups = (uint32_t)groups;
    q.groups_magic = (uint32_t)((1ull << 32) / (uint64_t)groups) + 1u;
    q.first = (uint32_t)total;
    total += groups * walked_rows;
    return total <= 0x7fffffffll;
}

}  // namespace
