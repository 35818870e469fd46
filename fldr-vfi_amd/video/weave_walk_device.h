// The walk of the weave kernels of ../field/field_kernels.hip and ../interlace/interlace_kernels.hip, device side, inlined into each: one
// launch serves every plane of a frame, a work item is one 16-byte column group of one row of one plane, consecutive lanes take
// consecutive groups of a row.  Here: what every plane of such a launch carries, the plane of a thread, the split of its
// item into row and bytes, and the choice of the 16-byte or the per-sample form.  Which rows the item rows are, where the sources lie
// and what is done with a group stay with the including kernel; weave_walk_host.h fills a plane's walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace fldr_weave {

// What every plane of such a launch carries, under these names, beside its sources and their pitches — a Plane below is any struct
// that has them:
//     uint8_t* out; int64_t pitch_out;
//     int64_t row_bytes;
//     int rows;                       R: even
//     int vec;                        every address and pitch of the plane is 16-byte aligned: 16-byte loads and stores
//     uint32_t groups;                ceil(row_bytes / 16)
//     uint32_t groups_magic;          floor(2^32 / groups) + 1
//     uint32_t first;                 the plane's first work item
// They are no base struct because the order of a plane's members is part of what a kernel costs: a lane reads them from the kernel
// arguments by its plane's number, and with the common members moved to the front the interlacer's filtered kernels took 1 to 2.5 %
// longer at 3840 x 2160 while its unfiltered one and the deinterlacer's took 1 to 4 % less (DESIGN_LOG.md).  Each library keeps the
// order it was measured with.

struct Item {
    uint32_t row;                      // the item row: which row of the plane that is, the kernel says
    int64_t xoff;                      // the group's first byte in its row: 0 in the row's first group
    int64_t rest;                      // bytes of the row from there on: > 0; a whole group has 16 or more
};

// item / groups without a division, which would go through float: with magic = floor(2^32 / groups) + 1, umulhi(item, magic) is the
// quotient while item x groups < 2^32 (the error item x (magic - 2^32 / groups) / 2^32 then stays below 1 / groups).  The host refuses
// larger planes; groups == 1 would need magic = 2^32 and is taken apart.
template <class Plane> __device__ __forceinline__ Item split(const Plane& pl, uint32_t item) {
    Item it;
    it.row = pl.groups == 1u ? item : __umulhi(item, pl.groups_magic);
    it.xoff = 16ll * (item - it.row * pl.groups);
    it.rest = pl.row_bytes - it.xoff;
    return it;
}

// Thread `id` of a launch over a.pl[0 .. a.planes - 1] (a.total items; plane q begins at a.pl[q].first): f(plane, item, VEC) with VEC
// a std::true_type where the plane takes 16-byte loads and stores, a std::false_type where it goes sample by sample.  f calls split
// itself, behind whatever else it dispatches on: split here, ahead of the deinterlacer's choice of `comp`, cost that kernel a VGPR.
template <class Args, class F> __device__ __forceinline__ void walk(const Args& a, uint32_t id, F f) {
    if (id >= a.total) return;
    const int q = (a.planes > 2 && id >= a.pl[2].first) ? 2 : (a.planes > 1 && id >= a.pl[1].first) ? 1 : 0;
    const auto& pl = a.pl[q];
    if (pl.vec) f(pl, id - pl.first, std::true_type());
    else f(pl, id - pl.first, std::false_type());
}

}  // namespace fldr_weave
