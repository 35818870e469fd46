// The kernel of libfldr_field.so: the weave of one field with an estimate of its missing lines (fldr_field.h has the rule).
//
// A pure streaming kernel: five sources read (cur; prev, next and temporal for the missing rows only), one frame written, integer
// arithmetic on code values, no LDS, no atomics, no float.  One launch serves every plane of the frame.  A work item is one 16-byte
// column group (16 samples at depth 8, 8 at depth 10) of one own-parity row: the lane copies that row, loads the own row below it and
// computes the missing row between the two, so every row of `cur` is loaded by two items, the second time from the L2.  (A lane that
// walks down several own rows and keeps the row above in registers loads each row once but halves the work items per step; tried at
// 3840 x 2160 it was slower, and it is not here.)  Consecutive lanes take consecutive groups of a row: a wave reads 1 KiB runs.
// The 16-byte loads and stores need every address and pitch of the plane 16-byte aligned (WeavePlane::vec, decided per plane); the same
// arithmetic runs on per-sample loads and stores otherwise, and a row's last, partial group goes sample by sample in either form.
// The +-1 column of the difference d comes from per-sample loads of the `comp` samples on either side of the group — they lie in the
// lines the neighbouring lanes load — and is clamped at the plane's edges by leaving the missing neighbour out of the maximum.
// The own-parity rows are stored as the dwords they were loaded as (P010: the low six bits included).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_internal.h"

namespace fldr_field_impl {
using namespace fldr_sample16;

#define WK_THREADS 256

// A group sample by sample — Sample, value_of, canonical, raw_at, put_at, load_raw, load_group, store_group — is ../video/sample16_device.h's;
// the walk — a thread's plane, its item's row and group, the 16-byte or per-sample form — ../video/weave_walk_device.h's.

// One missing row y of one group: ra / rb are the group's samples of the own rows above and below it (mirrored at the plane's edge).
// first: the group is the row's first; behind: the samples of the row behind the group's 16 bytes.
template <int FORM, bool VEC, int CS>
__device__ __forceinline__ void weave_row(const WeavePlane& pl, int y, int64_t xoff, int nv, bool first, int64_t behind, const uint32_t ra[4],
                                          const uint32_t rb[4], bool intra, int still, int slack) {
    using S = Sample<FORM>;
    uint32_t o[4] = { 0u, 0u, 0u, 0u };
    if (intra) {
#pragma unroll
        for (int i = 0; i < S::NS; ++i) {
            const int a = value_of<FORM>(raw_at<FORM>(ra, i)), b = value_of<FORM>(raw_at<FORM>(rb, i));
            put_at<FORM>(o, i, canonical<FORM>((a + b + 1) >> 1));
        }
    } else {
        const uint8_t* pp = pl.prev + (int64_t)y * pl.pitch_prev + xoff;
        const uint8_t* pn = pl.next + (int64_t)y * pl.pitch_next + xoff;
        const uint8_t* pt = pl.temporal + (int64_t)(y >> 1) * pl.pitch_temporal + xoff;
        uint32_t dp[4], dn[4], dt[4];
        load_group<FORM, VEC>(pp, nv, dp);
        load_group<FORM, VEC>(pn, nv, dn);
        load_group<FORM, VEC>(pt, nv, dt);
        int left[CS], right[CS];                                      // |prev - next| of the CS samples on either side; -1: no such sample
#pragma unroll
        for (int k = 0; k < CS; ++k) {
            left[k] = right[k] = -1;
            if (!first) left[k] = abs(value_of<FORM>(load_raw<FORM>(pp - (CS - k) * S::BPS)) - value_of<FORM>(load_raw<FORM>(pn - (CS - k) * S::BPS)));
            if (k < behind) right[k] = abs(value_of<FORM>(load_raw<FORM>(pp + 16 + k * S::BPS)) - value_of<FORM>(load_raw<FORM>(pn + 16 + k * S::BPS)));
        }
        int P[S::NS], N[S::NS], D[S::NS];
#pragma unroll
        for (int i = 0; i < S::NS; ++i) {
            P[i] = value_of<FORM>(raw_at<FORM>(dp, i));
            N[i] = value_of<FORM>(raw_at<FORM>(dn, i));
            D[i] = abs(P[i] - N[i]);
        }
#pragma unroll
        for (int i = 0; i < S::NS; ++i) {
            const int l = i >= CS ? D[i - CS] : left[i];
            const int r = i + CS < S::NS ? (i + CS < nv ? D[i + CS] : -1) : right[i + CS - S::NS];
            const int d = max(D[i], max(l, r));
            const int a = value_of<FORM>(raw_at<FORM>(ra, i)), b = value_of<FORM>(raw_at<FORM>(rb, i));
            const int lo = max(min(a, b) - slack, 0), hi = min(max(a, b) + slack, S::MX);
            const int t = value_of<FORM>(raw_at<FORM>(dt, i));
            const int v = (still >= 0 && d <= still) ? (P[i] + N[i] + 1) >> 1 : min(max(t, lo), hi);
            put_at<FORM>(o, i, canonical<FORM>(v));
        }
    }
    store_group<FORM, VEC>(pl.out + (int64_t)y * pl.pitch_out + xoff, nv, o);
}

// one group of one own-parity row (row parity + 2 i): the row itself and the missing row below it; the item of row i = 0 also takes
// the missing row 0 of a bottom field.  The own row below is loaded a second time by the item of row i + 1: the L2 serves it.
template <int FORM, bool VEC, int CS>
__device__ __forceinline__ void weave_item(const WeaveArgs& a, const WeavePlane& pl, uint32_t item, bool intra) {
    using S = Sample<FORM>;
    const fldr_weave::Item it = fldr_weave::split(pl, item);
    const int64_t xoff = it.xoff, rest = it.rest;
    const int nv = rest >= 16 ? S::NS : (int)(rest / S::BPS);
    const int64_t behind = rest >= 16 ? (rest - 16) / S::BPS : 0;
    const bool first = xoff == 0;
    const int n_own = pl.rows >> 1;
    const uint32_t i = it.row;
    const int yo = a.parity + 2 * (int)i;
    uint32_t ra[4], rb[4];
    load_group<FORM, VEC>(pl.cur + (int64_t)yo * pl.pitch_cur + xoff, nv, ra);
    store_group<FORM, VEC>(pl.out + (int64_t)yo * pl.pitch_out + xoff, nv, ra);
    if (i == 0u && a.parity == 1) weave_row<FORM, VEC, CS>(pl, 0, xoff, nv, first, behind, ra, ra, intra, a.still, a.slack);
    if (yo + 1 >= pl.rows) return;                                     // a bottom field's last own row is the plane's last
    if ((int)i + 1 < n_own) load_group<FORM, VEC>(pl.cur + (int64_t)(yo + 2) * pl.pitch_cur + xoff, nv, rb);
    else { rb[0] = ra[0]; rb[1] = ra[1]; rb[2] = ra[2]; rb[3] = ra[3]; }        // a top field's last missing row: mirrored
    weave_row<FORM, VEC, CS>(pl, yo + 1, xoff, nv, first, behind, ra, rb, intra, a.still, a.slack);
}

template <int FORM>
__global__ __launch_bounds__(WK_THREADS) void field_weave_kernel(WeaveArgs a) {
    fldr_weave::walk(a, blockIdx.x * WK_THREADS + threadIdx.x, [&](const WeavePlane& pl, uint32_t item, auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        const bool intra = a.intra || (a.intra_if && *a.intra_if != 0u);
        if (pl.comp == 2) weave_item<FORM, VEC, 2>(a, pl, item, intra);
        else weave_item<FORM, VEC, 1>(a, pl, item, intra);
    });
}

int weave(const WeaveArgs& a, int form, hipStream_t stream) {
    SAMPLE16_LAUNCH_FORM(field_weave_kernel, form, (a.total + WK_THREADS - 1) / WK_THREADS, WK_THREADS, stream, (a));
    return (int)hipGetLastError();
}

}  // namespace fldr_field_impl
