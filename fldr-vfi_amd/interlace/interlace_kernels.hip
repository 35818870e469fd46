// The kernel of libfldr_interlace.so: the weave of two progressive frames into one interlaced frame, each row through the vertical
// anti-twitter filter of fldr_interlace.h.
//
// A pure streaming kernel in the manner of ../field/field_kernels.hip: integer arithmetic on code values, no LDS, no atomics, no float.
// One launch serves every plane of the frame and both parities (or the one parity whose source is given).  A work item is one 16-byte
// column group (16 samples at depth 8, 8 at depth 10) of one output row y: the lane loads that group of the 1, 3 or 5 rows y - 2 ..
// y + 2 (clamped to the plane) of the row's source, filters and stores.  The rows of an item overlap those of the items two rows up and
// down in the same source; the L2 serves them, so from HBM every source row wanted is read once.  All loads of an item are issued
// before the first is used.  Consecutive lanes take consecutive groups of a row: a wave reads 1 KiB runs.  The walk — a thread's plane,
// its item's row and group, the 16-byte or per-sample form — is ../video/weave_walk_device.h's.
// The 16-byte loads and stores need every address and pitch of the plane 16-byte aligned (WeavePlane::vec, decided per plane); the same
// arithmetic runs on per-sample loads and stores otherwise, and a row's last, partial group goes sample by sample in either form.
// Under FLDR_INTERLACE_NONE the dwords are stored as they were loaded (P010: the low six bits included).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "interlace_internal.h"

namespace fldr_interlace_impl {
using namespace fldr_sample16;

#define IK_THREADS 256

// one output sample from the samples of the rows y - R .. y + R
template <int FORM, int FILTER> __device__ __forceinline__ int filter_sample(const int* s) {
    if (FILTER == FLDR_INTERLACE_LINEAR) return (s[0] + 2 * s[1] + s[2] + 2) >> 2;
    // clamp(floor(v / 8), 0, MX), written as the clamp of v to 0 .. 8 MX + 7 and then the shift.  The other order — arithmetic shift, clamp
    // to 0 .. 255, pack — is what hipcc turns into v_ashr_pk_u8_i32 at depth 8 and ORs two more bytes on top of, taking the result's high
    // half for zero; on the MI355X that half came back as the high half of the first source, all ones under a negative sum, and the two
    // bytes beside a clamped-low pair were written as 255 (DESIGN_LOG.md).
    const int v = -s[0] + 2 * s[1] + 6 * s[2] + 2 * s[3] - s[4] + 4;
    return min(max(v, 0), 8 * Sample<FORM>::MX + 7) >> 3;
}

// one group of `nv` samples of output row y: load the 2 R + 1 source rows, filter, store
template <int FORM, int FILTER, bool VEC>
__device__ __forceinline__ void weave_group(const WeavePlane& pl, int y, int64_t xoff, int nv) {
    using S = Sample<FORM>;
    constexpr int R = FILTER == FLDR_INTERLACE_NONE ? 0 : FILTER == FLDR_INTERLACE_LINEAR ? 1 : 2;
    const bool is_odd = (y & 1) != 0;
    const uint8_t* src = (is_odd ? pl.odd : pl.even) + xoff;
    const int64_t pitch = is_odd ? pl.pitch_odd : pl.pitch_even;
    uint32_t d[2 * R + 1][4];
#pragma unroll
    for (int k = -R; k <= R; ++k) {
        const int yy = min(max(y + k, 0), pl.rows - 1);
        load_group<FORM, VEC>(src + (int64_t)yy * pitch, nv, d[k + R]);
    }
    uint8_t* dst = pl.out + (int64_t)y * pl.pitch_out + xoff;
    if constexpr (FILTER == FLDR_INTERLACE_NONE) {
        store_group<FORM, VEC>(dst, nv, d[0]);
    } else {
        uint32_t o[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int n = 0; n < S::NS; ++n) {
            int s[2 * R + 1];
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) s[k] = value_of<FORM>(raw_at<FORM>(d[k], n));
            put_at<FORM>(o, n, canonical<FORM>(filter_sample<FORM, FILTER>(s)));
        }
        store_group<FORM, VEC>(dst, nv, o);
    }
}

template <int FORM, int FILTER>
__global__ __launch_bounds__(IK_THREADS) void interlace_weave_kernel(WeaveArgs a) {
    const int start = a.start, step = a.step;                          // here: read inside the lambda they came late, behind a wait of their own
    fldr_weave::walk(a, blockIdx.x * IK_THREADS + threadIdx.x, [=](const WeavePlane& pl, uint32_t item, auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        const fldr_weave::Item it = fldr_weave::split(pl, item);
        const int y = start + step * (int)it.row;                      // < pl.rows
        // a whole group knows its sample count at compile time: its loads carry no test and go out together
        if (it.rest >= 16) weave_group<FORM, FILTER, VEC>(pl, y, it.xoff, Sample<FORM>::NS);
        else weave_group<FORM, FILTER, VEC>(pl, y, it.xoff, (int)(it.rest / Sample<FORM>::BPS));
    });
}

int weave(const WeaveArgs& a, int form, int filter, hipStream_t stream) {
    const unsigned blocks = (a.total + IK_THREADS - 1) / IK_THREADS;
    if (filter == FLDR_INTERLACE_NONE) SAMPLE16_LAUNCH_FORM(interlace_weave_kernel, form, blocks, IK_THREADS, stream, (a), FLDR_INTERLACE_NONE);
    else if (filter == FLDR_INTERLACE_LINEAR) SAMPLE16_LAUNCH_FORM(interlace_weave_kernel, form, blocks, IK_THREADS, stream, (a), FLDR_INTERLACE_LINEAR);
    else SAMPLE16_LAUNCH_FORM(interlace_weave_kernel, form, blocks, IK_THREADS, stream, (a), FLDR_INTERLACE_COMPLEX);
    return (int)hipGetLastError();
}

}  // namespace fldr_interlace_impl
