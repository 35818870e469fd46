// The integer table of include/fldr_conform.h, section "THE RULE": pure host arithmetic in double, no device header, so that it compiles
// into a stand-alone program (tests/conform_coefs_main.cpp) as well as into conform_host.hip.  The operations are written in the order of
// tests/conform_oracle.py, so that both round the same doubles.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fldr_conform.h"

namespace fldr_conform_impl {

// what a side's range and depth give: the luma offset and span, the chroma centre and span, the largest code
struct ConformSide { int depth, yo, ys, cc, cs, mx; };

inline ConformSide conform_side(const fldr_video_format& f) {
    ConformSide s;
    s.depth = f.depth == 10 ? 10 : 8;
    const int sh = s.depth - 8;
    const bool lim = f.range == FLDR_VIDEO_LIMITED;
    s.mx = (1 << s.depth) - 1;
    s.yo = lim ? 16 << sh : 0;
    s.ys = lim ? 219 << sh : s.mx;
    s.cc = 1 << (s.depth - 1);
    s.cs = lim ? 224 << sh : s.mx;
    return s;
}

inline int32_t conform_round14(double v) { return (int32_t)floor(v * 16384.0 + 0.5); }

// k[FLDR_CONFORM_KYY .. FLDR_CONFORM_KVV] of src -> dst, two formats the caller has checked
inline void conform_coefs(const fldr_video_format& src, const fldr_video_format& dst, int32_t k[7]) {
    static const double KR[2] = { 0.299, 0.2126 }, KB[2] = { 0.114, 0.0722 };
    double myu = 0.0, myv = 0.0, muu = 1.0, muv = 0.0, mvu = 0.0, mvv = 1.0;        // equal matrices: exact, by definition
    if (src.matrix != dst.matrix) {
        const double kra = KR[src.matrix], kba = KB[src.matrix], kga = 1.0 - kra - kba;
        const double krb = KR[dst.matrix], kbb = KB[dst.matrix], kgb = 1.0 - krb - kbb;
        myu = 2.0 * (1.0 - kba) * (kbb - kgb * kba / kga);
        myv = 2.0 * (1.0 - kra) * (krb - kgb * kra / kga);
        muu = (2.0 * (1.0 - kba) - myu) / (2.0 * (1.0 - kbb));
        muv = -myv / (2.0 * (1.0 - kbb));
        mvv = (2.0 * (1.0 - kra) - myv) / (2.0 * (1.0 - krb));
        mvu = -myu / (2.0 * (1.0 - krb));
    }
    const ConformSide s = conform_side(src), d = conform_side(dst);
    const double ys_s = s.ys, cs_s = s.cs, ys_d = d.ys, cs_d = d.cs;
    k[FLDR_CONFORM_KYY] = conform_round14(ys_d / ys_s);
    k[FLDR_CONFORM_KYU] = conform_round14(myu * ys_d / cs_s);
    k[FLDR_CONFORM_KYV] = conform_round14(myv * ys_d / cs_s);
    k[FLDR_CONFORM_KUU] = conform_round14(muu * cs_d / cs_s);
    k[FLDR_CONFORM_KUV] = conform_round14(muv * cs_d / cs_s);
    k[FLDR_CONFORM_KVU] = conform_round14(mvu * cs_d / cs_s);
    k[FLDR_CONFORM_KVV] = conform_round14(mvv * cs_d / cs_s);
}

}  // namespace fldr_conform_impl
