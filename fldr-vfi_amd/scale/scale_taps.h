// The table builder of libfldr_scale.so (fldr_scale.h, "Tables"): pure host arithmetic, no device header, so that it also compiles into
// a stand-alone program under the host sanitizers (tests/scale_taps_main.cpp).  The centre and left of an output are exact integers over
// a common denominator; only the weights are float64.  Everything is in the unnamed namespace: nothing here becomes a symbol of the
// library.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "fldr_scale.h"

namespace {

int scale_radius(int filter) { return filter + 1; }                    // bilinear 1, bicubic 2, Lanczos3 3

bool scale_size_ok(int v) { return v >= 1 && v <= FLDR_SCALE_MAX_SIZE; }

// n = 2 ceil(a max(1, in / out)); FLDR_RATE_E_ARG for what fldr_scale_taps_count refuses
int scale_taps_count(int luma_in, int luma_out, int filter) {
    if (!scale_size_ok(luma_in) || !scale_size_ok(luma_out) || (unsigned)filter > (unsigned)FLDR_SCALE_LANCZOS3) return FLDR_RATE_E_ARG;
    const int64_t a = scale_radius(filter);
    const int64_t half = luma_in <= luma_out ? a : (a * luma_in + luma_out - 1) / luma_out;
    return 2 * half > FLDR_SCALE_MAX_TAPS ? FLDR_RATE_E_ARG : (int)(2 * half);
}

int scale_outputs(int luma_out, int kind) { return kind == FLDR_SCALE_LUMA ? luma_out : (luma_out + 1) / 2; }

double scale_weight(int filter, double x) {
    x = fabs(x);
    if (filter == FLDR_SCALE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    if (filter == FLDR_SCALE_BICUBIC) {
        if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
        if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
        return 0.0;
    }
    if (x >= 3.0) return 0.0;
    if (x == 0.0) return 1.0;
    const double px = M_PI * x;
    return sin(px) / px * (sin(px / 3.0) / (px / 3.0));
}

int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); }    // b > 0 here

// the table of one axis of one plane kind (fldr_scale_taps); left: outputs words, coef: outputs x n
int scale_taps(int luma_in, int luma_out, int filter, int kind, int32_t* left, int16_t* coef) {
    const int n = scale_taps_count(luma_in, luma_out, filter);
    if (n < 0) return n;
    if ((unsigned)kind > (unsigned)FLDR_SCALE_CHROMA_V || !left || !coef) return FLDR_RATE_E_ARG;
    const int64_t I = luma_in, O = luma_out;
    const double s = I > O ? (double)I / (double)O : 1.0;
    const int outputs = scale_outputs(luma_out, kind);
    for (int o = 0; o < outputs; ++o) {
        // c = num / den: (o + 1/2) r - 1/2 = ((2o + 1) I - O) / (2 O);  o r + (r - 1) / 4 = (4 o I + I - O) / (4 O)
        const int64_t den = kind == FLDR_SCALE_CHROMA_H ? 4 * O : 2 * O;
        const int64_t num = kind == FLDR_SCALE_CHROMA_H ? 4 * o * I + I - O : (2 * (int64_t)o + 1) * I - O;
        const int64_t l = floor_div(num, den) - n / 2 + 1;
        double w[FLDR_SCALE_MAX_TAPS], sum = 0.0;
        for (int k = 0; k < n; ++k) {
            w[k] = scale_weight(filter, (double)((l + k) * den - num) / (double)den / s);
            sum += w[k];
        }
        if (!(sum > 0.0)) return FLDR_RATE_E_ARG;
        int q[FLDR_SCALE_MAX_TAPS], total = 0, best = 0, mag = 0;
        for (int k = 0; k < n; ++k) {
            q[k] = (int)rint(16384.0 * w[k] / sum);                    // half to even under the default rounding mode
            total += q[k];
            if (q[k] > q[best]) best = k;
        }
        q[best] += 16384 - total;
        for (int k = 0; k < n; ++k) mag += abs(q[k]);
        if (mag > 32767) return FLDR_RATE_E_ARG;
        left[o] = (int32_t)l;
        for (int k = 0; k < n; ++k) coef[(int64_t)o * n + k] = (int16_t)q[k];
    }
    return 0;
}

}  // namespace
