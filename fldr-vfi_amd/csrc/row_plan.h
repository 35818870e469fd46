// Which rows the synthesis half has to produce when only the top Hc rows of the H-row (padded) frame are shown: plain C++, no GPU call
// (fldr_synth_row_plan, include/fldr_hip.h).  The row-limited launchers check their tile heights against the constants below.
//
// Derived backwards from the crop.  Two kinds of consumer -> producer edge:
//   * STRICT (dec23_synth and the 3x3 ring convolutions dec0 / dec1): the consumer reads every row its active tiles reach, halo included,
//     so the producer writes all of them.  Counts are whole tile rows, which makes this edge grow: dec1's rounded count is what decides
//     dec0's, and so on.
//   * MASKED (the stride-2 encoders enc1 / enc2 / enc3, called with src_rows = the producer's count): a source row at or beyond the
//     producer's count is zero padding to them and is never read, so the producer only writes the rows that the consumer's NEEDED output
//     rows reach ("need" below).  Consumer rows that saw the mask are finite, wrong, and never reach a needed row further down.
// Without the masked edges the rounding of the strict ones compounds through three resolutions and gives every encoder all its rows
// at 3840 x 2160 (padded to 2304).
#pragma once
#include <stdint.h>
#include "fldr_hip.h"

#define FLDR_PLAN_TH_DEC23 8        // half-resolution rows per tile row of dec23_synth_kernel (16 frame rows)
#define FLDR_PLAN_TH_CONV 8         // output rows per tile row of the stride-2 and the ring convolutions
#define FLDR_PLAN_TH_SPLAT 24       // destination rows per tile of the image splat
#define FLDR_PLAN_TH_PREP 4         // rows per workgroup of level0_prep_kernel

static inline int fldr_plan_up(int rows, int tile, int full) {          // whole tiles, never more than the tensor
    const int r = (rows + tile - 1) / tile * tile;
    return r < full ? r : full;
}
static inline int fldr_plan_min(int a, int b) { return a < b ? a : b; }
static inline int fldr_plan_max(int a, int b) { return a > b ? a : b; }

// H: padded frame rows, a multiple of 8; 0 < Hc <= H.  Every count is in the stage's own output rows.
static inline int fldr_plan_rows(int H, int Hc, fldr_synth_rows* p) {
    if (!p || H <= 0 || Hc <= 0 || Hc > H) return FLDR_E_ARG;
    if (H & 7) return FLDR_E_SHAPE;
    const int h2 = H / 2, h4 = H / 4, h8 = H / 8;
    const int T = FLDR_PLAN_TH_CONV;
    // dec23: tile rows of 16 frame rows; an active tile reads enc1 rows i0 - 2 .. i0 + 9, dec1 rows i0 / 2 - 1 .. i0 / 2 + 4 and the
    // candidates' frame rows 2 i0 .. 2 i0 + 15 (i0 = 8 * tile row)
    const int r23 = (Hc + 2 * FLDR_PLAN_TH_DEC23 - 1) / (2 * FLDR_PLAN_TH_DEC23);
    p->dec23 = fldr_plan_min(H, 2 * FLDR_PLAN_TH_DEC23 * r23);
    const int need_d1 = fldr_plan_min(h4, (FLDR_PLAN_TH_DEC23 / 2) * r23 + 1);
    p->dec1 = fldr_plan_up(need_d1, T, h4);
    // dec1 (3x3 on nearest-x2(dec0), enc2): output rows < n read input rows <= n, i.e. dec0 rows <= n >> 1
    p->dec0 = fldr_plan_up(fldr_plan_min(h8, (fldr_plan_min(p->dec1, h4 - 1) >> 1) + 1), T, h8);
    const int need_d0 = fldr_plan_min(h8, (fldr_plan_min(need_d1, h4 - 1) >> 1) + 1);
    // dec0 (3x3 on enc3): strict
    p->enc3 = fldr_plan_up(fldr_plan_min(h8, p->dec0 + 1), T, h8);
    const int need_e3 = fldr_plan_min(h8, need_d0 + 1);
    // enc2: dec1 strict (rows <= its count); enc3 masked (4x4 stride 2 pad 1: output row r reads rows 2 r - 1 .. 2 r + 2)
    const int need_e2 = fldr_plan_max(fldr_plan_min(h4, p->dec1 + 1), fldr_plan_min(h4, 2 * need_e3 + 1));
    p->enc2 = fldr_plan_up(need_e2, T, h4);
    // enc1: dec23 strict; enc2 masked
    const int need_e1 = fldr_plan_max(fldr_plan_min(h2, FLDR_PLAN_TH_DEC23 * r23 + 2), fldr_plan_min(h2, 2 * need_e2 + 1));
    p->enc1 = fldr_plan_up(need_e1, T, h2);
    // the frame-resolution planes enc1 and the blend read (warped frames; flowback, im_tot): dec23's candidates strict, enc1 masked
    const int need_f = fldr_plan_max(p->dec23, fldr_plan_min(H, 2 * need_e1 + 1));
    p->splat = fldr_plan_up(need_f, FLDR_PLAN_TH_SPLAT, H);
    p->prep2 = fldr_plan_up(need_f, FLDR_PLAN_TH_PREP, H);
    return 0;
}
