/*
 * fldr_pulldown.h — pulldown API of libfldr_pulldown.so: inverse telecine of film carried in interlaced video (24 fps film in a 60i
 * container by 3:2 pulldown, 25 fps film in 50i with the fields one frame out of phase), by field matching, and conversion of the
 * recovered progressive frames with the rate converter of include/fldr_rate.h.
 *
 * Plain C99; no device header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Error codes.  This header defines no code of its own.  Its own argument errors — a null pointer, a bad size, H not a multiple of 4, a
 * parameter out of range, a non-zero reserved word, a null model — return FLDR_RATE_E_ARG; a measure state that is null or not 256-byte
 * aligned returns FLDR_RATE_E_STATE; a derived rate the converter does not take returns FLDR_RATE_E_RATIO; no such device or a failed
 * allocation returns FLDR_RATE_E_DEVICE.  Codes of the video and model libraries pass through, and so does a positive hipError_t.
 * fldr_pulldown_error_string is fldr_rate_error_string.
 *
 * Terms.  A frame is H x W in a fldr_video_format: NV12 or I420 at depth 8 or 10 (P010 and yuv420p10le included), both fields woven
 * into it line by line.  H is a multiple of 4 and at least 4, so that the chroma planes also split into two fields of whole rows; W >= 1
 * for the two kernels (the model's minimum applies to the stream).  y8(sample) is fldr_rate.h's: the byte at depth 8, word >> 8 for
 * P010, (word & 0x3ff) >> 2 for yuv420p10le.  The anchor parity q (0 or 1) names the rows y % 2 == q of the frame `cur` that every
 * candidate keeps.  Candidate k takes the OTHER rows from S_k: FLDR_PULLDOWN_C (0) from cur itself, FLDR_PULLDOWN_P (1) from the
 * previous frame, FLDR_PULLDOWN_N (2) from the next frame.  Two fields of one film frame weave without combing; two fields of different
 * film frames comb wherever something moved.  Whatever the field order and the phase of the pulldown, the field that belongs to the
 * anchor field is in cur, prev or next: which one is measured, the field order is never asked for.
 *
 * Three layers:
 *
 * 1. fldr_pulldown_measure: how combed each candidate is, and whether the anchor field repeats, in integers.  Only plane 0 is read.
 *    The plane is cut into tiles of 32 x 32 luma samples; tile (ty, tx) covers rows 32 ty .. min(32 ty + 31, H - 1) and the same in
 *    columns (edge tiles are partial); tiles_x = ceil(W / 32), the tile's index is ty * tiles_x + tx.
 *      Combing.  For every row y with y % 2 != q and 1 <= y <= H - 2, and every x:
 *          a = y8(cur[y-1][x]), b = y8(cur[y+1][x]), m = y8(S_k[y][x]);
 *          the sample is combed when (a - m) * (b - m) > comb_thresh * comb_thresh  (strict; the product is an integer): m lies
 *          outside the span of the anchor lines above and below it, by more than comb_thresh on both sides.
 *          comb[k]          = the number of combed samples of candidate k
 *          max_tile_comb[k] = the largest number in one tile (0 .. 512), max_tile[k] = the lowest tile index that attains it (0 when
 *                             no sample is combed)
 *      Anchor repeat.  Over the rows y % 2 == q, tile_sad(i) = sum over tile i of |y8(cur) - y8(prev)|:
 *          dup_sad, dup_max_tile_sad (0 .. 16 x 32 x 255 = 130560), dup_max_tile (the lowest index),
 *          dup_moving_tiles = the tiles with tile_sad >= tile_sad_min.
 *      A candidate whose frame is NULL is not measured: its three words are 0; all dup_* are 0 when prev is NULL.
 *      Decision, taken on the device: match = the allowed candidate with the smallest (max_tile_comb, comb), compared lexicographically;
 *      ties go to C, then P, then N.  combed = max_tile_comb[match] >= comb_tile_min.
 *    Everything is an integer sum, maximum or count, so the result does not depend on the order of the reduction: it is the same from
 *    run to run and equal to the numpy statement of tests/pulldown_oracle.py.
 *    The three defaults (comb_thresh 6, comb_tile_min 32, tile_sad_min 1024) were set on this repository's synthetic content only —
 *    moving textures telecined 3:2, clean and with +-2 codes of noise per field instance —, not on footage.  At comb_thresh 12 the
 *    measure fails on a dark scene, where every candidate scores 0.  A maintainer with footage should look at max_tile_comb of the
 *    matched candidate on film frames (noise and fine vertical detail raise it: comb_tile_min belongs above it) against max_tile_comb of
 *    the wrong candidates on slow motion (comb_thresh belongs below what still separates them), and at dup_max_tile_sad of the repeated
 *    fields of re-encoded material (tile_sad_min belongs above it).
 *
 * 2. fldr_pulldown_assemble: the matched frame, in every plane.  Rows y % 2 == q of every plane are the row bytes of cur, copied as
 *    they are; the other rows are the row bytes of S_match, copied as they are (for P010 the low six bits are included: there is no
 *    arithmetic).  With post = FLDR_PULLDOWN_POST_AVERAGE and combed != 0 the other rows become the line average of the anchor field
 *    instead: o = (a + b + 1) >> 1 with a, b the sample values of cur at rows y - 1 and y + 1 (row y + 1 twice when y == 0, row y - 1
 *    twice when y is the plane's last row); the sample value is the byte at depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le,
 *    and o is written in the container's canonical form (o << 6 for P010); each component of the interleaved NV12 chroma plane is
 *    treated alike.  This is what a frame of true video, or an orphan field at an edit, falls back to.
 *
 * 3. fldr_pulldown_* streams: woven host frames in, converted progressive frames out.  The cadence is declared, not guessed: of every
 *    `cycle` matched frames `drop` are duplicates (3:2 pulldown is 5, 1; phase-shifted 2:2 and plain progressive frames in an interlaced
 *    container are 1, 0).  Which field goes with which, and WHICH frames of a cycle go, is measured.
 *      Schedule.  The push of frame n uploads it, then enqueues measure and assemble of frame n - 1 with prev = n - 2 and next = n.
 *      Frame 0 runs with allowed = C | N, the last frame runs at the flush with C | P (each intersected with cfg.params.allowed; C alone
 *      where that leaves nothing).  The matched frame and its result go to pinned memory.  A push that completes no cycle returns
 *      *n_out = 0 without synchronising.  When the matched frames c cycle .. c cycle + cycle - 1 exist — at the push of frame
 *      (c + 1) cycle — the push synchronises once and drops the `drop` frames with the smallest key (dup_max_tile_sad, dup_sad),
 *      compared lexicographically, the lower frame number first among equal keys; stream frame 0 has no key and is never dropped.  (A
 *      frame's matched content is fixed by the film frame of its anchor field, so equal anchor fields mean a duplicate after matching.)
 *      The survivors go, in order, into a fldr_rate created with cfg.rate, its input rate replaced by
 *      in_num (cycle - drop) / (in_den cycle) reduced by the gcd (fldr_pulldown_inner_rate).
 *    Contract of the stream: the frames fldr_pulldown_push and fldr_pulldown_flush return are, byte for byte and in order, what
 *    fldr_rate_push and fldr_rate_flush return on a fldr_rate of that derived configuration pushed the matched survivors
 *    (tests/test_gpu_pulldown.py holds the two together).  After any failed enqueue or wait the object is as after a reset.  Argument
 *    errors change nothing.  One thread drives a stream.
 *
 * Contract of fldr_pulldown_measure and fldr_pulldown_assemble: they enqueue on `stream`; no allocation, no synchronisation, no
 * host<->device copy: they can be captured into a graph.  Arguments are validated before anything is enqueued.  The measure state needs
 * no preparation: the library zeroes what it uses, on the stream.  Calls with different `state` may be in flight on different streams.
 * Output bytes between a row's end and its pitch are never written.  All offsets are 64-bit: there is no frame-size limit beyond that of
 * the tile index (H, W from 1 to 2^31 - 33, at most 2^31 - 1 tiles).
 *
 * Known costs and limits:
 *   - a survivor is downloaded here and uploaded again by the inner converter;
 *   - outputs arrive a frame plus a cycle late;
 *   - cycle and drop are not detected;
 *   - the comb measure is the plain three-line one: a one-line-high static detail scores in every candidate alike;
 *   - chroma follows the luma decision;
 *   - 4:2:2, packed and RGB interlaced formats are out of scope;
 *   - the stream is synchronous: it is built on the synchronous rate converter, not on the one with frames in flight.
 */
#ifndef FLDR_PULLDOWN_H
#define FLDR_PULLDOWN_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_PULLDOWN_VERSION 100        /* major*10000 + minor*100 + patch of this header */

#define FLDR_PULLDOWN_API __attribute__((visibility("default")))

#define FLDR_PULLDOWN_C 0                /* candidates: the other rows from cur, */
#define FLDR_PULLDOWN_P 1                /* from the previous frame, */
#define FLDR_PULLDOWN_N 2                /* from the next frame */
#define FLDR_PULLDOWN_POST_KEEP    0     /* the matched frame as it is */
#define FLDR_PULLDOWN_POST_AVERAGE 1     /* a frame that stays combed: the other rows from the anchor field's line average */

#define FLDR_PULLDOWN_TILE                 32      /* samples per tile side */
#define FLDR_PULLDOWN_TILE_COMB_MAX        512     /* 16 x 32: the other rows of a tile */
#define FLDR_PULLDOWN_TILE_SAD_MAX         130560  /* 16 x 32 x 255: the anchor rows of a tile */
#define FLDR_PULLDOWN_COMB_THRESH_DEFAULT  6       /* set on synthetic content only */
#define FLDR_PULLDOWN_COMB_TILE_DEFAULT    32      /* one sample in sixteen of a tile's other rows; set on synthetic content only */
#define FLDR_PULLDOWN_TILE_SAD_DEFAULT     1024    /* a mean difference of two codes over a tile's anchor rows; set on synthetic content only */
#define FLDR_PULLDOWN_STATE_BYTES          8192    /* device memory, 256-byte aligned; begins with a fldr_pulldown_result, the rest is the kernels' */
#define FLDR_PULLDOWN_MAX_CYCLE            16

typedef struct fldr_pulldown_params {
    int32_t comb_thresh;                 /* 1 .. 255; 0: FLDR_PULLDOWN_COMB_THRESH_DEFAULT */
    int32_t comb_tile_min;               /* 1 .. 512; 0: FLDR_PULLDOWN_COMB_TILE_DEFAULT */
    int32_t tile_sad_min;                /* 1 .. 130560; 0: FLDR_PULLDOWN_TILE_SAD_DEFAULT */
    int32_t allowed;                     /* bit 0 = C, bit 1 = P, bit 2 = N; 0: all three (7) */
    int32_t reserved[4];                 /* zero */
} fldr_pulldown_params;

typedef struct fldr_pulldown_result {    /* 96 bytes, at the start of the measure state */
    int32_t  match;                      /* offset 0: FLDR_PULLDOWN_C / _P / _N */
    uint32_t combed;                     /* offset 4: 1 when max_tile_comb[match] >= comb_tile_min */
    uint64_t comb[3];                    /* [k]: of candidate k */
    uint32_t max_tile_comb[3];
    uint32_t max_tile[3];                /* the lowest tile index that attains max_tile_comb */
    uint64_t dup_sad;
    uint32_t dup_max_tile_sad;
    uint32_t dup_max_tile;
    uint32_t dup_moving_tiles;           /* tiles with tile_sad >= tile_sad_min */
    uint32_t reserved[5];                /* written as zero */
} fldr_pulldown_result;

FLDR_PULLDOWN_API int         fldr_pulldown_version(void);
FLDR_PULLDOWN_API const char* fldr_pulldown_error_string(int code);
/* 0: sizeof(fldr_pulldown_params), 1: fldr_pulldown_result, 2: fldr_pulldown_config, 3: fldr_pulldown_report — binding self-check;
 * FLDR_RATE_E_ARG otherwise */
FLDR_PULLDOWN_API int         fldr_pulldown_sizeof(int which);

/* Enqueue the measure of cur against prev and next (device planes in *fmt; only plane 0 is read, but every plane of every frame given
 * is checked as fldr_scene_measure checks it).  anchor: q.  p: NULL = the defaults.  prev may be NULL when bit 1 of `allowed` is clear,
 * next when bit 2 is clear.  Checked in this order: fmt / cur null, H, W and anchor (FLDR_RATE_E_ARG); the parameters, and a NULL frame
 * that `allowed` needs (FLDR_RATE_E_ARG); the format; the planes, then the pitches, of cur, prev, next (the video library's codes); the
 * state (FLDR_RATE_E_STATE).  After the stream reaches this point `state` begins with the fldr_pulldown_result. */
FLDR_PULLDOWN_API int fldr_pulldown_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur,
                                            const fldr_video_frame* prev, const fldr_video_frame* next, int anchor,
                                            const fldr_pulldown_params* p, void* state, void* stream);

/* Enqueue the assembly of `out` (device planes, overlapping no input: FLDR_RATE_E_ARG) from cur and S_match.  match: 0 .. 2, with
 * `combed` the caller's (0 or not); or -1: both are read when the kernel runs from `decision`, a device pointer, 4-byte aligned, to the
 * two words {int32 match, uint32 combed} a measure state begins with, so that a graph replay follows a rewritten measure (a word
 * outside 0 .. 2 is taken as C).  prev / next may be NULL when match is given and is not theirs; with match = -1 a NULL frame stands for
 * cur — the `allowed` of the measure keeps it from being chosen.  Checked in this order: null pointers, H, W, anchor, match, post, a
 * null or misaligned decision, a NULL frame the match needs (FLDR_RATE_E_ARG); the format; planes, then pitches, of cur, prev, next,
 * out (the video library's codes); overlap (FLDR_RATE_E_ARG). */
FLDR_PULLDOWN_API int fldr_pulldown_assemble(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur,
                                             const fldr_video_frame* prev, const fldr_video_frame* next, const fldr_video_frame* out,
                                             int anchor, int match, int combed, const void* decision, int post, void* stream);

/* ---- the stream: woven frames in, converted progressive frames out ---------------------------------------------------------------- */
typedef struct fldr_pulldown_config {
    fldr_rate_config     rate;           /* as fldr_rate_create takes it; in_num / in_den is the CONTAINER's frame rate (30000/1001 for 60i) */
    int32_t              cycle;          /* 1 .. FLDR_PULLDOWN_MAX_CYCLE */
    int32_t              drop;           /* 0 .. cycle - 1 matched frames of every cycle are duplicates */
    int32_t              anchor;         /* 0 / 1: the parity of the rows every candidate keeps */
    int32_t              post;           /* FLDR_PULLDOWN_POST_KEEP / _AVERAGE */
    fldr_pulldown_params params;         /* zeros = the defaults */
    int32_t              reserved[4];    /* zero */
} fldr_pulldown_config;

typedef struct fldr_pulldown_report {    /* of the cycle a push completed, or the partial cycle a flush ended; all zero otherwise */
    int64_t  first_frame;                /* stream number of the cycle's frame 0 */
    uint32_t n_frames;                   /* frames in it: cycle, or fewer at a flush */
    uint32_t dropped_mask;               /* bit k: frame first_frame + k was dropped */
    uint32_t combed_mask;                /* bit k: frame first_frame + k stayed combed after matching (true video, an orphan field) */
    uint32_t moving_dropped;             /* dropped frames with dup_moving_tiles != 0: the declared cadence is wrong, or broken at an edit */
    uint32_t still_kept;                 /* kept frames that have a key and dup_moving_tiles == 0 */
    uint32_t cut_mask;                   /* bit k: the pair that ended in the cycle's k-th survivor was a cut for the inner converter */
    int32_t  match[FLDR_PULLDOWN_MAX_CYCLE];   /* [k]: the candidate frame first_frame + k was assembled from */
    uint32_t reserved[2];                /* zero */
    fldr_pulldown_result measure[FLDR_PULLDOWN_MAX_CYCLE];   /* [k]: of frame first_frame + k */
} fldr_pulldown_report;

typedef struct fldr_pulldown fldr_pulldown;

/* *num / *den = in_num (cycle - drop) / (in_den cycle), reduced: the input rate of the inner fldr_rate.  FLDR_RATE_E_ARG on a null
 * pointer or cycle / drop out of range, FLDR_RATE_E_RATIO when in_num or in_den is not positive or a reduced term does not fit int32. */
FLDR_PULLDOWN_API int  fldr_pulldown_inner_rate(const fldr_pulldown_config* cfg, int32_t* num, int32_t* den);
/* Validation order: cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words,
 * thresholds, format, rate terms); then H a multiple of 4, cycle, drop, anchor, post, the parameters and the reserved words
 * (FLDR_RATE_E_ARG); then the derived rate and its ratio to the output rate (FLDR_RATE_E_RATIO); then a null model (FLDR_RATE_E_ARG):
 * all before any device call. */
FLDR_PULLDOWN_API int  fldr_pulldown_create(const fldr_model* model, const fldr_pulldown_config* cfg, fldr_pulldown** out);
/* (cycle - drop) x the inner fldr_rate_max_out, + 1 for a flush: the most frames one call can return; negative on a null handle */
FLDR_PULLDOWN_API int  fldr_pulldown_max_out(const fldr_pulldown* c);
/* Frame n of the stream.  host_outs may be NULL unless the push completes a cycle (n a multiple of cycle, n > 0): it must then be
 * fldr_pulldown_max_out frames, of which [0 .. *n_out - 1] are written.  report (may be NULL): see above. */
FLDR_PULLDOWN_API int  fldr_pulldown_push(fldr_pulldown* c, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                          fldr_pulldown_report* report);
/* End of the stream: the last frame is matched, the partial last cycle of m frames drops floor(m drop / cycle) by the same rule, its
 * survivors are pushed, then fldr_rate_flush of the inner converter follows.  host_outs: fldr_pulldown_max_out frames.  The frame
 * pushed after a flush is matched as the first frame of a stream is (no previous frame, no key) and begins a new cycle; the inner
 * converter goes on as a fldr_rate does after its flush. */
FLDR_PULLDOWN_API int  fldr_pulldown_flush(fldr_pulldown* c, const fldr_video_frame* host_outs, int* n_out, fldr_pulldown_report* report);
/* Forget everything pushed, here and in the inner converter: the next push is frame 0 of a new stream. */
FLDR_PULLDOWN_API int  fldr_pulldown_reset(fldr_pulldown* c);
FLDR_PULLDOWN_API void fldr_pulldown_destroy(fldr_pulldown* c);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_PULLDOWN_H */
