/*
 * fldr_probe.h — probe API of libfldr_probe.so: what kind of material a stream of 4:2:0 frames carries — progressive frames (with or
 * without repeated frames), film in interlaced video (with its pulldown cadence), or true interlaced video (with its field order) —
 * measured on the GPU in one pass per frame and classified on the host.  The answer names the converter the stream belongs in and the
 * declaration that converter needs.
 *
 * Plain C99; no device header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h, and needs no fldr_model: no forward runs.
 *
 * Error codes.  This header defines no code of its own.  Its own argument errors — a null pointer, a bad size, H not a multiple of 4, a
 * parameter out of range, a non-zero reserved word, a window outside 3 .. 64 — return FLDR_RATE_E_ARG; a measure state that is null or
 * not 256-byte aligned returns FLDR_RATE_E_STATE; no such device or a failed allocation returns FLDR_RATE_E_DEVICE.  Codes of the video
 * library (format, planes, pitches) pass through, and so does a positive hipError_t.  fldr_probe_error_string is fldr_rate_error_string.
 *
 * Terms.  A frame is H x W in a fldr_video_format: NV12 or I420 at depth 8 or 10 (P010 and yuv420p10le included).  H is a multiple of 4
 * and at least 4, W >= 1.  y8(sample) is fldr_rate.h's: the byte at depth 8, word >> 8 for P010, (word & 0x3ff) >> 2 for yuv420p10le.
 * Only plane 0 is read.  The plane is cut into tiles of 32 x 32 luma samples; tile (ty, tx) covers rows 32 ty .. min(32 ty + 31, H - 1)
 * and the same in columns (edge tiles are partial); tiles_x = ceil(W / 32), the tile's index is ty * tiles_x + tx.  S_k is the frame of
 * candidate k: FLDR_PROBE_C (0) cur itself, FLDR_PROBE_P (1) the previous frame, FLDR_PROBE_N (2) the next frame.
 *
 * Three layers:
 *
 * 1. fldr_probe_measure: every word below for the frame `cur` against `prev` and `next`, in one pass over the three luma planes.
 *      Comb words, for the anchor parity q in {0, 1} and the candidate k.  For every row y with y % 2 != q and 1 <= y <= H - 2, and
 *      every x:
 *          a = y8(cur[y-1][x]), b = y8(cur[y+1][x]), m = y8(S_k[y][x]);
 *          the sample is combed when (a - m) * (b - m) > comb_thresh * comb_thresh  (strict; the product is an integer): m lies
 *          outside the span of the lines of cur above and below it, by more than comb_thresh on both sides.
 *          comb[q][k]          = the number of combed samples
 *          max_tile_comb[q][k] = the largest number in one tile (0 .. 512), max_tile[q][k] = the lowest tile index that attains it (0
 *                                when no sample is combed)
 *      Field SAD words, for the field parity p.  Over the rows y % 2 == p, tile_sad_p(i) = sum over tile i of |y8(cur) - y8(prev)|:
 *          field_sad[p], field_max_tile_sad[p] (0 .. 16 x 32 x 255 = 130560), field_max_tile[p] (the lowest index),
 *          field_moving_tiles[p] = the tiles with tile_sad_p >= tile_sad_min.
 *      Whole-frame motion.  frame_moving_tiles = the tiles with tile_sad_0 + tile_sad_1 >= frame_tile_sad_min;
 *          repeat = (frame_moving_tiles == 0): cur repeats prev.
 *      Order sums.  For the candidate k and the row parity p,
 *          lap[k][p] = sum of |y8(cur[y-1][x]) + y8(cur[y+1][x]) - 2 y8(S_k[y][x])| over the rows y % 2 == p with 1 <= y <= H - 2 and
 *          every x (a uint64; a tile contributes at most 16 x 32 x 510 = 261120);
 *          tff_sum = lap[P][1] + lap[N][0],  bff_sum = lap[P][0] + lap[N][1].
 *      With the top field first, the odd rows of prev and the even rows of next are one field interval away from the lines of cur
 *      around them; the other two pairings are three intervals away.  So the smaller sum is on the true order's side.
 *      A frame that is NULL is not measured and its words are 0: comb, max_tile_comb, max_tile and lap of its candidate; without prev
 *      also every field_* word, frame_moving_tiles and repeat; tff_sum and bff_sum are 0 unless prev and next are both given.
 *    Everything is an integer sum, maximum, count or lowest index, so the result does not depend on the order of the reduction: it is
 *    the same from run to run and equal to the numpy statement of tests/probe_oracle.py.
 *    The defaults restate those of the stream libraries a verdict leads to (comb_thresh 6, comb_tile_min 32, tile_sad_min 1024 for a
 *    field; frame_tile_sad_min 2048 for a whole tile) and, like them, were set on this repository's synthetic content only — moving
 *    textures, telecined or woven from two instants —, not on footage.
 *
 * 2. fldr_probe_classify: a pure host function of M results of consecutive frames, each measured with both neighbours.
 *      Per frame.  moved = frame_moving_tiles > 0.  A frame that has not moved is still and takes no part in the class counts.  A moved
 *      frame is
 *          FLDR_PROBE_FRAME_PROG  when max_tile_comb[0][C] and max_tile_comb[1][C] are both below comb_tile_min;
 *          FLDR_PROBE_FRAME_FILM  when it is not PROG and, for both q, the smallest max_tile_comb[q][k] over k is below comb_tile_min;
 *          FLDR_PROBE_FRAME_VIDEO otherwise.
 *      A VIDEO frame votes tff when tff_sum < bff_sum, bff when tff_sum > bff_sum, and nothing when they are equal.
 *      Kind.  n_prog, n_film, n_video are the numbers of moved frames of each class (the verdict carries them as counted); for the rules
 *      below a class with at most max_outliers frames counts as 0.  In this order:
 *          fewer than min_moved moved frames            FLDR_PROBE_UNKNOWN
 *          n_video == 0 and n_film == 0                 FLDR_PROBE_PROGRESSIVE
 *          n_video == 0 (film frames present)           FLDR_PROBE_FILM
 *          n_film == 0 (video frames present)           FLDR_PROBE_INTERLACED; tff = 1 when more frames vote tff than bff, 0 when fewer,
 *                                                       -1 on a tie; mixed = (n_prog > 0)
 *          anything else                                FLDR_PROBE_MIXED
 *      tff is -1 and mixed is 0 for every other kind.
 *      Cadence, for PROGRESSIVE and FILM (cycle 1, drop 0, irregular 0, confirmed 0 otherwise).  r is a 0 / 1 sequence over the M
 *      frames: for PROGRESSIVE r[n] = the frame is still; for FILM r[n] = (field_moving_tiles[anchor] == 0), anchor from the parameters.
 *          cycle     = the smallest c in 1 .. 16 with c < M and r[n] == r[n + c] wherever both exist;
 *          drop      = the number of ones among the first `cycle` entries of r;
 *          r all zero gives 1, 0; no such c gives 1, 0 with irregular = 1;
 *          confirmed = the number of n with r[n] == 1, n + cycle < M and r[n + cycle] == 1 (0 when irregular).
 *      What to do with the verdict:
 *          PROGRESSIVE with drop == 0    the rate converter of fldr_rate.h
 *          PROGRESSIVE with drop > 0     the cadence stream (cycle, drop)
 *          FILM                          the pulldown stream (cycle, drop, anchor)
 *          INTERLACED                    the deinterlacer (tff)
 *      UNKNOWN and MIXED, an irregular cadence and a tff of -1 are for the caller to decide: the verdict carries every count and vote.
 *
 * 3. fldr_probe_* stream: host frames in, a verdict out.  The object keeps three frames on the device; each frame is uploaded once.  The
 *    push of frame n (n >= 2) enqueues the measure of frame n - 1 with prev = n - 2 and next = n and the copy of its result into a pinned
 *    ring of `window` entries; frame 0 has no previous frame and is not measured.  A push does not wait for the measure.
 *    fldr_probe_verdict_get synchronises and classifies what the ring holds: the results of the last min(n - 2, window) measured frames,
 *    oldest first.  After any failed enqueue or wait the object is as after a reset.  Argument errors change nothing.  One thread drives
 *    a stream.
 *
 * Contract of fldr_probe_measure: it enqueues on `stream`; no allocation, no synchronisation, no host<->device copy: it can be captured
 * into a graph.  Arguments are validated before anything is enqueued.  The state needs no preparation: the library zeroes what it uses,
 * on the stream.  Calls with different `state` may be in flight on different streams.  The frames are never written.  All offsets are
 * 64-bit: there is no frame-size limit beyond that of the tile index (H, W up to 2^31 - 33, at most 2^31 - 1 tiles).
 *
 * Known limits:
 *   - the comb measure is the plain three-line one: a one-line-high static detail scores in every candidate alike;
 *   - a cadence longer than 16 frames, or one that changes inside the window, is reported irregular;
 *   - a window shorter than two cycles can show a shorter period than the true one: `confirmed` counts the repeats seen twice;
 *   - the field order of film is not reported: the pulldown stream does not need it;
 *   - 4:2:2, packed and RGB formats are out of scope.
 */
#ifndef FLDR_PROBE_H
#define FLDR_PROBE_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_PROBE_VERSION 100           /* major*10000 + minor*100 + patch of this header */

#define FLDR_PROBE_API __attribute__((visibility("default")))

#define FLDR_PROBE_C 0                   /* candidates: the rows of cur itself, */
#define FLDR_PROBE_P 1                   /* of the previous frame, */
#define FLDR_PROBE_N 2                   /* of the next frame */

#define FLDR_PROBE_TILE                       32      /* samples per tile side */
#define FLDR_PROBE_TILE_COMB_MAX              512     /* 16 x 32: the rows of one parity of a tile */
#define FLDR_PROBE_TILE_SAD_MAX               130560  /* 16 x 32 x 255: one field of a tile */
#define FLDR_PROBE_FRAME_TILE_SAD_MAX         261120  /* 32 x 32 x 255: a whole tile */
#define FLDR_PROBE_COMB_THRESH_DEFAULT        6       /* set on synthetic content only */
#define FLDR_PROBE_COMB_TILE_DEFAULT          32      /* one sample in sixteen of a tile's rows of one parity; set on synthetic content only */
#define FLDR_PROBE_TILE_SAD_DEFAULT           1024    /* a mean difference of two codes over one field of a tile; set on synthetic content only */
#define FLDR_PROBE_FRAME_TILE_SAD_DEFAULT     2048    /* a mean difference of two codes over a full tile; set on synthetic content only */
#define FLDR_PROBE_MIN_MOVED_DEFAULT          4
#define FLDR_PROBE_STATE_BYTES                16384   /* device memory, 256-byte aligned; begins with a fldr_probe_result, the rest is the kernels' */
#define FLDR_PROBE_MAX_CYCLE                  16
#define FLDR_PROBE_MIN_WINDOW                 3
#define FLDR_PROBE_MAX_WINDOW                 64

#define FLDR_PROBE_UNKNOWN     0         /* kinds */
#define FLDR_PROBE_PROGRESSIVE 1
#define FLDR_PROBE_FILM        2
#define FLDR_PROBE_INTERLACED  3
#define FLDR_PROBE_MIXED       4

#define FLDR_PROBE_FRAME_STILL 0         /* classes of one frame */
#define FLDR_PROBE_FRAME_PROG  1
#define FLDR_PROBE_FRAME_FILM  2
#define FLDR_PROBE_FRAME_VIDEO 3

typedef struct fldr_probe_params {
    int32_t comb_thresh;                 /* 1 .. 255; 0: FLDR_PROBE_COMB_THRESH_DEFAULT */
    int32_t comb_tile_min;               /* 1 .. 512; 0: FLDR_PROBE_COMB_TILE_DEFAULT */
    int32_t tile_sad_min;                /* 1 .. 130560; 0: FLDR_PROBE_TILE_SAD_DEFAULT */
    int32_t frame_tile_sad_min;          /* 1 .. 261120; 0: FLDR_PROBE_FRAME_TILE_SAD_DEFAULT */
    int32_t min_moved;                   /* 1 .. 64; 0: FLDR_PROBE_MIN_MOVED_DEFAULT (the classifier's) */
    int32_t max_outliers;                /* 0 .. 64 (the classifier's) */
    int32_t anchor;                      /* 0 / 1: the field whose repeats give a film's cadence (the classifier's) */
    int32_t reserved[5];                 /* zero */
} fldr_probe_params;

typedef struct fldr_probe_result {       /* 256 bytes, at the start of the measure state */
    uint64_t comb[2][3];                 /* [q][k] */
    uint32_t max_tile_comb[2][3];
    uint32_t max_tile[2][3];             /* the lowest tile index that attains max_tile_comb */
    uint64_t field_sad[2];               /* [p] */
    uint32_t field_max_tile_sad[2];
    uint32_t field_max_tile[2];
    uint32_t field_moving_tiles[2];      /* tiles with tile_sad_p >= tile_sad_min */
    uint32_t frame_moving_tiles;         /* tiles with tile_sad_0 + tile_sad_1 >= frame_tile_sad_min */
    uint32_t repeat;                     /* 1 when prev is given and frame_moving_tiles == 0 */
    uint64_t lap[3][2];                  /* [k][p] */
    uint64_t tff_sum;                    /* lap[P][1] + lap[N][0] */
    uint64_t bff_sum;                    /* lap[P][0] + lap[N][1] */
    uint32_t reserved[12];               /* written as zero */
} fldr_probe_result;

typedef struct fldr_probe_verdict {      /* 96 bytes */
    int32_t kind;                        /* FLDR_PROBE_UNKNOWN .. _MIXED */
    int32_t tff;                         /* INTERLACED: 1 / 0 by majority, -1 on a tie; -1 otherwise */
    int32_t mixed;                       /* INTERLACED with progressive frames among the video */
    int32_t cycle;                       /* PROGRESSIVE, FILM: the cadence; 1, 0 otherwise */
    int32_t drop;
    int32_t anchor;                      /* the parameters' */
    int32_t irregular;                   /* r has no period of 1 .. 16 frames shorter than the window */
    int32_t confirmed;                   /* ones of r seen again one cycle later */
    int32_t n_frames;                    /* M */
    int32_t n_moved;
    int32_t n_still;
    int32_t n_prog;                      /* as counted, before max_outliers */
    int32_t n_film;
    int32_t n_video;
    int32_t votes_tff;                   /* VIDEO frames with tff_sum < bff_sum */
    int32_t votes_bff;
    int32_t reserved[8];                 /* zero */
} fldr_probe_verdict;

FLDR_PROBE_API int         fldr_probe_version(void);
FLDR_PROBE_API const char* fldr_probe_error_string(int code);
/* 0: sizeof(fldr_probe_params), 1: fldr_probe_result, 2: fldr_probe_verdict, 3: fldr_probe_config — binding self-check;
 * FLDR_RATE_E_ARG otherwise */
FLDR_PROBE_API int         fldr_probe_sizeof(int which);

/* Enqueue the measure of cur against prev and next (device planes in *fmt; only plane 0 is read, but every plane of every frame given
 * is checked as fldr_scene_measure checks it).  p: NULL = the defaults.  prev and next may each be NULL.  Checked in this order: fmt /
 * cur null, H and W (FLDR_RATE_E_ARG); the parameters (FLDR_RATE_E_ARG); the format; the planes, then the pitches, of cur, prev, next
 * (the video library's codes); the state (FLDR_RATE_E_STATE).  After the stream reaches this point `state` begins with the
 * fldr_probe_result. */
FLDR_PROBE_API int fldr_probe_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                                      const fldr_video_frame* next, const fldr_probe_params* p, void* state, void* stream);

/* The class of one frame (FLDR_PROBE_FRAME_*) by the rules above; FLDR_RATE_E_ARG on a null result or bad parameters.  Host only. */
FLDR_PROBE_API int fldr_probe_frame_class(const fldr_probe_result* r, const fldr_probe_params* p);

/* The verdict on results[0 .. M - 1] (host memory; M >= 0, results may be NULL when M == 0).  p: NULL = the defaults.  Host only, no
 * device call; FLDR_RATE_E_ARG on a null pointer, a negative M or bad parameters. */
FLDR_PROBE_API int fldr_probe_classify(const fldr_probe_result* results, int M, const fldr_probe_params* p, fldr_probe_verdict* out);

/* ---- the stream: host frames in, a verdict out -------------------------------------------------------------------------------------- */
typedef struct fldr_probe_config {
    int32_t           H, W;
    fldr_video_format format;
    int32_t           device;            /* >= 0 */
    int32_t           window;            /* FLDR_PROBE_MIN_WINDOW .. FLDR_PROBE_MAX_WINDOW results kept */
    fldr_probe_params params;            /* zeros = the defaults */
    int32_t           reserved[4];       /* zero */
} fldr_probe_config;

typedef struct fldr_probe fldr_probe;

/* Validation order: null pointers, H, W, device, window, the parameters, the reserved words (FLDR_RATE_E_ARG); the format (the video
 * library's code): all before any device call.  Then FLDR_RATE_E_DEVICE when the device or its memory cannot be had. */
FLDR_PROBE_API int  fldr_probe_create(const fldr_probe_config* cfg, fldr_probe** out);
/* Frame n of the stream (host planes). */
FLDR_PROBE_API int  fldr_probe_push(fldr_probe* c, const fldr_video_frame* host_frame);
/* Waits for what was enqueued, then classifies the ring (M = 0 .. window results: UNKNOWN while fewer than min_moved have moved). */
FLDR_PROBE_API int  fldr_probe_verdict_get(fldr_probe* c, fldr_probe_verdict* out);
/* Waits, then copies result i of the ring, 0 = the oldest held; FLDR_RATE_E_ARG when i is not below the number held (the verdict's
 * n_frames).  *frame (may be NULL) = the stream number of the frame it measures. */
FLDR_PROBE_API int  fldr_probe_result_get(fldr_probe* c, int i, fldr_probe_result* out, int64_t* frame);
/* Forget everything pushed: the next push is frame 0 of a new stream. */
FLDR_PROBE_API int  fldr_probe_reset(fldr_probe* c);
FLDR_PROBE_API void fldr_probe_destroy(fldr_probe* c);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_PROBE_H */
