/*
 * fldr_cadence.h — cadence API of libfldr_cadence.so: drop the repeated frames of a container stream (24 fps film in 60p, 25 in 50p,
 * animation on twos, captures) and convert the survivors with the rate converter of include/fldr_rate.h.
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Two layers:
 *   - fldr_repeat_measure: how much, and where, two frames differ, per tile of 32 x 32 luma samples, in integers;
 *   - fldr_cadence_* streams: container frames in; of every `cycle` frames the `drop` that differ least from their predecessors are
 *     taken out, the others go, in order, into a fldr_rate whose input rate is the container's x (cycle - drop) / cycle.
 *
 * The repeat measure.  y8(sample) is fldr_rate.h's: the byte at depth 8, word >> 8 for P010, (word & 0x3ff) >> 2 for yuv420p10le.
 * Only plane 0 is read.  The plane is cut into tiles of 32 x 32 samples; tile (ty, tx) covers rows 32 ty .. min(32 ty + 31, H - 1) and
 * the same in columns (edge tiles are partial); tiles_x = ceil(W / 32), the tile's index is ty * tiles_x + tx.
 *     tile_sad(i)  = sum over tile i of |y8(I0) - y8(I1)|                                (0 .. 32 x 32 x 255 = 261120)
 *     sad          = sum over all tiles of tile_sad
 *     max_tile_sad = the largest tile_sad, max_tile = the lowest index that attains it (0 when the frames are equal)
 *     moving_tiles = the number of tiles with tile_sad >= tile_sad_min
 *     repeat       = moving_tiles == 0
 * A whole-frame sum cannot tell a re-encoded repeat (a little noise everywhere) from a small object moving on a still background (a
 * lot in one place); the largest tile can.  Everything is an integer sum, maximum or count, so the result does not depend on the order
 * of the reduction: it is the same from run to run and equal to the numpy statement of tests/cadence_oracle.py.
 * FLDR_REPEAT_TILE_SAD_DEFAULT (a mean difference of two codes over a full tile) was set on synthetic content only — moving textures,
 * repeats perturbed by a code here and there —, not on footage: a maintainer with re-encoded material should look at max_tile_sad of
 * its repeats and set tile_sad_min above it.
 *
 * Contract of fldr_repeat_measure (that of fldr_scene_measure): it enqueues on `stream`; no allocation, no synchronisation, no
 * host<->device copy: it can be captured into a graph.  Arguments are validated before anything is enqueued.  `state` needs no
 * preparation: the library zeroes what it uses, on the stream.  Calls with different `state` may be in flight on different streams.
 *
 * The cadence is declared, not guessed (as with ffmpeg's decimate): 3:2 pulldown in 60p is cycle 5, drop 3; 2:2 is 2, 1; 24 fps in 30p
 * is 5, 1; 1, 0 is plain fldr_rate.  WHICH frames of a cycle go is measured.  Frame n of the stream (n from 0) belongs to cycle
 * n / cycle.  Its key is (max_tile_sad, sad) of the pair (n - 1, n), compared lexicographically; frame 0 of a stream has no key and is
 * never dropped.  When a cycle is complete the `drop` frames with the smallest keys are dropped, the lower frame number first among
 * equal keys.  (Any window of one period of a periodic pattern holds the same number of repeats, so no phase is tracked.  A still
 * scene loses `drop` frames that are all alike; a cut inside a cycle has the largest key and stays.)  The survivors are treated as
 * equally spaced in time and pushed, in order, into a fldr_rate created with cfg.rate, its input rate replaced by
 * in_num (cycle - drop) / (in_den cycle) reduced by the gcd (fldr_cadence_inner_rate).
 *
 * Contract of the stream: the frames fldr_cadence_push and fldr_cadence_flush return are, byte for byte and in order, what
 * fldr_rate_push and fldr_rate_flush return on a fldr_rate of that derived configuration pushed the survivor sequence
 * (tests/test_gpu_cadence.py holds the two together).  After any failed enqueue or wait the object is as after a reset.  Argument
 * errors change nothing.  One thread drives a stream.
 *
 * Known costs and limits:
 *   - a survivor is uploaded twice: once here for the measure, once by the inner fldr_rate_push;
 *   - a stream that starts in the middle of a run of repeats may lose one real frame in its first cycle, and so may a cycle that
 *     straddles an edit that breaks the cadence: moving_dropped of the report says so;
 *   - outputs arrive one cycle late;
 *   - cycle and drop are not detected, interlaced fields are not handled, and the stream is synchronous: it is built on fldr_rate, not
 *     on the converter with frames in flight.
 *
 * Every function returns 0, a negative FLDR_CADENCE_E_* code, a negative FLDR_RATE_E_*, FLDR_VIDEO_E_* or FLDR_MODEL_E_* code passed
 * through, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_CADENCE_H
#define FLDR_CADENCE_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_CADENCE_VERSION 100         /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -600 and below, apart from the ranges of the libraries below it */
#define FLDR_CADENCE_E_ARG      (-600)   /* null pointer, bad size, tile_sad_min outside 0 .. 261120, cycle / drop out of range, non-zero reserved word, null model */
#define FLDR_CADENCE_E_STATE    (-601)   /* repeat state null or not 256-byte aligned */
#define FLDR_CADENCE_E_DEVICE   (-602)   /* stream: no such device, or an allocation failed */

#define FLDR_CADENCE_API __attribute__((visibility("default")))

#define FLDR_REPEAT_TILE              32      /* samples per tile side */
#define FLDR_REPEAT_TILE_SAD_MAX      261120  /* 32 x 32 x 255 */
#define FLDR_REPEAT_TILE_SAD_DEFAULT  2048    /* a mean difference of two codes over a full tile; set on synthetic content only */
#define FLDR_REPEAT_STATE_BYTES       4096    /* device memory, 256-byte aligned; begins with a fldr_repeat_result, the rest is the kernels' */
#define FLDR_CADENCE_MAX_CYCLE        16

typedef struct fldr_repeat_params {
    int32_t tile_sad_min;                /* 1 .. 261120; 0: FLDR_REPEAT_TILE_SAD_DEFAULT */
    int32_t reserved[3];                 /* zero */
} fldr_repeat_params;

typedef struct fldr_repeat_result {      /* 32 bytes, at the start of the repeat state */
    uint64_t sad;
    uint32_t max_tile_sad;
    uint32_t max_tile;                   /* the lowest tile index that attains max_tile_sad */
    uint32_t moving_tiles;               /* tiles with tile_sad >= tile_sad_min */
    uint32_t repeat;                     /* 1 when moving_tiles == 0 */
    uint32_t reserved[2];                /* written as zero */
} fldr_repeat_result;

FLDR_CADENCE_API int         fldr_cadence_version(void);
FLDR_CADENCE_API const char* fldr_cadence_error_string(int code);
/* 0: sizeof(fldr_repeat_params), 1: fldr_repeat_result, 2: fldr_cadence_config, 3: fldr_cadence_report — binding self-check;
 * FLDR_CADENCE_E_ARG otherwise */
FLDR_CADENCE_API int         fldr_cadence_sizeof(int which);

/* Enqueue the repeat measure of the pair in[0], in[1] (device planes in *fmt, any H, W from 1 to 2^31 - 33 with at most 2^31 - 1
 * tiles; only plane 0 is read, but every plane of the format is checked as fldr_scene_measure checks it).  p: NULL = the defaults.
 * After the stream reaches this point `state` begins with the pair's fldr_repeat_result. */
FLDR_CADENCE_API int fldr_repeat_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2],
                                         const fldr_repeat_params* p, void* state, void* stream);

/* ---- the stream: container frames in, converted frames out ------------------------------------------------------------------------- */
typedef struct fldr_cadence_config {
    fldr_rate_config   rate;             /* as fldr_rate_create takes it; in_num / in_den is the CONTAINER's rate */
    int32_t            cycle;            /* 1 .. FLDR_CADENCE_MAX_CYCLE */
    int32_t            drop;             /* 0 .. cycle - 1 frames of every cycle are repeats */
    fldr_repeat_params repeat;           /* 0 = the default */
    int32_t            reserved[2];      /* zero */
} fldr_cadence_config;

typedef struct fldr_cadence_report {     /* of the cycle a push completed, or the partial cycle a flush ended; all zero otherwise */
    int64_t  first_frame;                /* stream number of the cycle's frame 0 */
    uint32_t n_frames;                   /* frames in it: cycle, or fewer at a flush */
    uint32_t dropped_mask;               /* bit k: frame first_frame + k was dropped */
    uint32_t moving_dropped;             /* dropped frames with repeat == 0: the declared cadence is wrong, or broken at an edit */
    uint32_t still_kept;                 /* kept frames with repeat == 1 */
    uint32_t cut_mask;                   /* bit k: the pair that ended in the cycle's k-th survivor was a cut for the inner converter */
    uint32_t reserved;                   /* zero */
    fldr_repeat_result measure[FLDR_CADENCE_MAX_CYCLE];   /* [k]: of the pair (first_frame + k - 1, first_frame + k); zero for stream frame 0 */
} fldr_cadence_report;

typedef struct fldr_cadence fldr_cadence;

/* *num / *den = in_num (cycle - drop) / (in_den cycle), reduced: the input rate of the inner fldr_rate.  FLDR_CADENCE_E_ARG on a null
 * pointer or cycle / drop out of range, FLDR_RATE_E_RATIO when in_num or in_den is not positive or a reduced term does not fit int32. */
FLDR_CADENCE_API int  fldr_cadence_inner_rate(const fldr_cadence_config* cfg, int32_t* num, int32_t* den);
/* cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words, thresholds,
 * format, rate terms), then cycle, drop, repeat and the reserved words (FLDR_CADENCE_E_ARG), then the derived rate and its ratio to the
 * output rate (FLDR_RATE_E_RATIO), then a null model (FLDR_CADENCE_E_ARG): all before any device call. */
FLDR_CADENCE_API int  fldr_cadence_create(const fldr_model* model, const fldr_cadence_config* cfg, fldr_cadence** out);
/* (cycle - drop) x the inner fldr_rate_max_out, + 1 for a flush: the most frames one call can return; negative on a null handle */
FLDR_CADENCE_API int  fldr_cadence_max_out(const fldr_cadence* c);
/* Frame n of the stream.  A push that does not complete a cycle packs the frame into pinned memory, enqueues its upload, the repeat
 * measure of the pair (n - 1, n) and a 32-byte copy of the result, and returns *n_out = 0 without synchronising; host_outs may then
 * be NULL.  The push that completes a cycle synchronises once, chooses the drops and pushes the survivors into the inner converter:
 * host_outs must then be fldr_cadence_max_out frames, of which [0 .. *n_out - 1] are written.  report (may be NULL): see above. */
FLDR_CADENCE_API int  fldr_cadence_push(fldr_cadence* c, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                        fldr_cadence_report* report);
/* End of the stream: the partial last cycle of m frames drops floor(m drop / cycle) by the same rule, its survivors are pushed, then
 * fldr_rate_flush of the inner converter follows.  host_outs: fldr_cadence_max_out frames.  A push after a flush begins a new cycle;
 * the inner converter goes on as a fldr_rate does after its flush. */
FLDR_CADENCE_API int  fldr_cadence_flush(fldr_cadence* c, const fldr_video_frame* host_outs, int* n_out, fldr_cadence_report* report);
/* Forget everything pushed, here and in the inner converter: the next push is frame 0 of a new stream. */
FLDR_CADENCE_API int  fldr_cadence_reset(fldr_cadence* c);
FLDR_CADENCE_API void fldr_cadence_destroy(fldr_cadence* c);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_CADENCE_H */
