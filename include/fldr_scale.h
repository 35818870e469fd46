/*
 * fldr_scale.h — scale API of libfldr_scale.so: resizing of YUV 4:2:0 video on the device, placed on the cheaper side of the frame
 * interpolation, on top of the rate API (include/fldr_rate.h).  1080p24 becomes 2160p60 with the model run at 1080; 2160p becomes 1080p50
 * with the model run at 1080 too.
 *
 * Plain C99; no device header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Error codes.  This header defines no code of its own.  Its own argument errors — a null pointer, a size outside 1 .. 16384, more than
 * FLDR_SCALE_MAX_TAPS taps on an axis, a filter, kind or `where` out of range, a non-zero reserved word, an output that overlaps the
 * source, a null model where a forward runs, a workspace that is null, misaligned or short — return FLDR_RATE_E_ARG; a map that is null,
 * not created or destroyed returns FLDR_RATE_E_STATE; a ratio of the rates the converter does not take returns FLDR_RATE_E_RATIO; no such
 * device or a failed allocation returns FLDR_RATE_E_DEVICE.  Codes of the video and model libraries pass through, and so does a positive
 * hipError_t.  fldr_scale_error_string is fldr_rate_error_string.
 *
 * Terms.  A frame is H x W in a fldr_video_format: NV12 or I420 at depth 8 or 10 (P010 and yuv420p10le included).  Odd sizes are allowed:
 * the chroma planes are ceil(W/2) x ceil(H/2).  The format is the same on both sides of a scale: layout and depth conversion are out of
 * scope.  The sample value s(.) is the byte at depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le; D is the depth, mx = 255 or
 * 1023, e = 14 - D (6 or 4).
 *
 * THE RULE.  A scale is separable: horizontal first, then vertical, in every plane.  An axis of a plane is described by a tap count n
 * and, for every output index o, a first source index left[o] and n signed 16-bit coefficients q[o][0 .. n-1] with 14 fraction bits
 * that sum to EXACTLY 16384.  A source index is clamped to the plane: clamp(left[o] + k, 0, N - 1).
 *
 *   Tables (fldr_scale_taps, pure host arithmetic).  r = luma_in / luma_out as an exact rational, s = max(1, r), a the filter's radius:
 *     n = 2 ceil(a s), the same for luma and chroma;
 *     the centre c of output o:
 *       luma, either axis                                      c = (o + 1/2) r - 1/2
 *       chroma rows (4:2:0, sited between the luma rows)       c = (o + 1/2) r - 1/2      on chroma row indices
 *       chroma columns (sited "left": on the even luma column,  c = o r + (r - 1) / 4      on chroma column indices
 *         as fldr_video.h defines it)
 *     left = floor(c) - n/2 + 1, exactly, in integers;
 *     w_k = f((left + k - c) / s);  x_k = 16384 w_k / sum(w);  q_k = rint(x_k), half to even; the residual 16384 - sum(q) is added to the
 *     largest q_k (the lowest k among equals).
 *   Chroma uses the LUMA ratio r, not the ratio of its own plane sizes (they differ at odd sizes), and the chroma-column centre is what a
 *   plain per-plane resize gets wrong: at 2x up (r = 1/2) c = o/2 - 1/8, not o/2 - 1/4.
 *     FLDR_SCALE_BILINEAR   a = 1   f = max(0, 1 - |x|)
 *     FLDR_SCALE_BICUBIC    a = 2   Catmull-Rom (Keys, -0.5): 1.5|x|^3 - 2.5|x|^2 + 1 below 1, -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 below 2
 *     FLDR_SCALE_LANCZOS3   a = 3   sinc(x) sinc(x/3) below 3
 *   With r = 1 every row of every table is a single 16384: identity sizes give identity samples.
 *
 *   Arithmetic, all integer.
 *     horizontal   m = (sum_k qx[k] s(x_k) + (1 << (13 - e))) >> (14 - e), the shift arithmetic (floor); m is held as int16
 *     vertical     o = clamp((sum_k qy[k] m(y_k) + (1 << (13 + e))) >> (14 + e), 0, mx)
 *   The output is written in the container's canonical form: o << 6 for P010, the high bits zero for yuv420p10le.  These fit because
 *   fldr_scale_taps refuses a row with sum|q| > 32767: |m| <= 1023 x 16 x 32767 / 16384 < 32767, and the vertical sum stays below
 *   32767 x 32767 < 2^31.  The worst row of the three filters over the sizes tried is Lanczos3 at 33 -> 32 with sum|q| = 25424, so the
 *   refusal guards the arithmetic and never meets a real table.  With identity sizes m = 2^e s and o = s.  tests/scale_oracle.py is the
 *   numpy statement of all this.
 *
 *   Limits: every luma size is 1 .. FLDR_SCALE_MAX_SIZE = 16384, and n <= FLDR_SCALE_MAX_TAPS = 64 on both axes: Lanczos3 shrinks by at
 *   most 10.66, bicubic by 16, bilinear by 32.  Anything else is FLDR_RATE_E_ARG, before any device call.
 *
 * Four layers:
 *
 * 1. fldr_scale_taps_count, fldr_scale_taps: the tables, on the host.
 *
 * 2. fldr_scale_map_create, fldr_scale_frame: the tables of one in size -> out size in one format, uploaded once (the map is read-only
 *    afterwards and may serve any number of streams and threads), and the kernel that scales one device frame with them: one launch for
 *    all planes, both passes in it, the int16 intermediate in LDS.  The create fills the caller's fldr_scale_map: the resolved `where`,
 *    the tap counts and the tile each plane kind is cut into.
 *
 * 3. fldr_scale_forward: the forward of a pair placed by map->where.
 *      FLDR_SCALE_BEFORE  in[0], in[1] are scaled into two temporaries at the out size, then fldr_rate_forward (scene = 1) or
 *                         fldr_video_forward (scene = 0) runs at the out size straight into io->v.out
 *      FLDR_SCALE_AFTER   the forward runs at the in size into n_t temporaries, then one fldr_scale_frame per output
 *    FLDR_SCALE_AUTO resolves at the create: BEFORE iff out_H x out_W < in_H x in_W; equal pixel counts resolve to AFTER.  The forward is
 *    about linear in the pixel count, so it runs at the smaller size.  fldr_scale_temp_frame says where temporary k lives: after a
 *    forward the temporaries hold, byte for byte, what the underlying calls give.
 *
 * 4. fldr_scale_* streams: host frames at the in size and in_num / in_den per second in, host frames at the out size and out_num /
 *    out_den out.  The schedule is fldr_rate.h's.  Each pushed frame is uploaded once; with BEFORE it is scaled once, at the upload, not
 *    once per pair.  With equal rates (B == 1) no forward ever runs: the model may then be NULL and no model workspace is allocated — a
 *    pure scaling stream.
 *      Contract of the stream.  BEFORE: output j is, byte for byte, output j of a fldr_rate of the same rates and scene settings at the
 *    OUT size, pushed the scaled frames.  AFTER: output j is, byte for byte, the scale of output j of a fldr_rate at the IN size pushed
 *    the same frames — the outputs that land on an input frame and the ones replaced on a cut included (tests/test_gpu_scale.py holds
 *    both against the fldr_rate binding and tests/scale_oracle.py).  After a failed enqueue or wait the object is as after a reset.
 *    Argument errors change nothing.  One thread drives a stream.
 *
 * Contract of fldr_scale_frame and fldr_scale_forward: fldr_scene_measure's.  They enqueue on `stream`; no allocation, no
 * synchronisation, no host<->device copy: they can be captured into a graph.  Every argument is validated before anything is enqueued.
 * Output bytes between a row's end and its pitch are never written.  `out` must not overlap `in`.
 *
 * Known costs and limits:
 *   - the filters are fixed and linear in code values: no linear-light scaling and no ringing control;
 *   - chroma siting is "left" only;
 *   - 4:2:2, 4:4:4, packed and RGB formats are out of scope;
 *   - there is no cropping or aspect handling: the caller picks the sizes;
 *   - the stream is synchronous: it synchronises in every push, as the rate converter does;
 *   - the table builder uses the host's sin, so two hosts may differ by one unit in a coefficient; the kernel is exact for the tables it
 *     is given.
 */
#ifndef FLDR_SCALE_H
#define FLDR_SCALE_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_SCALE_VERSION 100           /* major*10000 + minor*100 + patch of this header */

#define FLDR_SCALE_API __attribute__((visibility("default")))

#define FLDR_SCALE_MAX_SIZE  16384       /* the largest luma size, either axis, either side */
#define FLDR_SCALE_MAX_TAPS  64          /* the most taps of an axis */

#define FLDR_SCALE_BILINEAR  0
#define FLDR_SCALE_BICUBIC   1
#define FLDR_SCALE_LANCZOS3  2

#define FLDR_SCALE_LUMA      0           /* kind of a table: luma, either axis */
#define FLDR_SCALE_CHROMA_H  1           /* chroma columns */
#define FLDR_SCALE_CHROMA_V  2           /* chroma rows */

#define FLDR_SCALE_BEFORE    0           /* scale, then interpolate at the out size */
#define FLDR_SCALE_AFTER     1           /* interpolate at the in size, then scale */
#define FLDR_SCALE_AUTO      2           /* whichever runs the forward on fewer pixels */

#define FLDR_SCALE_READ_AUTO   0         /* the library's pick (below) */
#define FLDR_SCALE_READ_DIRECT 1         /* every tap of the horizontal pass loads its sample from global memory */
#define FLDR_SCALE_READ_STAGED 2         /* the source rows of a tile go through LDS, each sample loaded once */

#define FLDR_SCALE_MAP_LIVE  0x5ca1e001  /* fldr_scale_map.live of a created map; 0 before the create and after the destroy */

FLDR_SCALE_API int         fldr_scale_version(void);
FLDR_SCALE_API const char* fldr_scale_error_string(int code);
/* 0: sizeof(fldr_scale_map_config), 1: fldr_scale_map, 2: fldr_scale_io, 3: fldr_scale_config — binding self-check; FLDR_RATE_E_ARG
 * otherwise */
FLDR_SCALE_API int         fldr_scale_sizeof(int which);

/* ---- the tables: pure host arithmetic, no device is touched ---------------------------------------------------------------------------- */
/* n of luma_in -> luma_out under `filter`; FLDR_RATE_E_ARG for a size outside 1 .. FLDR_SCALE_MAX_SIZE, a filter out of range or
 * n > FLDR_SCALE_MAX_TAPS */
FLDR_SCALE_API int fldr_scale_taps_count(int luma_in, int luma_out, int filter);
/* The table of one axis of one plane kind.  left: one int32 per output; coef: outputs x n int16, row o at coef + o n.  The outputs are
 * luma_out for FLDR_SCALE_LUMA and ceil(luma_out / 2) for the chroma kinds.  FLDR_RATE_E_ARG as fldr_scale_taps_count, for a kind out of
 * range, a null pointer, or a row with sum|q| > 32767. */
FLDR_SCALE_API int fldr_scale_taps(int luma_in, int luma_out, int filter, int kind, int32_t* left, int16_t* coef);

/* ---- the map: the tables of one scale on the device ------------------------------------------------------------------------------------- */
typedef struct fldr_scale_map_config {
    int32_t           in_H, in_W;        /* luma size of the source frames */
    int32_t           out_H, out_W;      /* luma size of the scaled frames */
    fldr_video_format format;            /* of both sides */
    int32_t           filter;            /* FLDR_SCALE_BILINEAR / _BICUBIC / _LANCZOS3 */
    int32_t           device;            /* HIP device ordinal */
    int32_t           where;             /* FLDR_SCALE_BEFORE / _AFTER / _AUTO: read by fldr_scale_forward alone */
    int32_t           read;              /* FLDR_SCALE_READ_AUTO / _DIRECT / _STAGED: how the kernel's horizontal pass reads its source */
    int32_t           reserved[3];       /* zero */
} fldr_scale_map_config;

typedef struct fldr_scale_map {          /* filled by fldr_scale_map_create, read-only afterwards */
    fldr_scale_map_config cfg;           /* as given */
    int32_t  where;                      /* resolved: FLDR_SCALE_BEFORE or FLDR_SCALE_AFTER */
    int32_t  taps_x, taps_y;             /* n of the horizontal and of the vertical axis */
    int32_t  tile_w[2];                  /* [0] luma, [1] chroma planes: the samples of an output row one workgroup owns (NV12 chroma: U and V both count) */
    int32_t  tile_h[2];                  /* ... and its output rows, picked so that the workgroup's LDS stays at or below 65536 bytes */
    int32_t  lds_bytes;                  /* of a workgroup */
    int32_t  live;                       /* FLDR_SCALE_MAP_LIVE */
    void*    tables;                     /* device memory: the four axis tables */
    int64_t  offset[8];                  /* of left and coef of luma x, luma y, chroma x, chroma y inside `tables` */
    int32_t  read;                       /* resolved: FLDR_SCALE_READ_DIRECT or FLDR_SCALE_READ_STAGED */
    int32_t  stage_span[2];              /* STAGED: the samples of a source row a tile of luma / chroma keeps in LDS; 0 otherwise */
    int32_t  stage_at;                   /* STAGED: where the staged rows begin in the workgroup's LDS, in bytes */
} fldr_scale_map;

/* Builds the four axis tables (luma and chroma, horizontal and vertical: a left and a coef array each) with fldr_scale_taps, uploads
 * them to cfg->device, synchronises, and fills *map.  Validation order: cfg / map null, the four sizes, filter, where, device negative,
 * read, the reserved words (FLDR_RATE_E_ARG); the format (FLDR_VIDEO_E_FORMAT); the tap limit of either axis, and FLDR_SCALE_READ_STAGED
 * where the staged rows do not fit (FLDR_RATE_E_ARG): all before any device call; then no such device or a failed allocation
 * (FLDR_RATE_E_DEVICE).  On an error *map is zeroed when it is not null.
 *   The two reads give the same bytes.  STAGED keeps 4 (depth 8) or 8 (depth 10) source rows of the tile's source columns in LDS as
 * 16-bit words at a time; it fits while that is at most 32768 bytes, i.e. while a tile's source span is at most 4096 (2048) samples:
 * every enlargement, and reductions up to about 15.  AUTO is STAGED where the width shrinks under bicubic or Lanczos3 and the rows
 * fit, DIRECT otherwise: the faster one in sixteen of the eighteen cases measured (DESIGN_LOG.md). */
FLDR_SCALE_API int  fldr_scale_map_create(const fldr_scale_map_config* cfg, fldr_scale_map* map);
/* Frees the tables and zeroes *map; a null or zeroed map is left alone.  No launch that reads the map may be in flight. */
FLDR_SCALE_API void fldr_scale_map_destroy(fldr_scale_map* map);

/* Enqueue the scale of `in` (device planes, cfg.in_H x cfg.in_W) into `out` (device planes, cfg.out_H x cfg.out_W), both in cfg.format.
 * Checked in this order: map null, not created or destroyed (FLDR_RATE_E_STATE); in / out null (FLDR_RATE_E_ARG); the planes, then the
 * pitches, of `in`, then of `out` (FLDR_VIDEO_E_PLANE / FLDR_VIDEO_E_PITCH); an `out` that overlaps `in` (FLDR_RATE_E_ARG).  An output
 * plane whose address and pitch are multiples of 16 is written 16 bytes at a time, any other sample by sample; the bytes are the same. */
FLDR_SCALE_API int  fldr_scale_frame(const fldr_scale_map* map, const fldr_video_frame* in, const fldr_video_frame* out, void* stream);

/* ---- the forward: a pair interpolated and scaled, in the order map->where says ------------------------------------------------------------ */
typedef struct fldr_scale_io {
    fldr_video_io     v;                 /* as fldr_rate_forward takes it, but H, W and in[2] are the map's IN size and out[k] its OUT size;
                                            n_t 1 .. FLDR_RATE_MAX_OUT; in_format == out_format == the map's */
    int32_t           scene;             /* 0: fldr_video_forward; 1: fldr_rate_forward (measure + select on a cut) */
    fldr_scene_params scene_params;      /* 0, 0 = the defaults */
    int32_t           reserved[4];       /* zero */
} fldr_scale_io;

/* With fH x fW the size the forward runs at (the out size under BEFORE, the in size under AFTER): fldr_rate_workspace_bytes(model, fH,
 * fW, n_t) rounded up to 256, plus the temporaries — 2 under BEFORE, n_t under AFTER — of fH x fW each in the map's format.  The scene state of a forward
 * with scene = 1, and so the pair's fldr_scene_result, is at ws + fldr_rate_workspace_bytes(model, fH, fW, n_t) -
 * FLDR_SCENE_STATE_BYTES.  Negative on bad arguments: FLDR_RATE_E_STATE for a bad map, FLDR_RATE_E_ARG for n_t outside 1 ..
 * FLDR_RATE_MAX_OUT, the video and model libraries' codes otherwise. */
FLDR_SCALE_API int64_t fldr_scale_workspace_bytes(const fldr_model* model, const fldr_scale_map* map, int n_t);
/* *frame = temporary k of a forward with n_t outputs in the workspace ws: planes in *fmt (the map's layout and depth: FLDR_RATE_E_FORMAT
 * otherwise) at fH x fW, every pitch a multiple of 16.
 * BEFORE: k = 0, 1 are the scaled in[0], in[1]; AFTER: k = 0 .. n_t - 1 are the forward's outputs before the scale. */
FLDR_SCALE_API int  fldr_scale_temp_frame(const fldr_model* model, const fldr_scale_map* map, const fldr_video_format* fmt, int n_t, int k, void* ws,
                                          fldr_video_frame* frame);
/* Enqueue on `stream`, after all validation and nothing else.  Checked in this order: io null (FLDR_RATE_E_ARG); the map
 * (FLDR_RATE_E_STATE); H, W against the map's in size, n_t, t / out null, scene, the reserved words, the scene thresholds
 * (FLDR_RATE_E_ARG); the formats (FLDR_VIDEO_E_FORMAT; FLDR_RATE_E_FORMAT where they differ from each other or from the map's); planes,
 * then pitches, of in[0] and in[1], then of every out[k]; a null model (FLDR_RATE_E_ARG); the workspace size (the model's code for a
 * frame it does not take); ws null, not 256-byte aligned or shorter than fldr_scale_workspace_bytes, an out[k] that overlaps an input
 * or lies inside ws (FLDR_RATE_E_ARG). */
FLDR_SCALE_API int  fldr_scale_forward(const fldr_model* model, const fldr_scale_map* map, const fldr_scale_io* io, void* ws, int64_t ws_bytes,
                                       void* stream);

/* ---- the stream: host frames at the in size and rate in, host frames at the out size and rate out ---------------------------------------- */
typedef struct fldr_scale_config {
    fldr_rate_config rate;               /* as fldr_rate_create takes it; H, W: the IN size */
    int32_t          out_H, out_W;       /* luma size of the frames returned */
    int32_t          filter;             /* FLDR_SCALE_BILINEAR / _BICUBIC / _LANCZOS3 */
    int32_t          where;              /* FLDR_SCALE_BEFORE / _AFTER / _AUTO */
    int32_t          reserved[4];        /* zero */
} fldr_scale_config;

typedef struct fldr_scale fldr_scale;

/* Validation order: cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words,
 * thresholds, format, rate terms, the ratio of the rates: FLDR_RATE_E_RATIO); then this library's own words: the sizes against
 * FLDR_SCALE_MAX_SIZE, filter, where, the reserved words and the tap limit (FLDR_RATE_E_ARG); then a null model with B != 1
 * (FLDR_RATE_E_ARG) and the model's code for a frame it does not take: all before any device call.  Then no such device or a failed
 * allocation (FLDR_RATE_E_DEVICE).  On success cfg->where is overwritten with the resolved placement (FLDR_SCALE_BEFORE or
 * FLDR_SCALE_AFTER); nothing else of *cfg is written, and nothing at all on an error. */
FLDR_SCALE_API int  fldr_scale_create(const fldr_model* model, fldr_scale_config* cfg, fldr_scale** out);
/* ceil(B / A): the most frames one push can return; negative (FLDR_RATE_E_ARG) on a null handle */
FLDR_SCALE_API int  fldr_scale_max_out(const fldr_scale* s);
/* Frame n of the stream, at the in size.  host_outs: fldr_scale_max_out frames at the out size, of which [0 .. *n_out - 1] are written
 * (may be NULL when no output is due).  scene (may be NULL): as fldr_rate_push fills it — measured at the size the forward runs at.
 * Synchronises before it returns. */
FLDR_SCALE_API int  fldr_scale_push(fldr_scale* s, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                    fldr_scene_result* scene);
/* End of the stream: the one output, if any, that lands exactly on the last pushed frame.  A second flush returns none. */
FLDR_SCALE_API int  fldr_scale_flush(fldr_scale* s, const fldr_video_frame* host_outs, int* n_out);
/* Forget everything pushed: the next push is frame 0 of a new stream, output 0 included. */
FLDR_SCALE_API int  fldr_scale_reset(fldr_scale* s);
FLDR_SCALE_API void fldr_scale_destroy(fldr_scale* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_SCALE_H */
