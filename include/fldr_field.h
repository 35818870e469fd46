/*
 * fldr_field.h — field API of libfldr_field.so: motion-compensated deinterlacing of interlaced 4:2:0 video (1080i, 576i, 480i) on
 * top of the rate converter's cut measure (include/fldr_rate.h) and the video API (include/fldr_video.h).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * An interlaced frame holds two instants.  The missing lines of field m are the picture at time m on the line grid that fields m - 1
 * and m + 1 sample: the model's forward at t = 0.5 on that half-height pair.  Three layers:
 *   - fldr_field_weave: one kernel that puts a field and an estimate of its missing lines together, guarded in integers;
 *   - fldr_field_forward: fldr_scene_measure + fldr_video_forward on the two neighbouring fields (zero-copy views) + the weave;
 *   - fldr_field_* streams: woven host frames in, progressive host frames out, one per frame or one per field.
 *
 * Terms.  A frame is H x W in a fldr_video_format (NV12 / I420, depth 8 / 10, so P010 and yuv420p10le are included).  H is a multiple
 * of 4 and at least 4 (FLDR_FIELD_E_SIZE otherwise), so that the chroma planes, H / 2 rows, also split into two fields of whole rows.
 * Frame k of a stream (from 0) holds fields 2k and 2k + 1.  The parity of field m is par(m) = (m & 1) ^ (tff ? 0 : 1); in every plane
 * the field is the rows y = par(m) (mod 2).  The field view of a frame is, for each plane, plane + par * pitch with pitch 2 * pitch,
 * of size H / 2 x W: no copy is made.
 *
 * The weave.  The rule below is applied to every plane alike, and to each component of the interleaved NV12 chroma plane alike.  A
 * plane has R rows and C samples per component and row.  v(.) is the sample value: the byte at depth 8, word >> 6 for P010,
 * word & 0x3ff for yuv420p10le; mx is 255 or 1023.
 *   - Rows with y % 2 == parity: the row bytes of `cur`, copied as they are (P010: the low six bits included).
 *   - The other rows:  a = v(cur[y-1][x]), taken from row y + 1 when y == 0;  b = v(cur[y+1][x]), taken from row y - 1 when y == R - 1.
 *       INTRA:   o = (a + b + 1) >> 1
 *       MOTION:  d = max over x' in {max(x-1, 0), x, min(x+1, C-1)} of |v(prev[y][x']) - v(next[y][x'])|
 *                if still >= 0 && d <= still:   o = (v(prev[y][x]) + v(next[y][x]) + 1) >> 1
 *                otherwise:                     o = min(max(v(temporal[y>>1][x]), max(min(a,b) - slack, 0)), min(max(a,b) + slack, mx))
 *     o is written in the container's canonical form: o << 6 for P010, o with the high bits zero for yuv420p10le.
 * The static rule makes a still picture come back exactly, whatever the model says; the clamp keeps a wrong motion estimate inside
 * what the field's own neighbouring lines allow.  Both are the usual guards of motion-adaptive deinterlacers, stated in integers:
 * the result is equal, byte for byte, to the numpy statement of tests/field_oracle.py.
 * `still` (-1 .. mx; -1: the static rule is off) and `slack` (0 .. mx) are in the format's own code units.  The defaults,
 * FLDR_FIELD_STILL_DEFAULT8 << (depth - 8) and FLDR_FIELD_SLACK_DEFAULT8 << (depth - 8), were set on synthetic content only — moving
 * textures, still pictures with a code of noise —, not on footage: a maintainer with interlaced material should look at the combing
 * left on its still areas and the softness on its moving ones and set the two from that.
 *
 * Contract of fldr_field_weave (that of fldr_scene_measure) and fldr_field_forward: they enqueue on `stream`; no allocation, no
 * synchronisation, no host<->device copy: they can be captured into a graph.  Every argument is validated before anything is
 * enqueued.  Output bytes between a row's end and its pitch are never written.  `out` must not overlap an input.
 * fldr_field_forward: a device fault flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); the cut
 * measure and the input conversion have then been enqueued, `out` is untouched.  Fields too small for the model are refused as the
 * model refuses them (FLDR_MODEL_E_SHAPE): its reflect padding needs pad < size, and with the shipped five scales a field of 128
 * rows (a frame of 256) is refused while one of 200 rows (a frame of 400) is fine.
 *
 * The schedule of a stream (fldr_field_plan).  Output j carries field m = j at rate 2 (one output per field) and m = 2j at rate 1
 * (one per frame, the even fields only).  Its `cur` is frame m >> 1; fields m - 1 and m + 1 are in frames (m - 1) >> 1 and
 * (m + 1) >> 1.  Field 0 has no predecessor and the last field of a stream no successor: they are woven in INTRA mode.  At rate 2
 * the push of frame 0 returns field 0, every later push of frame n returns fields 2n - 1 and 2n, and fldr_field_flush returns the
 * last field: 2N outputs for N frames.  At rate 1 every push returns one frame and a flush none.
 *
 * Known limits:
 *   - each field is treated as a progressive half-height 4:2:0 picture, so the chroma siting inside a field is off by a quarter line;
 *   - 4:2:2, packed and RGB interlaced formats are out of scope;
 *   - the field order is declared (tff), not detected;
 *   - at rate 2 outputs arrive one frame late (field 2n - 1 waits for frame n);
 *   - the deinterlaced stream can be pushed into a fldr_rate by the caller; no fused path exists;
 *   - the stream is synchronous, as fldr_rate is.
 *
 * Every function returns 0, a negative FLDR_FIELD_E_* code, a negative FLDR_RATE_E_*, FLDR_VIDEO_E_* or FLDR_MODEL_E_* code passed
 * through unchanged, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_FIELD_H
#define FLDR_FIELD_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_FIELD_VERSION 100           /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -1000 and below, apart from the ranges of the libraries below it */
#define FLDR_FIELD_E_ARG        (-1000)  /* null pointer, W out of range, parity / mode / tff / rate / scene out of range, still / slack out of range, non-zero reserved word, null model */
#define FLDR_FIELD_E_SIZE       (-1001)  /* H below 4 or not a multiple of 4 */
#define FLDR_FIELD_E_WORKSPACE  (-1002)  /* workspace null, not 256-byte aligned or smaller than fldr_field_workspace_bytes */
#define FLDR_FIELD_E_DEVICE     (-1003)  /* stream: no such device, or an allocation failed */

#define FLDR_FIELD_API __attribute__((visibility("default")))

enum { FLDR_FIELD_MOTION = 0,            /* the rule above with prev, next and temporal */
       FLDR_FIELD_INTRA = 1 };           /* the line average of the field's own rows */

#define FLDR_FIELD_STILL_DEFAULT8  2     /* in 8-bit codes, << (depth - 8); set on synthetic content only */
#define FLDR_FIELD_SLACK_DEFAULT8  16    /* in 8-bit codes, << (depth - 8); set on synthetic content only */

typedef struct fldr_field_params {       /* in the format's own code units: mx = 255 at depth 8, 1023 at depth 10 */
    int32_t still;                       /* -1 .. mx; -1: the static rule is off */
    int32_t slack;                       /* 0 .. mx */
    int32_t reserved[2];                 /* zero */
} fldr_field_params;

/* One forward: all plane pointers are device pointers. */
typedef struct fldr_field_io {
    int32_t                  H, W;       /* frame size (luma): H a multiple of 4, W >= 2 */
    fldr_video_format        format;     /* of every frame here */
    fldr_video_frame         cur;        /* the frame holding field m */
    fldr_video_frame         prev;       /* the frame holding field m - 1 */
    fldr_video_frame         next;       /* the frame holding field m + 1 */
    int32_t                  parity;     /* 0 / 1: the rows of `cur` that are field m */
    int32_t                  scene;      /* 0: always MOTION; 1: measure the pair (m - 1, m + 1), INTRA on a cut */
    fldr_scene_params        scene_params;   /* 0, 0 = the defaults */
    const fldr_field_params* params;     /* NULL = the defaults */
    fldr_video_frame         out;        /* H x W, progressive */
    int32_t                  reserved[4];    /* zero */
} fldr_field_io;

typedef struct fldr_field_config {
    int32_t                  H, W;
    fldr_video_format        format;     /* of the host frames pushed and returned */
    int32_t                  tff;        /* 1: top field first (field 2k is the even rows), 0: bottom field first */
    int32_t                  rate;       /* 1: one output per frame (the even fields); 2: one per field */
    int32_t                  device;     /* HIP device ordinal: the model's */
    int32_t                  scene;      /* as fldr_field_io.scene */
    fldr_scene_params        scene_params;
    const fldr_field_params* params;     /* NULL = the defaults; copied at create */
    int32_t                  reserved[4];    /* zero */
} fldr_field_config;

typedef struct fldr_field_schedule {     /* what fldr_field_plan says of output j */
    int64_t field;                       /* m */
    int64_t cur;                         /* m >> 1: the frame holding field m */
    int64_t prev;                        /* (m - 1) >> 1: the frame holding field m - 1; -1 for m = 0 */
    int64_t next;                        /* (m + 1) >> 1: the frame holding field m + 1 */
    int32_t parity;                      /* par(m) */
    int32_t reserved;                    /* zero */
} fldr_field_schedule;

typedef struct fldr_field_report {       /* of one output */
    int64_t           field;             /* m */
    uint32_t          parity;            /* par(m) */
    uint32_t          mode_used;         /* FLDR_FIELD_MOTION / FLDR_FIELD_INTRA: INTRA for the first and the last field and on a cut */
    uint32_t          cut;               /* 0 / 1: the pair (m - 1, m + 1) was a cut (always 0 with scene = 0) */
    uint32_t          reserved;          /* zero */
    fldr_scene_result scene;             /* of that pair; all zero without a measure */
} fldr_field_report;

typedef struct fldr_field fldr_field;

FLDR_FIELD_API int         fldr_field_version(void);
FLDR_FIELD_API const char* fldr_field_error_string(int code);
/* 0: sizeof(fldr_field_params), 1: fldr_field_io, 2: fldr_field_config, 3: fldr_field_schedule, 4: fldr_field_report — binding
 * self-check; FLDR_FIELD_E_ARG otherwise */
FLDR_FIELD_API int         fldr_field_sizeof(int which);

/* Enqueue the weave of one frame (device planes in *fmt; H a multiple of 4, W >= 1).  cur: the frame holding the field; prev, next:
 * the frames holding the fields before and after it, of which the rows y % 2 != parity are read; temporal: an H / 2 x W frame in
 * *fmt, the estimate of the missing field (row r of it stands for row 2r + 1 - parity).  mode = FLDR_FIELD_INTRA: prev, next and
 * temporal are ignored and may be NULL.  intra_if (may be NULL): a device word read when the kernel runs; non-zero forces INTRA, so
 * a graph replay follows a rewritten word (prev, next and temporal must then be valid all the same).  p: NULL = the defaults.
 * Checked in this order: null fmt / cur / out, H (FLDR_FIELD_E_SIZE), W, parity, mode (FLDR_FIELD_E_ARG), the format
 * (FLDR_VIDEO_E_FORMAT), p (FLDR_FIELD_E_ARG), then the planes and pitches of cur, out and, in MOTION, prev, next, temporal
 * (FLDR_VIDEO_E_PLANE, FLDR_VIDEO_E_PITCH); last, the frame's size against the kernel's
 * 32-bit index arithmetic: with g = ceil(row bytes / 16) of a plane and R its rows, g * g * R / 2 must stay below 2^32 and the sum of
 * g * R / 2 over the planes below 2^31 (FLDR_FIELD_E_ARG; fldr_field_forward refuses the same frames).  At depth 8 that allows
 * 15360 x 8640 and refuses 16384 x 8640; at depth 10 it allows 8192 x 4320 and refuses 15360 x 8640. */
FLDR_FIELD_API int fldr_field_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* cur, const fldr_video_frame* prev,
                                    const fldr_video_frame* next, const fldr_video_frame* temporal, int parity, int mode,
                                    const uint32_t* intra_if, const fldr_field_params* p, const fldr_video_frame* out, void* stream);

/* fldr_video_workspace_bytes(model, H / 2, W, 1) rounded up to 256, the scene state, the t word and the temporal frame (sized for
 * depth 10, whatever the format).  Negative on bad arguments: FLDR_FIELD_E_SIZE, FLDR_FIELD_E_ARG (null model), or the video / model
 * code for a field the model does not take. */
FLDR_FIELD_API int64_t fldr_field_workspace_bytes(const fldr_model* model, int H, int W);
/* Where in `ws` the H / 2 x W temporal frame of a forward in *fmt lives: its planes are 256-byte aligned, its pitches the row bytes
 * rounded up to 256.  After a forward it holds fldr_video_forward's output at t = 0.5 of the field pair. */
FLDR_FIELD_API int fldr_field_temporal(const fldr_model* model, int H, int W, const fldr_video_format* fmt, void* ws, fldr_video_frame* frame);
/* Where in `ws` the scene state of a forward lives (FLDR_SCENE_STATE_BYTES; begins with the pair's fldr_scene_result when
 * io->scene = 1); NULL on bad arguments. */
FLDR_FIELD_API void* fldr_field_scene_state(const fldr_model* model, int H, int W, void* ws);
/* Enqueue on `stream`, after all validation, and nothing else: with io->scene = 1 fldr_scene_measure of the views of prev and next at
 * parity 1 - parity (H / 2 x W) into the scene state; 0.5f into the t word (a 4-byte memset node); fldr_video_forward of those two
 * views, n_t = 1, into the temporal frame; the weave in MOTION mode, its intra_if the scene state's `cut` word (NULL with scene = 0).
 * Checked in this order: null io, H (FLDR_FIELD_E_SIZE), W < 2, parity, scene, reserved words (FLDR_FIELD_E_ARG), the format
 * (FLDR_VIDEO_E_FORMAT), params (FLDR_FIELD_E_ARG), scene_params (FLDR_RATE_E_ARG), the frames cur, prev, next, out
 * (FLDR_VIDEO_E_PLANE / _PITCH), a null model (FLDR_FIELD_E_ARG), the field size (the model's code), the workspace
 * (FLDR_FIELD_E_WORKSPACE).  ws: device memory of at least fldr_field_workspace_bytes, 256-byte aligned, not used by another forward
 * in flight. */
FLDR_FIELD_API int fldr_field_forward(const fldr_model* model, const fldr_field_io* io, void* ws, int64_t ws_bytes, void* stream);

/* Which field output j >= 0 of a stream carries (only cfg->tff and cfg->rate are read; FLDR_FIELD_E_ARG when they are out of range,
 * on a null pointer or for j outside 0 .. 2^61). */
FLDR_FIELD_API int  fldr_field_plan(const fldr_field_config* cfg, int64_t j, fldr_field_schedule* plan);

/* ---- the stream: woven host frames in, progressive host frames out ---------------------------------------------------------------
 * The stream owns its device memory, pinned staging and stream, keeps the last two uploaded frames on the device (a frame is uploaded
 * once) and synchronises in every push.  After a failed enqueue or wait the object is as after a reset; argument errors change
 * nothing.  One thread drives a stream.  Checked at create, before any device call: null cfg / out, H (FLDR_FIELD_E_SIZE), W < 2,
 * tff, rate, device, scene, reserved words (FLDR_FIELD_E_ARG), the format, params, scene_params (as the forward), a null model. */
FLDR_FIELD_API int  fldr_field_create(const fldr_model* model, const fldr_field_config* cfg, fldr_field** out);
/* cfg->rate: the most frames one push or flush can return; negative on a null handle */
FLDR_FIELD_API int  fldr_field_max_out(const fldr_field* f);
/* Upload host_frame (frame n of the stream, n from 0) and write to host_outs[0 .. *n_out - 1], in order, the outputs that became
 * computable (see the schedule).  host_outs: fldr_field_max_out frames; reports (may be NULL): as many fldr_field_report. */
FLDR_FIELD_API int  fldr_field_push(fldr_field* f, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                    fldr_field_report* reports);
/* End of the stream: at rate 2 the last field, in INTRA mode; none at rate 1, before a push or at a second flush. */
FLDR_FIELD_API int  fldr_field_flush(fldr_field* f, const fldr_video_frame* host_outs, int* n_out, fldr_field_report* reports);
/* Forget everything pushed: the next push is frame 0 of a new stream. */
FLDR_FIELD_API int  fldr_field_reset(fldr_field* f);
FLDR_FIELD_API void fldr_field_destroy(fldr_field* f);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_FIELD_H */
