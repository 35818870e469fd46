/*
 * fldr_rate.h — rate API of libfldr_rate.so: frame-rate conversion between constant rational rates with scene-cut detection on the
 * device, on top of the video API (include/fldr_video.h).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_video.h and fldr_model.h.
 *
 * Three layers ("Rate API"):
 *   - fldr_scene_measure: the cut measure of one frame pair, in integers, read from the luma planes alone;
 *   - fldr_rate_forward: fldr_scene_measure + fldr_video_forward + one select launch that, on a cut, replaces every output by a copy
 *     of the nearer input frame;
 *   - fldr_rate_* sessions: a stream of host frames at in_num / in_den frames per second in, frames at out_num / out_den out.
 *
 * The cut measure.  y8(sample) is the luma sample reduced to 8 bits: the byte at depth 8, word >> 8 for P010, (word & 0x3ff) >> 2 for
 * yuv420p10le.  Only plane 0 is read, so the layout decides nothing but the 10-bit word form, and matrix and range do not enter.
 *     sad       = sum over all H x W of |y8(I0) - y8(I1)|
 *     hist_dist = sum over b of |h0[b] - h1[b]|, h0 / h1 the 256-bin histograms of y8 of each frame      (0 .. 2 H W)
 *     cut       = sad * 1000 >= sad_permille * 255 * H * W  &&  hist_dist * 1000 >= hist_permille * 2 * H * W    (64-bit)
 * Everything is an integer sum, so the result does not depend on the order of the reduction: it is the same from run to run and
 * equal to the numpy statement of tests/scene_oracle.py.
 *
 * Contract:
 *   - fldr_scene_measure and fldr_rate_forward enqueue on `stream`.  No allocation, no synchronisation, no host<->device copy: they
 *     can be captured into a graph.  Arguments are validated before anything is enqueued.  `state` needs no preparation: the library
 *     zeroes what it uses, on the stream.  Calls with different `state` / workspace may be in flight on different streams.
 *   - fldr_rate_forward: a device fault flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); the cut
 *     measure of the pair has then been enqueued, no output frame is written.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_RATE_E_* code, a negative FLDR_VIDEO_E_* or FLDR_MODEL_E_* code passed through, or a
 * positive hipError_t from the runtime.
 */
#ifndef FLDR_RATE_H
#define FLDR_RATE_H

#include <stdint.h>

#include "fldr_video.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_RATE_VERSION 100            /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -200 and below, apart from FLDR_VIDEO_E_* (-100 .. -199) and FLDR_MODEL_E_* (-1 .. -99) */
#define FLDR_RATE_E_ARG         (-200)   /* null pointer, bad size, a threshold outside 0 .. 1000, scene not 0 / 1, non-zero reserved word */
#define FLDR_RATE_E_FORMAT      (-201)   /* fldr_rate_forward: in_format and out_format differ */
#define FLDR_RATE_E_STATE       (-202)   /* scene state null or not 256-byte aligned */
#define FLDR_RATE_E_RATIO       (-203)   /* a rate term not positive, more than FLDR_RATE_MAX_OUT outputs per pushed frame, or a reduced term above 2^24 */
#define FLDR_RATE_E_DEVICE      (-204)   /* session: no such device, or an allocation failed */

#define FLDR_RATE_API __attribute__((visibility("default")))

#define FLDR_SCENE_SAD_DEFAULT   80      /* permille of 255 H W */
#define FLDR_SCENE_HIST_DEFAULT  100     /* permille of 2 H W */
#define FLDR_SCENE_STATE_BYTES   4096    /* device memory, 256-byte aligned; begins with a fldr_scene_result, the rest is the kernels' */
#define FLDR_RATE_MAX_OUT        64      /* most output frames one pushed frame may produce */

typedef struct fldr_scene_params {
    int32_t sad_permille;                /* 1 .. 1000; 0: FLDR_SCENE_SAD_DEFAULT */
    int32_t hist_permille;               /* 1 .. 1000; 0: FLDR_SCENE_HIST_DEFAULT */
    int32_t reserved[2];                 /* zero */
} fldr_scene_params;

typedef struct fldr_scene_result {       /* 32 bytes, at the start of the scene state */
    uint64_t sad;
    uint32_t hist_dist;
    uint32_t cut;                        /* 0 / 1 */
    uint32_t reserved[4];                /* written as zero */
} fldr_scene_result;

FLDR_RATE_API int         fldr_rate_version(void);
FLDR_RATE_API const char* fldr_rate_error_string(int code);
/* 0: sizeof(fldr_scene_params), 1: fldr_scene_result, 2: fldr_rate_config — binding self-check; FLDR_RATE_E_ARG otherwise */
FLDR_RATE_API int         fldr_rate_sizeof(int which);

/* Enqueue the cut measure of the pair in[0], in[1] (device planes in *fmt, any H, W >= 1; only plane 0 is read, but every plane
 * of the format is checked as fldr_video_forward checks it).  p: NULL = the defaults.  After the stream reaches this point `state`
 * begins with the pair's fldr_scene_result. */
FLDR_RATE_API int fldr_scene_measure(int H, int W, const fldr_video_format* fmt, const fldr_video_frame in[2],
                                     const fldr_scene_params* p, void* state, void* stream);

/* fldr_video_workspace_bytes(model, H, W, n_t) rounded up to 256, plus FLDR_SCENE_STATE_BYTES.  Negative on bad arguments. */
FLDR_RATE_API int64_t fldr_rate_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue on `stream`: fldr_scene_measure of io->in, fldr_video_forward(model, io, ws, ..) unchanged, then the select: if the pair
 * is a cut, output k becomes a copy of the samples of io->in[t[k] < 0.5f ? 0 : 1], plane by plane, row bytes only (P010: the low six
 * bits of each word are copied as they are); if not, the select returns without touching memory.  t is read on the device, so a
 * graph replay follows rewritten times.  (One select launch serves 64 outputs; a call with more runs one per 64.)
 * io->in_format must equal io->out_format (FLDR_RATE_E_FORMAT).  ws: device memory of at least fldr_rate_workspace_bytes, 256-byte
 * aligned, not used by another forward in flight; the scene state, and so the pair's fldr_scene_result, is at
 * ws + fldr_rate_workspace_bytes(model, H, W, io->n_t) - FLDR_SCENE_STATE_BYTES (by the n_t of the call, whatever ws_bytes is). */
FLDR_RATE_API int fldr_rate_forward(const fldr_model* model, const fldr_video_io* io, const fldr_scene_params* p, void* ws, int64_t ws_bytes,
                                    void* stream);

/* ---- the rate converter: host frames at in_num / in_den per second in, host frames at out_num / out_den out -----------------------
 * With A / B = (in_num * out_den) / (in_den * out_num) reduced, output frame j sits at input position j A / B: i = floor(j A / B),
 * r = j A mod B.  r == 0: the output is input frame i, its bytes.  Otherwise it is the interpolation of frames (i, i + 1) at
 * t = (float)r / (float)B; with scene = 1 and the pair a cut, it is the nearer frame instead (r * 2 < B: frame i, else frame i + 1). */
typedef struct fldr_rate_config {
    int32_t           H, W;
    fldr_video_format format;            /* of the host frames pushed and returned */
    int32_t           in_num, in_den;    /* input frames per second, a rational; all four terms > 0 */
    int32_t           out_num, out_den;
    int32_t           device;            /* HIP device ordinal: the model's */
    int32_t           scene;             /* 0: interpolate every pair; 1: measure every pair, repeat the nearer frame on a cut */
    fldr_scene_params scene_params;      /* 0, 0 = the defaults */
    int32_t           reserved[4];       /* zero */
} fldr_rate_config;

typedef struct fldr_rate fldr_rate;

FLDR_RATE_API int  fldr_rate_create(const fldr_model* model, const fldr_rate_config* cfg, fldr_rate** out);
/* ceil(B / A): the most frames one push can return; negative on a null handle */
FLDR_RATE_API int  fldr_rate_max_out(const fldr_rate* r);
/* Upload host_frame (frame n of the stream, n from 0) and write to host_outs[0 .. *n_out - 1], in order, every output j with
 * n - 1 <= j A / B < n: none on the first push.  host_outs: fldr_rate_max_out frames (may be NULL when no output is due).  A pair with
 * no interpolated output in it runs no forward.  scene (may be NULL): with cfg.scene = 1 the fldr_scene_result of the pair
 * (n - 1, n); all zero on the first push or with cfg.scene = 0.  Synchronises before it returns. */
FLDR_RATE_API int  fldr_rate_push(fldr_rate* r, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                  fldr_scene_result* scene);
/* End of the stream: the one output j, if any, that lands exactly on the last pushed frame (its bytes).  A second flush returns none. */
FLDR_RATE_API int  fldr_rate_flush(fldr_rate* r, const fldr_video_frame* host_outs, int* n_out);
/* Forget everything pushed: the next push is frame 0 of a new stream, output 0 included. */
FLDR_RATE_API int  fldr_rate_reset(fldr_rate* r);
FLDR_RATE_API void fldr_rate_destroy(fldr_rate* r);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_RATE_H */
