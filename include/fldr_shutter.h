/*
 * fldr_shutter.h — shutter API of libfldr_shutter.so: frame-rate conversion that integrates over a shutter interval (motion blur), on
 * top of the rate API (include/fldr_rate.h) and the video API (include/fldr_video.h).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Three layers ("Shutter API"):
 *   - fldr_shutter_accumulate / resolve / mix: the weighted integer average of frames, in the frames' own format and sample domain;
 *   - fldr_shutter_forward: fldr_video_forward of one pair into scratch frames + one mix of the inputs and the sub-frames;
 *   - fldr_shutter_* sessions: a stream of host frames at in_num / in_den per second in, frames at out_num / out_den out, each the
 *     box-shutter average of the grid points inside its exposure window.
 *
 * Samples.  The formats are fldr_video_format's (NV12 / I420, depth 8 / 10); every plane is treated alike, Y', Cb and Cr code values.
 * The value of a sample is the byte at depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le; it is written back as the byte,
 * v << 6 (low six bits zero), or v.  With integer weights w[k] and total = sum of w[k]:
 *     acc   = sum over k of w[k] * value(frame k)                                  (uint32, exact)
 *     value = min((2 acc + total) / (2 total), 255 or 1023)                        (unsigned division: round half up)
 * All of it is integer arithmetic, so a result does not depend on the launch shape and equals the numpy statement of
 * tests/shutter_oracle.py.
 *
 * Contract:
 *   - accumulate, resolve, mix and fldr_shutter_forward enqueue on `stream`.  No allocation, no synchronisation, no host<->device
 *     copy: they can be captured into a graph.  Arguments are validated before anything is enqueued; formats and frames by the rules
 *     of fldr_video_forward (FLDR_VIDEO_E_FORMAT / E_PITCH / E_PLANE).  `frames` and `weights` are host arrays read during the call.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_SHUTTER_E_* code, a negative FLDR_RATE_E_*, FLDR_VIDEO_E_* or FLDR_MODEL_E_* code passed
 * through, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_SHUTTER_H
#define FLDR_SHUTTER_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_SHUTTER_VERSION 100         /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -300 and below, apart from FLDR_RATE_E_* (-200 ..), FLDR_VIDEO_E_* (-100 ..) and FLDR_MODEL_E_* (-1 ..) */
#define FLDR_SHUTTER_E_ARG      (-300)   /* null pointer, bad size or count, scene not 0 / 1, sub outside 1 .. 64, non-zero reserved word */
#define FLDR_SHUTTER_E_FORMAT   (-301)   /* fldr_shutter_forward: in_format and out_format differ */
#define FLDR_SHUTTER_E_ACC      (-302)   /* accumulator null or not 256-byte aligned */
#define FLDR_SHUTTER_E_WEIGHT   (-303)   /* a weight outside 1 .. 255 (forward: w0, w1 outside 0 .. 255), or a total outside 1 .. 65535 */
#define FLDR_SHUTTER_E_RATIO    (-304)   /* a rate or shutter term not positive, s > 1, a reduced term above 2^24, a window that could hold
                                            no grid point or more than 65535, or more than FLDR_SHUTTER_MAX_OUT outputs per push */
#define FLDR_SHUTTER_E_DEVICE   (-305)   /* session: no such device, or an allocation failed */

#define FLDR_SHUTTER_API __attribute__((visibility("default")))

#define FLDR_SHUTTER_MAX_OUT       64    /* most output frames one pushed frame may produce */
#define FLDR_SHUTTER_MAX_SUB       64    /* most grid points per input interval */
#define FLDR_SHUTTER_LAUNCH_FRAMES 66    /* frames one kernel launch takes: an accumulate of more runs several launches, a mix of more is
                                            refused (FLDR_SHUTTER_E_ARG); 66 = both inputs and the 64 sub-frames a forward can have */
#define FLDR_SHUTTER_MAX_TOTAL     65535 /* 2 * 1023 * 65535 + 65535 < 2^32 */

FLDR_SHUTTER_API int         fldr_shutter_version(void);
FLDR_SHUTTER_API const char* fldr_shutter_error_string(int code);
/* 0: sizeof(fldr_shutter_config), 1: fldr_shutter_info — binding self-check; FLDR_SHUTTER_E_ARG otherwise */
FLDR_SHUTTER_API int         fldr_shutter_sizeof(int which);

/* ---- the integration kernels ---------------------------------------------------------------------------------------------------------
 * Bytes of an accumulator for H x W frames in *fmt: one uint32 per sample of the packed frame, rounded up to 256.  The layout inside
 * is the library's own; the caller sizes it and aligns it to 256 bytes.  Negative on bad arguments. */
FLDR_SHUTTER_API int64_t fldr_shutter_acc_bytes(int H, int W, const fldr_video_format* fmt);
/* acc = (first ? 0 : acc) + sum over k < n of weights[k] * value(frames[k]), for every sample.  frames: n >= 1 frames of device planes
 * in *fmt; weights: 1 .. 255 each.  One launch reads up to FLDR_SHUTTER_LAUNCH_FRAMES frames and reads and writes acc once for all of
 * them.  The sum over all calls into one accumulator must stay within 1023 * 65535 per sample (weights totalling at most 65535). */
FLDR_SHUTTER_API int fldr_shutter_accumulate(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* frames, const int32_t* weights,
                                             int n, int first, void* acc, void* stream);
/* out = the rounded, clamped quotient acc / total of every sample, written in *fmt; total 1 .. 65535, the sum of the weights
 * accumulated (acc <= 1023 * total is what the arithmetic is exact for). */
FLDR_SHUTTER_API int fldr_shutter_resolve(int H, int W, const fldr_video_format* fmt, const void* acc, int total, const fldr_video_frame* out,
                                          void* stream);
/* The fused form, 1 <= n <= FLDR_SHUTTER_LAUNCH_FRAMES: the bytes of accumulate(first = 1) + resolve(sum of weights), with the sums
 * kept in registers.  `out` may be one of the frames. */
FLDR_SHUTTER_API int fldr_shutter_mix(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* frames, const int32_t* weights, int n,
                                      const fldr_video_frame* out, void* stream);
/* What resolve divides with: for x <= 2047 * total, ((uint64_t)x * *mul >> 32) >> *shift == x / (2 * total).  Host only. */
FLDR_SHUTTER_API int fldr_shutter_reciprocal(int total, uint32_t* mul, uint32_t* shift);

/* ---- one pair -------------------------------------------------------------------------------------------------------------------------
 * fldr_video_workspace_bytes(model, H, W, n_t) rounded up to 256, plus n_t packed frames (8-bit sized or 10-bit sized whatever the
 * format: 2 bytes per sample) each rounded up to 256.  Negative on bad arguments. */
FLDR_SHUTTER_API int64_t fldr_shutter_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue on `stream`: fldr_video_forward(model, io', ..) with io' = *io but its n_t outputs in scratch frames inside ws, then one
 * fldr_shutter_mix of io->in[0] (weight w0), io->in[1] (weight w1) — a weight of 0 leaves that frame out — and the n_t sub-frames
 * (weights w[k], 1 .. 255) into io->out[0], the ONE output frame.  1 <= io->n_t <= FLDR_SHUTTER_MAX_SUB.  io->in_format must equal
 * io->out_format (FLDR_SHUTTER_E_FORMAT).  t is read on the device: a graph replay follows rewritten times.  A device fault flag of an
 * earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); the output is then not written.  ws: device memory of at
 * least fldr_shutter_workspace_bytes, 256-byte aligned, not used by another forward in flight. */
FLDR_SHUTTER_API int fldr_shutter_forward(const fldr_model* model, const fldr_video_io* io, int w0, int w1, const int32_t* w, void* ws,
                                          int64_t ws_bytes, void* stream);

/* ---- the converter: host frames at in_num / in_den per second in, box-shutter frames at out_num / out_den out ------------------------
 * With A / B = (in_num * out_den) / (in_den * out_num) reduced and s = shutter_num / shutter_den (0 < s <= 1, the exposure as a
 * fraction of the OUTPUT interval; 180 degrees is 1 / 2):
 *   grid    point m sits at input position m / sub; i = m div sub, k = m mod sub.  k == 0: the samples of input frame i; k > 0: the
 *           output of fldr_video_forward on (i, i + 1) at t = (float)k / (float)sub.
 *   window  output j is exposed over [j A / B, j A / B + s A / B): m belongs to j iff
 *           j A sub sd <= m B sd < j A sub sd + sn A sub   (sn / sd = s).  Windows are disjoint.  Output j is the equal-weight
 *           average of its points, resolved by their count.
 *   cuts    (scene = 1) every pair is measured with fldr_scene_measure and the flag is read on the host before the pair is planned.
 *           On a cut pair no forward runs: a point with k > 0 takes the samples of frame i when 2 k < sub, else of frame i + 1.  A
 *           point's scene is the number of cuts at or before it, a cut pair's points with 2 k >= sub counting as after the cut; a
 *           window keeps only the points in the scene of its first point.
 *   pushes  the push of frame n supplies the points (n - 1) sub < m <= n sub (m = 0 on the first).  Output j is returned by the push
 *           that supplies its last kept point — the push whose measure shows the cut, for a window a cut truncates.  flush returns
 *           the output whose window has begun but not ended, averaged over the points that exist.  Over a stream of N frames the
 *           outputs are exactly the j with j A / B <= N - 1, the count fldr_rate returns. */
typedef struct fldr_shutter_config {
    int32_t           H, W;
    fldr_video_format format;            /* of the host frames pushed and returned */
    int32_t           in_num, in_den;    /* input frames per second, a rational; all four terms > 0 */
    int32_t           out_num, out_den;
    int32_t           shutter_num, shutter_den;   /* s: 0 < s <= 1 */
    int32_t           sub;               /* grid points per input interval: 1 .. FLDR_SHUTTER_MAX_SUB */
    int32_t           device;            /* HIP device ordinal: the model's */
    int32_t           scene;             /* 0: interpolate every pair; 1: measure every pair, never mix two scenes */
    fldr_scene_params scene_params;      /* 0, 0 = the defaults */
    int32_t           reserved[4];       /* zero */
} fldr_shutter_config;

typedef struct fldr_shutter_info {       /* one per output frame of a push or flush */
    int64_t j;                           /* the output's index */
    int32_t points;                      /* grid points averaged */
    int32_t interpolated;                /* of them, outputs of fldr_video_forward */
    int32_t truncated;                   /* 1: a cut ended the window early (push) or the stream did (flush) */
    int32_t reserved;                    /* written as zero */
} fldr_shutter_info;

typedef struct fldr_shutter fldr_shutter;

/* Host only, no device call: the first and last grid point of output j's window (j >= 0) under cfg's rates, shutter and sub; H, W,
 * format, device, scene are not looked at.  FLDR_SHUTTER_E_RATIO as create refuses. */
FLDR_SHUTTER_API int  fldr_shutter_plan(const fldr_shutter_config* cfg, int64_t j, int64_t* first, int64_t* last);

FLDR_SHUTTER_API int  fldr_shutter_create(const fldr_model* model, const fldr_shutter_config* cfg, fldr_shutter** out);
/* ceil(B / A) + 1: the most frames one push can return; negative on a null handle */
FLDR_SHUTTER_API int  fldr_shutter_max_out(const fldr_shutter* s);
/* Upload host_frame (frame n of the stream) and write to host_outs[0 .. *n_out - 1] / info[0 .. *n_out - 1], in order, every output
 * whose last kept point this push supplies.  host_outs, info: fldr_shutter_max_out entries (may be NULL when no output is due; info
 * may always be NULL).  At most one fldr_video_forward runs, with exactly the sub-times some window keeps.  scene (may be NULL): with
 * cfg.scene = 1 the fldr_scene_result of the pair (n - 1, n); zero otherwise.  Synchronises before it returns. */
FLDR_SHUTTER_API int  fldr_shutter_push(fldr_shutter* s, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs,
                                        fldr_shutter_info* info, int* n_out, fldr_scene_result* scene);
/* End of the stream: the output whose window is open, if any.  A second flush returns none. */
FLDR_SHUTTER_API int  fldr_shutter_flush(fldr_shutter* s, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out);
/* Forget everything pushed: the next push is frame 0 of a new stream. */
FLDR_SHUTTER_API int  fldr_shutter_reset(fldr_shutter* s);
FLDR_SHUTTER_API void fldr_shutter_destroy(fldr_shutter* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_SHUTTER_H */
