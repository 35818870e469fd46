/*
 * fldr_light.h — linear-light API of libfldr_light.so: the shutter integration of include/fldr_shutter.h done on light instead of on
 * code values, on top of the shutter API, the rate API (include/fldr_rate.h) and the video API (include/fldr_video.h).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_shutter.h, fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * A camera shutter integrates light.  libfldr_shutter.so averages gamma-encoded numbers: a white point that crosses black for half the
 * window comes out as code 128 of 255 where an exposure gives 191.  Here every sample goes through a transfer curve before it is
 * summed and back through it afterwards.
 *
 * Domain.  R'G'B' code values at the frame's depth.  A frame in fldr_video_format becomes planar BGR codes by the video library's rule
 * (the input conversion of fldr_video_forward; tests/yuv_hd_oracle.yuv420_to_bgr) and the result goes back by its output conversion
 * (bgr_to_yuv420).  With the curve's table lin[0 .. max] (max = 2^depth - 1, entries 0 .. S = 2^24 - 1, strictly increasing),
 * mid[c] = lin[c - 1] + lin[c], integer weights w[k] and total = sum of w[k]:
 *     acc  = sum over k of w[k] * lin[code of frame k]             (uint32; weights 1 .. 255, total <= 255, so acc <= 255 S < 2^32)
 *     q    = (2 acc + total) / (2 total)                            (unsigned division: round half up)
 *     code = the number of c in 1 .. max with mid[c] <= 2 q         (the nearest table entry; a tie goes up)
 * for each of the three channels of every pixel.  All of it is integer arithmetic on the curve's table, so a result does not depend on
 * the launch shape or on the host's libm, and equals the numpy statement of tests/light_oracle.py fed the same table.  One frame alone
 * comes back as its own R'G'B' codes (the table is strictly increasing), but not as its own Y'CbCr bytes: it has been through R'G'B'.
 *
 * Contract:
 *   - fldr_light_curve_create is the only call that allocates or copies.  accumulate, resolve, mix and fldr_light_forward enqueue on
 *     `stream`, only read the curve, and can be captured into a graph.  Arguments are validated before anything is enqueued; formats
 *     and frames by the rules of fldr_video_forward (FLDR_VIDEO_E_FORMAT / E_PITCH / E_PLANE).  `frames` and `weights` are host arrays
 *     read during the call.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_LIGHT_E_* code, a negative FLDR_SHUTTER_E_*, FLDR_RATE_E_*, FLDR_VIDEO_E_* or
 * FLDR_MODEL_E_* code passed through, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_LIGHT_H
#define FLDR_LIGHT_H

#include <stdint.h>

#include "fldr_shutter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_LIGHT_VERSION 100           /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -400 and below, apart from the ranges of the libraries under it */
#define FLDR_LIGHT_E_ARG      (-400)     /* null pointer, bad size or count, unknown transfer or depth, non-zero reserved word */
#define FLDR_LIGHT_E_CURVE    (-401)     /* the curve's depth is not the format's */
#define FLDR_LIGHT_E_TABLE    (-402)     /* a caller's table is not strictly increasing, or its last entry is above 2^24 - 1 */
#define FLDR_LIGHT_E_ACC      (-403)     /* accumulator or scratch null or not 256-byte aligned */
#define FLDR_LIGHT_E_WEIGHT   (-404)     /* a weight outside 1 .. 255 (forward: w0, w1 outside 0 .. 255), or a total outside 1 .. 255 */
#define FLDR_LIGHT_E_RATIO    (-405)     /* what FLDR_SHUTTER_E_RATIO says, with windows of at most 255 grid points */
#define FLDR_LIGHT_E_DEVICE   (-406)     /* no such device, or an allocation failed */
#define FLDR_LIGHT_E_FORMAT   (-407)     /* fldr_light_forward: in_format and out_format differ */

#define FLDR_LIGHT_API __attribute__((visibility("default")))

#define FLDR_LIGHT_MAX_TOTAL 255         /* 255 * (2^24 - 1) < 2^32 */
#define FLDR_LIGHT_SCALE     16777215    /* S: the table entry of light 1 */

enum { FLDR_LIGHT_GAMMA24 = 0,           /* BT.1886 with zero black: L = V^2.4 */
       FLDR_LIGHT_PQ      = 1,           /* SMPTE ST 2084 EOTF, 10000 cd/m^2 = 1 */
       FLDR_LIGHT_HLG     = 2,           /* BT.2100 HLG inverse OETF (scene light): V <= 1/2: V^2 / 3, else (exp((V - c) / a) + b) / 12 */
       FLDR_LIGHT_TABLE   = 3 };         /* the caller's table */

typedef struct fldr_light_curve fldr_light_curve;
typedef struct fldr_light fldr_light;

FLDR_LIGHT_API int         fldr_light_version(void);
FLDR_LIGHT_API const char* fldr_light_error_string(int code);
/* 0: sizeof(fldr_light_config) — binding self-check; FLDR_LIGHT_E_ARG otherwise */
FLDR_LIGHT_API int         fldr_light_sizeof(int which);

/* ---- the curve ------------------------------------------------------------------------------------------------------------------------
 * Host only: the built-in table of `transfer` (GAMMA24, PQ, HLG) at `depth` (8 or 10; 0 means 8) into lin[0 .. 2^depth - 1].  With
 * V = c / max, f the transfer's curve in double precision and S = 2^24 - 1:
 *     lin[0] = 0,   lin[c] = max(round(f(V) * S), lin[c - 1] + 1)
 * so the table is strictly increasing and one frame through the curve and back is the identity on R'G'B' codes.  Where f is flatter than
 * 1 / S per code the `+ 1` floor carries the table instead of f: a PQ table at depth 10 leans on it for its first few dozen codes (PQ
 * code 1 of 1023 is 4e-10 of 10000 cd/m^2), GAMMA24 at depth 10 for its first handful.  The kernels use whatever table the curve holds,
 * bit for bit; only this function touches libm, and an entry may differ by 1 between hosts. */
FLDR_LIGHT_API int fldr_light_table(int transfer, int depth, uint32_t* lin);
/* A curve on `device`: the built-in table of `transfer`, or (FLDR_LIGHT_TABLE) the caller's `table` of 2^depth words, which must be
 * strictly increasing with table[max] <= S (FLDR_LIGHT_E_TABLE); table is not looked at otherwise.  Uploads lin and mid
 * (mid[c] = lin[c - 1] + lin[c], c = 1 .. max) and synchronises.  Everything below only reads the curve; destroy it after the work that
 * uses it has finished. */
FLDR_LIGHT_API int  fldr_light_curve_create(int transfer, int depth, const uint32_t* table, int device, fldr_light_curve** out);
FLDR_LIGHT_API void fldr_light_curve_destroy(fldr_light_curve* curve);

/* ---- the integration kernels ---------------------------------------------------------------------------------------------------------
 * align256(12 H W): three uint32 planes (B, G, R), H x W each, row-major.  Negative on bad arguments. */
FLDR_LIGHT_API int64_t fldr_light_acc_bytes(int H, int W);
/* Bytes of scratch the three calls below need for H x W frames in *fmt (256-byte aligned device memory, not shared with work in
 * flight on another stream): a planar BGR pair and one planar BGR frame, the staging on either side of the video library's converters,
 * and the accumulator a mix of more than two frames runs through.  Negative on bad arguments. */
FLDR_LIGHT_API int64_t fldr_light_scratch_bytes(int H, int W, const fldr_video_format* fmt);
/* acc = (first ? 0 : acc) + sum over k < n of weights[k] * lin[code of frames[k]].  frames: n >= 1 frames of device planes in *fmt;
 * weights 1 .. 255 each, at most 255 together; the sum over all calls into one accumulator must stay within 255 as well. */
FLDR_LIGHT_API int fldr_light_accumulate(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve, const fldr_video_frame* frames,
                                         const int32_t* weights, int n, int first, void* acc, void* scratch, void* stream);
/* out = the frame of the codes nearest to acc / total; total 1 .. 255, the sum of the weights accumulated. */
FLDR_LIGHT_API int fldr_light_resolve(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve, const void* acc, int total,
                                      const fldr_video_frame* out, void* scratch, void* stream);
/* The bytes of accumulate(first = 1) + resolve(sum of weights), 1 <= n <= FLDR_SHUTTER_LAUNCH_FRAMES, total <= 255.  Up to two frames
 * are summed in registers; more go through the accumulator inside scratch.  `out` may be one of the frames. */
FLDR_LIGHT_API int fldr_light_mix(int H, int W, const fldr_video_format* fmt, const fldr_light_curve* curve, const fldr_video_frame* frames,
                                  const int32_t* weights, int n, const fldr_video_frame* out, void* scratch, void* stream);

/* ---- one pair -------------------------------------------------------------------------------------------------------------------------
 * fldr_video_workspace_bytes(model, H, W, n_t) rounded up to 256, plus fldr_light_acc_bytes, plus the scratch of the largest format.
 * Negative on bad arguments. */
FLDR_LIGHT_API int64_t fldr_light_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* The contract of fldr_shutter_forward — one output frame io->out[0], io->in_format == io->out_format (FLDR_LIGHT_E_FORMAT),
 * 1 <= io->n_t <= FLDR_SHUTTER_MAX_SUB, t read on the device — with the integration in linear light: fldr_video_forward of the pair,
 * then one mix of in[0] (weight w0, 0 = left out), in[1] (w1) and the n_t sub-frames (w[k], 1 .. 255), w0 + w1 + sum of w <= 255.
 * The points are read where fldr_video_forward leaves them as planar BGR in its workspace (fldr_video.h documents the offsets): the
 * converted input pair and the model's n_t planar outputs.  A SUB-FRAME'S CODES ARE THE MODEL'S PLANAR OUTPUT: they are never rounded
 * to Y'CbCr and back.  ws: device memory of at least fldr_light_workspace_bytes, 256-byte aligned, not used by another forward in
 * flight. */
FLDR_LIGHT_API int fldr_light_forward(const fldr_model* model, const fldr_video_io* io, const fldr_light_curve* curve, int w0, int w1,
                                      const int32_t* w, void* ws, int64_t ws_bytes, void* stream);

/* ---- the converter ----------------------------------------------------------------------------------------------------------------------
 * The shutter converter of fldr_shutter.h — the same windows, cut rule, pushes and fldr_shutter_info, planned by the same code — with
 * every output the linear-light mean of its points.  The points of a window are frames in cfg.shutter.format: the input frames and the
 * output frames of fldr_video_forward (windows span pushes, so here a sub-frame does pass through the format).  Two rules are new:
 *   - a window of more than 255 grid points is refused at create (FLDR_LIGHT_E_RATIO);
 *   - a window that keeps exactly one point, and that point takes the samples of an input frame, returns that frame's bytes unchanged:
 *     it does not pass through R'G'B'. */
typedef struct fldr_light_config {
    fldr_shutter_config     shutter;     /* everything fldr_shutter_create takes */
    const fldr_light_curve* curve;       /* on shutter.device, of shutter.format's depth; must outlive the converter */
} fldr_light_config;

FLDR_LIGHT_API int  fldr_light_create(const fldr_model* model, const fldr_light_config* cfg, fldr_light** out);
FLDR_LIGHT_API int  fldr_light_max_out(const fldr_light* s);
FLDR_LIGHT_API int  fldr_light_push(fldr_light* s, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs,
                                    fldr_shutter_info* info, int* n_out, fldr_scene_result* scene);
FLDR_LIGHT_API int  fldr_light_flush(fldr_light* s, const fldr_video_frame* host_outs, fldr_shutter_info* info, int* n_out);
FLDR_LIGHT_API int  fldr_light_reset(fldr_light* s);
FLDR_LIGHT_API void fldr_light_destroy(fldr_light* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_LIGHT_H */
