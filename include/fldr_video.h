/*
 * fldr_video.h — video API of libfldr_video.so: frame interpolation on 8-bit and 10-bit YUV 4:2:0 frames (NV12 / P010, I420 /
 * yuv420p10le), the formats decoders hand out and encoders take back, on top of the C model API (include/fldr_model.h).
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_model.h.
 *
 * Colour ("Video API"): integer fixed point, BT.601 or BT.709, limited or full range, chroma sited "left" (chroma
 * sample (i, j) at luma (2i, 2j + 1/2), the MPEG-2 / H.264 / HEVC default).  The input frames are converted to the 8-bit BGR frames a
 * caller would get by converting on the host, so a forward on a YUV pair is, bit for bit, the model's forward on those BGR frames.
 * Odd widths and heights are allowed; the chroma planes are ceil(W/2) x ceil(H/2).
 * Depth 10 (fldr_video_format.depth): samples are little-endian 16-bit words, pitches stay in BYTES.  FLDR_VIDEO_NV12 is then P010 (the
 * value in the high 10 bits, word = v << 6; the low 6 bits are ignored on input and written as zero), FLDR_VIDEO_I420 is yuv420p10le (the
 * value in the low 10 bits; input words are masked with 0x3ff).  The same matrices, siting and fixed point with limited range Y 64 .. 940,
 * C 64 .. 960; the model then runs on 10-bit BGR code values (FLDR_MODEL_IN_U10_PLANAR / OUT_U10_PLANAR), so the two extra bits go
 * through the network.  in_format and out_format may differ in depth.  No transfer function is applied: PQ / HLG frames pass through as
 * code values like any other.
 *
 * Contract:
 *   - fldr_video_forward enqueues on `stream`: the input conversion, one fldr_model_forward (8-bit planar in and out, n_t outputs
 *     sharing the pair's work) and n_t output conversions.  No allocation, no synchronisation, no host<->device copy: it can be
 *     captured into a graph.  Arguments are validated before anything is enqueued.  A device fault flag of an earlier call is
 *     reported as the model reports it (FLDR_MODEL_E_STATUS); no output frame is then written.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API (fldr_video_session_*) owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_VIDEO_E_* code, a negative FLDR_MODEL_E_* code passed through from the model, or a
 * positive hipError_t from the runtime.
 */
#ifndef FLDR_VIDEO_H
#define FLDR_VIDEO_H

#include <stdint.h>

#include "fldr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_VIDEO_VERSION 101           /* major*10000 + minor*100 + patch of this header; 101: fldr_video_format.depth (10-bit frames) */

/* codes of this library: -100 and below, apart from the FLDR_MODEL_E_* range (-1 .. -99) */
#define FLDR_VIDEO_E_ARG        (-100)   /* null pointer, bad size, n_t < 1, null model */
#define FLDR_VIDEO_E_FORMAT     (-101)   /* unknown layout / matrix / range / depth, or a non-zero reserved word */
#define FLDR_VIDEO_E_PITCH      (-102)   /* a plane pitch shorter than its row; depth 10: or an odd pitch */
#define FLDR_VIDEO_E_PLANE      (-103)   /* a null plane pointer; depth 10: or an odd plane address */
#define FLDR_VIDEO_E_WORKSPACE  (-104)   /* workspace null, not 256-byte aligned or smaller than fldr_video_workspace_bytes */
#define FLDR_VIDEO_E_DEVICE     (-105)   /* session: no such device, or an allocation failed */

#define FLDR_VIDEO_API __attribute__((visibility("default")))

enum { FLDR_VIDEO_NV12 = 0,              /* plane[0] = Y (W bytes per row), plane[1] = interleaved U, V (2 ceil(W/2) bytes per row) */
       FLDR_VIDEO_I420 = 1 };            /* plane[0] = Y, plane[1] = U, plane[2] = V (ceil(W/2) bytes per chroma row) */
enum { FLDR_VIDEO_BT601 = 0, FLDR_VIDEO_BT709 = 1 };
enum { FLDR_VIDEO_LIMITED = 0,           /* Y 16 .. 235, C 16 .. 240 */
       FLDR_VIDEO_FULL = 1 };            /* Y, C 0 .. 255 */

typedef struct fldr_video_format {
    int32_t layout;                      /* FLDR_VIDEO_NV12 / FLDR_VIDEO_I420 */
    int32_t matrix;                      /* FLDR_VIDEO_BT601 / FLDR_VIDEO_BT709 */
    int32_t range;                       /* FLDR_VIDEO_LIMITED / FLDR_VIDEO_FULL */
    int32_t depth;                       /* 0 or 8: 8-bit samples; 10: 10-bit samples in 16-bit words (NV12 = P010, I420 = yuv420p10le) */
    int32_t reserved[4];                 /* zero */
} fldr_video_format;

/* One frame: plane pointers (plane[2] unused for NV12) and their pitches in bytes (row r of plane p at plane[p] + r * pitch[p]). */
typedef struct fldr_video_frame {
    void*   plane[3];
    int64_t pitch[3];
} fldr_video_frame;

/* One forward: all plane pointers and `t` are device pointers; `out` is a host array of n_t frames, read during the call. */
typedef struct fldr_video_io {
    int32_t                 H, W;        /* frame size (luma) */
    fldr_video_format       in_format;
    fldr_video_frame        in[2];       /* I0, I1 */
    fldr_video_format       out_format;
    int32_t                 n_t;         /* outputs: >= 1 */
    const float*            t;           /* n_t floats on the device (output k at t[k]); may be rewritten between graph replays */
    const fldr_video_frame* out;         /* n_t frames in out_format */
} fldr_video_io;

typedef struct fldr_video_session_config {
    int32_t           H, W;
    fldr_video_format in_format;         /* of the host frames pushed */
    fldr_video_format out_format;        /* of the host frames returned */
    int32_t           n_t;               /* interpolated frames per pushed frame: >= 1 */
    int32_t           device;            /* HIP device ordinal: the model's */
    const float*      t;                 /* host array of n_t times, copied at create; NULL: t[k] = (k + 1) / (n_t + 1) */
    int32_t           reserved[4];       /* zero */
} fldr_video_session_config;

typedef struct fldr_video_session fldr_video_session;

FLDR_VIDEO_API int         fldr_video_version(void);
FLDR_VIDEO_API const char* fldr_video_error_string(int code);
/* 0: sizeof(fldr_video_format), 1: fldr_video_frame, 2: fldr_video_io, 3: fldr_video_session_config — binding self-check;
 * FLDR_VIDEO_E_ARG otherwise */
FLDR_VIDEO_API int         fldr_video_sizeof(int which);

/* Bytes of workspace one forward of an H x W pair with n_t outputs needs, whatever the formats: fldr_model_workspace_bytes, then the
 * planar BGR pair ([1,2,3,H,W]: uint8 as FLDR_MODEL_IN_U8_PLANAR takes it, or uint16 for a 10-bit input), then n_t planar BGR outputs
 * ([1,3,H,W] each: uint8, or uint16 for a 10-bit output), each part starting 256-byte aligned.  After a forward these planar frames stay
 * there.  With 8-bit formats the pair is at align(model bytes) and output k at pair + align(6 H W) + k align(3 H W), as before the 10-bit
 * formats existed; a 10-bit input puts the outputs behind align(12 H W), a 10-bit output spaces them align(6 H W) apart.  The size is that
 * of the 16-bit regions, so it grew by 6 H W + 3 H W n_t bytes plus alignment over version 100: at 3840 x 2160 the part behind the model's
 * 2,304.7 MB went from 49.8 + 24.9 n_t MB to 99.5 + 49.8 n_t MB.  Negative on bad arguments. */
FLDR_VIDEO_API int64_t fldr_video_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue one forward on `stream` (NULL = the null stream).  ws: device memory of at least fldr_video_workspace_bytes, 256-byte
 * aligned, not used by another forward in flight. */
FLDR_VIDEO_API int fldr_video_forward(const fldr_model* model, const fldr_video_io* io, void* ws, int64_t ws_bytes, void* stream);

/* ---- sessions: a stream of host frames; each frame is uploaded once and is the second frame of one pair and the first of the next */
FLDR_VIDEO_API int  fldr_video_session_create(const fldr_model* model, const fldr_video_session_config* cfg, fldr_video_session** out);
/* Upload `frame` (host planes in cfg->in_format); if a previous frame is held, interpolate n_t frames between it and this one into
 * host_outs[0 .. n_t-1] (host planes in cfg->out_format).  Synchronises before it returns.  *n_out: 0 on the first push and the first
 * after a reset, n_t otherwise (host_outs may be NULL when no output is due). */
FLDR_VIDEO_API int  fldr_video_session_push(fldr_video_session* s, const fldr_video_frame* frame, const fldr_video_frame* host_outs, int* n_out);
/* Forget the previous frame (a scene cut): the next push returns no output. */
FLDR_VIDEO_API int  fldr_video_session_reset(fldr_video_session* s);
FLDR_VIDEO_API void fldr_video_session_destroy(fldr_video_session* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_VIDEO_H */
