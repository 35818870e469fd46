/*
 * fldr_chroma.h — API of libfldr_chroma.so: frame interpolation on YUV 4:2:2 and 4:4:4 frames at 8 and 10 bits (yuv422p, NV16, UYVY,
 * YUYV, yuv444p, NV24 and the 10-bit yuv422p10le, P210, yuv444p10le, P410), the formats of camera originals, SDI capture and mastering,
 * on top of the C model API (include/fldr_model.h).  A sibling of libfldr_video.so (4:2:0), with its own format struct.
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_model.h.
 *
 * Colour: the integer fixed point of fldr_video.h (BT.601 or BT.709, limited or full range, 16 fraction
 * bits, the same tables).  4:2:2 chroma is co-sited with the even luma columns ("left") and has no vertical taps: chroma is interpolated
 * along the row with the 4:2:0 horizontal taps, and decimated along the row with (1, 2, 1).  4:4:4 has no taps at all.  Odd widths and
 * heights are allowed; the chroma planes are H x ceil(W/2) at 4:2:2 and H x W at 4:4:4.
 * Depth 10: samples are little-endian 16-bit words, pitches stay in BYTES.  FLDR_CHROMA_PLANAR keeps the value in the low 10 bits (input
 * words are masked with 0x3ff), FLDR_CHROMA_SEMIPLANAR in the high 10 bits (word = v << 6; the low 6 bits are ignored on input).  Bits
 * that carry no value are written as zero.  The model then runs on 10-bit BGR code values.  No transfer function is applied.
 *
 * Contract (that of fldr_video.h):
 *   - fldr_chroma_to_planar, fldr_chroma_from_planar and fldr_chroma_forward enqueue on `stream`.  No allocation, no synchronisation,
 *     no host<->device copy: they can be captured into a graph.  Arguments are validated before anything is enqueued.  A device fault
 *     flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); no output frame is then written.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API (fldr_chroma_session_*) owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_CHROMA_E_* code, a negative FLDR_MODEL_E_* code passed through from the model, or a
 * positive hipError_t from the runtime.
 *
 * Out of scope: v210, Y210 / Y410, 12-bit samples, alpha planes and interlaced material; and 4:2:2 / 4:4:4 through the libraries built
 * on fldr_video.h, whose frames are described by fldr_video_format (4:2:0 only).
 */
#ifndef FLDR_CHROMA_H
#define FLDR_CHROMA_H

#include <stdint.h>

#include "fldr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_CHROMA_VERSION 100          /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -700 and below; the ranges above belong to the model and the other libraries */
#define FLDR_CHROMA_E_ARG        (-700)  /* null pointer, bad size, n_t < 1, null model */
#define FLDR_CHROMA_E_FORMAT     (-701)  /* unknown sampling / layout / matrix / range / depth, a packed layout at depth 10 or at 4:4:4,
                                            or a non-zero reserved word */
#define FLDR_CHROMA_E_PITCH      (-702)  /* a plane pitch shorter than its row; depth 10: or an odd pitch */
#define FLDR_CHROMA_E_PLANE      (-703)  /* a null plane pointer; depth 10: or an odd plane address */
#define FLDR_CHROMA_E_WORKSPACE  (-704)  /* workspace null, not 256-byte aligned or smaller than fldr_chroma_workspace_bytes */
#define FLDR_CHROMA_E_DEVICE     (-705)  /* session: no such device, or an allocation failed */

#define FLDR_CHROMA_API __attribute__((visibility("default")))

enum { FLDR_CHROMA_422 = 0,              /* chroma planes H x ceil(W/2) */
       FLDR_CHROMA_444 = 1 };            /* chroma planes H x W */
enum { FLDR_CHROMA_PLANAR = 0,           /* plane[0] = Y, plane[1] = U, plane[2] = V: yuv422p / yuv444p; depth 10: yuv422p10le / yuv444p10le */
       FLDR_CHROMA_SEMIPLANAR = 1,       /* plane[0] = Y, plane[1] = interleaved U, V: NV16 / NV24; depth 10: P210 / P410 */
       FLDR_CHROMA_UYVY = 2,             /* plane[0] = U Y0 V Y1 per two pixels, 4 ceil(W/2) bytes per row; 4:2:2 at depth 8 only */
       FLDR_CHROMA_YUYV = 3 };           /* plane[0] = Y0 U Y1 V, otherwise as UYVY.  With odd W the second luma byte of the last group is
                                            ignored on input and written as a copy of the last luma sample. */
enum { FLDR_CHROMA_BT601 = 0, FLDR_CHROMA_BT709 = 1 };
enum { FLDR_CHROMA_LIMITED = 0,          /* Y 16 .. 235, C 16 .. 240 (x 4 at depth 10) */
       FLDR_CHROMA_FULL = 1 };           /* the whole code range */

typedef struct fldr_chroma_format {
    int32_t sampling;                    /* FLDR_CHROMA_422 / FLDR_CHROMA_444 */
    int32_t layout;                      /* FLDR_CHROMA_PLANAR / SEMIPLANAR / UYVY / YUYV */
    int32_t matrix;                      /* FLDR_CHROMA_BT601 / FLDR_CHROMA_BT709 */
    int32_t range;                       /* FLDR_CHROMA_LIMITED / FLDR_CHROMA_FULL */
    int32_t depth;                       /* 0 or 8: 8-bit samples; 10: 10-bit samples in 16-bit words */
    int32_t reserved[3];                 /* zero */
} fldr_chroma_format;

/* One frame: plane pointers (unused ones ignored) and their pitches in bytes (row r of plane p at plane[p] + r * pitch[p]). */
typedef struct fldr_chroma_frame {
    void*   plane[3];
    int64_t pitch[3];
} fldr_chroma_frame;

/* One forward: all plane pointers and `t` are device pointers; `out` is a host array of n_t frames, read during the call. */
typedef struct fldr_chroma_io {
    int32_t                  H, W;       /* frame size (luma) */
    fldr_chroma_format       in_format;
    fldr_chroma_frame        in[2];      /* I0, I1 */
    fldr_chroma_format       out_format; /* may differ from in_format in everything */
    int32_t                  n_t;        /* outputs: >= 1 */
    const float*             t;          /* n_t floats on the device (output k at t[k]); may be rewritten between graph replays */
    const fldr_chroma_frame* out;        /* n_t frames in out_format */
} fldr_chroma_io;

typedef struct fldr_chroma_session_config {
    int32_t            H, W;
    fldr_chroma_format in_format;        /* of the host frames pushed */
    fldr_chroma_format out_format;       /* of the host frames returned */
    int32_t            n_t;              /* interpolated frames per pushed frame: >= 1 */
    int32_t            device;           /* HIP device ordinal: the model's */
    const float*       t;                /* host array of n_t times, copied at create; NULL: t[k] = (k + 1) / (n_t + 1) */
    int32_t            reserved[4];      /* zero */
} fldr_chroma_session_config;

typedef struct fldr_chroma_session fldr_chroma_session;

FLDR_CHROMA_API int         fldr_chroma_version(void);
FLDR_CHROMA_API const char* fldr_chroma_error_string(int code);
/* 0: sizeof(fldr_chroma_format), 1: fldr_chroma_frame, 2: fldr_chroma_io, 3: fldr_chroma_session_config — binding self-check;
 * FLDR_CHROMA_E_ARG otherwise */
FLDR_CHROMA_API int         fldr_chroma_sizeof(int which);

/* The two converters alone, for callers that feed fldr_model_forward themselves.  H, W >= 1.
 * to_planar: n_frames frames in `format` -> the model's planar BGR [n_frames,3,H,W] at `planar` (device memory; uint8, or uint16 code
 * values 0 .. 1023 at depth 10, then 2-byte aligned). */
FLDR_CHROMA_API int fldr_chroma_to_planar(const fldr_chroma_frame* frames, int n_frames, const fldr_chroma_format* format, void* planar,
                                          int H, int W, void* stream);
/* from_planar: one planar BGR frame [3,H,W] (uint8, or uint16 at depth 10) -> out_frame in `format`. */
FLDR_CHROMA_API int fldr_chroma_from_planar(const void* planar, const fldr_chroma_format* format, const fldr_chroma_frame* out_frame,
                                            int H, int W, void* stream);

/* Bytes of workspace one forward of an H x W pair with n_t outputs needs, whatever the formats, laid out as fldr_video_workspace_bytes
 * lays it out: fldr_model_workspace_bytes, then the planar BGR pair ([1,2,3,H,W]: uint8, or uint16 for a 10-bit input), then n_t planar
 * BGR outputs ([1,3,H,W] each: uint8, or uint16 for a 10-bit output), each part starting 256-byte aligned: the pair at align(model
 * bytes), output k at pair + align(6 H W b_in) + k align(3 H W b_out) with b = bytes per sample of that side.  The size is that of the
 * 16-bit regions.  After a forward the planar frames stay there.  Negative on bad arguments. */
FLDR_CHROMA_API int64_t fldr_chroma_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue one forward on `stream` (NULL = the null stream): the input conversion, one fldr_model_forward (FLDR_MODEL_IN_U8_PLANAR /
 * OUT_U8_PLANAR, or the U10 forms for a 10-bit side) and n_t output conversions.  ws: device memory of at least
 * fldr_chroma_workspace_bytes, 256-byte aligned, not used by another forward in flight.  H, W >= 2. */
FLDR_CHROMA_API int fldr_chroma_forward(const fldr_model* model, const fldr_chroma_io* io, void* ws, int64_t ws_bytes, void* stream);

/* ---- sessions: a stream of host frames; each frame is uploaded once and is the second frame of one pair and the first of the next */
FLDR_CHROMA_API int  fldr_chroma_session_create(const fldr_model* model, const fldr_chroma_session_config* cfg, fldr_chroma_session** out);
/* Upload `frame` (host planes in cfg->in_format); if a previous frame is held, interpolate n_t frames between it and this one into
 * host_outs[0 .. n_t-1] (host planes in cfg->out_format).  Synchronises before it returns.  *n_out: 0 on the first push and the first
 * after a reset, n_t otherwise (host_outs may be NULL when no output is due). */
FLDR_CHROMA_API int  fldr_chroma_session_push(fldr_chroma_session* s, const fldr_chroma_frame* frame, const fldr_chroma_frame* host_outs,
                                              int* n_out);
/* Forget the previous frame (a scene cut): the next push returns no output. */
FLDR_CHROMA_API int  fldr_chroma_session_reset(fldr_chroma_session* s);
FLDR_CHROMA_API void fldr_chroma_session_destroy(fldr_chroma_session* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_CHROMA_H */
