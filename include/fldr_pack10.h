/*
 * fldr_pack10.h — API of libfldr_pack10.so: frame interpolation on the packed 10-bit YUV formats that capture cards and hardware
 * decoders deliver (v210, Y210, Y410 / xv30le), on top of the C model API (include/fldr_model.h).  A sibling of the other YUV
 * libraries, with its own format struct; a frame is ONE plane.
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_model.h.
 *
 * Containers.  All are little-endian and hold 10-bit code values 0 .. 1023; every value passes through (SDI's
 * reserved codes are not policed).
 *   v210   4:2:2.  A row is ceil(W/6) groups of 16 bytes; a group is four 32-bit words of three samples each, at bits 0-9, 10-19 and
 *          20-29 (bits 30-31 are ignored on input and written as zero):
 *              word 0 = U0 Y0 V0    word 1 = Y1 U1 Y2    word 2 = V1 Y3 U2    word 3 = Y4 V2 Y5      (lowest field first)
 *          for the six pixels Y0 .. Y5 and their three chroma pairs.  With W % 6 != 0 the last group has spare slots: they are ignored
 *          on input; on output a spare luma slot repeats luma W - 1 and a spare chroma slot repeats chroma sample ceil(W/2) - 1, so a
 *          written row is fully defined.  row bytes = 16 ceil(W/6); the customary pitch 128 ceil(W/48) is merely one valid pitch.
 *   Y210   4:2:2.  16-bit words Y0 U Y1 V per two pixels, the value in the high 10 bits (word = v << 6; the low 6 bits are ignored on
 *          input and written as zero).  row bytes = 8 ceil(W/2); with odd W the second luma word of the last group is ignored on input
 *          and written as a copy of the last luma sample.
 *   Y410   4:4:4.  One 32-bit word per pixel: U in bits 0-9, Y in 10-19, V in 20-29, alpha in 30-31 (ignored on input, written as 3).
 *          ffmpeg's xv30le is the same layout with the top bits unused.  row bytes = 4 W.
 *
 * Colour: the integer fixed point of fldr_video.h at depth 10 (BT.601 or BT.709, limited or full range, 16 fraction bits, the same
 * tables).  4:2:2 chroma is co-sited with the even luma columns ("left") and has no vertical taps: chroma is interpolated along the row
 * with the 4:2:0 horizontal taps, and decimated along the row with (1, 2, 1).  4:4:4 has no taps at all.  Odd widths and heights are
 * allowed.  A frame in one of these containers gives byte for byte the planar 10-bit BGR that the same samples give as yuv422p10le /
 * yuv444p10le through the planar 4:2:2 / 4:4:4 library, and the same holds for the way back.  No transfer function is applied.
 *
 * Contract (that of fldr_video.h):
 *   - fldr_pack10_to_planar, fldr_pack10_from_planar and fldr_pack10_forward enqueue on `stream`.  No allocation, no synchronisation,
 *     no host<->device copy: they can be captured into a graph.  Arguments are validated before anything is enqueued.  A device fault
 *     flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); no output frame is then written.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API (fldr_pack10_session_*) owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_PACK10_E_* code, a negative FLDR_MODEL_E_* code passed through from the model, or a
 * positive hipError_t from the runtime.
 *
 * Out of scope: 12-bit and 16-bit packed formats (Y212, Y216, Y416), big-endian v210 variants, alpha and interlaced material.
 */
#ifndef FLDR_PACK10_H
#define FLDR_PACK10_H

#include <stdint.h>

#include "fldr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_PACK10_VERSION 100          /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -800 and below; the ranges above belong to the model and the other libraries */
#define FLDR_PACK10_E_ARG        (-800)  /* null pointer, bad size, n_t < 1, null model */
#define FLDR_PACK10_E_FORMAT     (-801)  /* unknown container / matrix / range, a depth other than 10, or a non-zero reserved word */
#define FLDR_PACK10_E_PITCH      (-802)  /* a pitch shorter than its row, or not a multiple of 4 (v210, Y410) / of 2 (Y210) */
#define FLDR_PACK10_E_PLANE      (-803)  /* a null plane pointer, or an address that is not a multiple of 4 (v210, Y410) / of 2 (Y210) */
#define FLDR_PACK10_E_WORKSPACE  (-804)  /* workspace null, not 256-byte aligned or smaller than fldr_pack10_workspace_bytes */
#define FLDR_PACK10_E_DEVICE     (-805)  /* session: no such device, or an allocation failed */

#define FLDR_PACK10_API __attribute__((visibility("default")))

enum { FLDR_PACK10_V210 = 0,             /* 4:2:2, 16-byte groups of six pixels */
       FLDR_PACK10_Y210 = 1,             /* 4:2:2, 16-bit words Y0 U Y1 V, value in the high 10 bits */
       FLDR_PACK10_Y410 = 2 };           /* 4:4:4, one 32-bit word per pixel: U, Y, V, alpha */
enum { FLDR_PACK10_BT601 = 0, FLDR_PACK10_BT709 = 1 };
enum { FLDR_PACK10_LIMITED = 0,          /* Y 64 .. 940, C 64 .. 960 */
       FLDR_PACK10_FULL = 1 };           /* the whole code range */

typedef struct fldr_pack10_format {
    int32_t container;                   /* FLDR_PACK10_V210 / Y210 / Y410 */
    int32_t matrix;                      /* FLDR_PACK10_BT601 / FLDR_PACK10_BT709 */
    int32_t range;                       /* FLDR_PACK10_LIMITED / FLDR_PACK10_FULL */
    int32_t depth;                       /* 10 */
    int32_t reserved[4];                 /* zero */
} fldr_pack10_format;

/* One frame: only plane[0] / pitch[0] are read (row r at plane[0] + r * pitch[0], the pitch in bytes); the other two entries keep the
 * struct laid out as the frames of the other YUV libraries. */
typedef struct fldr_pack10_frame {
    void*   plane[3];
    int64_t pitch[3];
} fldr_pack10_frame;

/* One forward: all plane pointers and `t` are device pointers; `out` is a host array of n_t frames, read during the call. */
typedef struct fldr_pack10_io {
    int32_t                  H, W;       /* frame size (luma) */
    fldr_pack10_format       in_format;
    fldr_pack10_frame        in[2];      /* I0, I1 */
    fldr_pack10_format       out_format; /* may differ from in_format in everything (v210 in, Y410 out) */
    int32_t                  n_t;        /* outputs: >= 1 */
    const float*             t;          /* n_t floats on the device (output k at t[k]); may be rewritten between graph replays */
    const fldr_pack10_frame* out;        /* n_t frames in out_format */
} fldr_pack10_io;

typedef struct fldr_pack10_session_config {
    int32_t            H, W;
    fldr_pack10_format in_format;        /* of the host frames pushed */
    fldr_pack10_format out_format;       /* of the host frames returned */
    int32_t            n_t;              /* interpolated frames per pushed frame: >= 1 */
    int32_t            device;           /* HIP device ordinal: the model's */
    const float*       t;                /* host array of n_t times, copied at create; NULL: t[k] = (k + 1) / (n_t + 1) */
    int32_t            reserved[4];      /* zero */
} fldr_pack10_session_config;

typedef struct fldr_pack10_session fldr_pack10_session;

FLDR_PACK10_API int         fldr_pack10_version(void);
FLDR_PACK10_API const char* fldr_pack10_error_string(int code);
/* 0: sizeof(fldr_pack10_format), 1: fldr_pack10_frame, 2: fldr_pack10_io, 3: fldr_pack10_session_config — binding self-check;
 * FLDR_PACK10_E_ARG otherwise */
FLDR_PACK10_API int         fldr_pack10_sizeof(int which);

/* The two converters alone, for callers that feed fldr_model_forward themselves.  H, W >= 1.
 * to_planar: n_frames frames in `format` -> the model's planar BGR [n_frames,3,H,W] at `planar` (device memory; uint16 code values
 * 0 .. 1023, 2-byte aligned). */
FLDR_PACK10_API int fldr_pack10_to_planar(const fldr_pack10_frame* frames, int n_frames, const fldr_pack10_format* format, void* planar,
                                          int H, int W, void* stream);
/* from_planar: one planar BGR frame [3,H,W] (uint16 code values) -> out_frame in `format`. */
FLDR_PACK10_API int fldr_pack10_from_planar(const void* planar, const fldr_pack10_format* format, const fldr_pack10_frame* out_frame,
                                            int H, int W, void* stream);

/* Bytes of workspace one forward of an H x W pair with n_t outputs needs, whatever the containers, laid out as
 * fldr_video_workspace_bytes lays it out for 10-bit sides: fldr_model_workspace_bytes, then the planar BGR pair ([1,2,3,H,W] uint16),
 * then n_t planar BGR outputs ([1,3,H,W] uint16 each), each part starting 256-byte aligned: the pair at align(model bytes), output k at
 * pair + align(12 H W) + k align(6 H W).  After a forward the planar frames stay there.  Negative on bad arguments. */
FLDR_PACK10_API int64_t fldr_pack10_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue one forward on `stream` (NULL = the null stream): the input conversion, one fldr_model_forward (FLDR_MODEL_IN_U10_PLANAR /
 * OUT_U10_PLANAR) and n_t output conversions.  ws: device memory of at least fldr_pack10_workspace_bytes, 256-byte aligned, not used by
 * another forward in flight.  H, W >= 2. */
FLDR_PACK10_API int fldr_pack10_forward(const fldr_model* model, const fldr_pack10_io* io, void* ws, int64_t ws_bytes, void* stream);

/* ---- sessions: a stream of host frames; each frame is uploaded once and is the second frame of one pair and the first of the next */
FLDR_PACK10_API int  fldr_pack10_session_create(const fldr_model* model, const fldr_pack10_session_config* cfg, fldr_pack10_session** out);
/* Upload `frame` (a host plane in cfg->in_format); if a previous frame is held, interpolate n_t frames between it and this one into
 * host_outs[0 .. n_t-1] (host planes in cfg->out_format; bytes between a row's end and its pitch are not written).  Synchronises before
 * it returns.  *n_out: 0 on the first push and the first after a reset, n_t otherwise (host_outs may be NULL when no output is due). */
FLDR_PACK10_API int  fldr_pack10_session_push(fldr_pack10_session* s, const fldr_pack10_frame* frame, const fldr_pack10_frame* host_outs,
                                              int* n_out);
/* Forget the previous frame (a scene cut): the next push returns no output. */
FLDR_PACK10_API int  fldr_pack10_session_reset(fldr_pack10_session* s);
FLDR_PACK10_API void fldr_pack10_session_destroy(fldr_pack10_session* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_PACK10_H */
