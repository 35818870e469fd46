/*
 * fldr_rgb.h — API of libfldr_rgb.so: frame interpolation on the RGB frames that desktop and game capture, compositors, graphics
 * interop surfaces, image libraries and image-sequence tools deliver (four bytes per pixel, 10-bit RGB in one 32-bit word, planar
 * GBR at 8 or 10 bits), with alpha, on top of the C model API (include/fldr_model.h).  A sibling of the YUV libraries, with its own
 * format struct; a frame has one, three or four planes.
 *
 * Plain C99; no HIP header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_model.h.
 *
 * Layouts.  W pixels per row, H rows.
 *   BGRA, RGBA, ARGB, ABGR   depth 8 (0 means 8).  One plane, four bytes per pixel in the named order in memory (ffmpeg bgra / rgba /
 *                            argb / abgr; with the alpha policy OPAQUE on both sides these are bgr0 / rgb0 / 0rgb / 0bgr).
 *                            row bytes = 4 W; the plane and its pitch are multiples of 4.
 *   X2RGB10                  depth 10.  One plane, one little-endian 32-bit word per pixel: B in bits 0-9, G in 10-19, R in 20-29, a
 *                            2-bit alpha in 30-31 (ffmpeg x2rgb10le; A2R10G10B10).  row bytes = 4 W, multiples of 4.
 *   X2BGR10                  the same with R in bits 0-9 and B in 20-29 (ffmpeg x2bgr10le; R10G10B10A2).
 *   GBRP                     depth 8 or 10.  Three planes in the order G, B, R (ffmpeg gbrp; depth 10: gbrp10le, 16-bit little-endian
 *                            words with the value in the low 10 bits: input is masked with 0x3ff, the upper bits are written zero).
 *                            row bytes = W or 2 W; at depth 10 planes and pitches are even.
 *   GBRAP                    the same with a fourth plane A (ffmpeg gbrap, gbrap10le).
 * Worked example: the pixel R = 1023, G = 0, B = 1 with alpha 3 is the word 0xFFF00001 as X2RGB10 and 0xC01003FF as X2BGR10.
 *
 * Colour.  Plane c of the model's planar frame is BGR channel c.  No colour arithmetic happens anywhere in this library: a colour code
 * value goes in and comes out as it is (at depth 10, what the model writes is 0 .. 1023).
 *
 * Alpha.  The policy is format.alpha of the OUT format of a forward; it is ignored where the out layout has no alpha (GBRP).
 *   OPAQUE   input alpha is ignored; output alpha is the largest code: 255, 1023, or 3 for the 2-bit field.
 *   NEARER   the alpha of output k is the alpha of in[t[k] < 0.5f ? 0 : 1] at the same pixel; t is read on the device.
 *   BLEND    w = t[k] >= 0 ? min(rintf(t[k] * 65536.0f), 65536) : 0, then a = (a0 * (65536 - w) + a1 * w + 32768) >> 16 in uint32,
 *            a0 / a1 the alpha of in[0] / in[1] at the same pixel.  A NaN t fails the comparison and gives w = 0.  The arithmetic is
 *            exact integer arithmetic (t * 65536 is exact in fp32): a0 = 255, a1 = 0 gives 128 at t = 0.5 and 191 at t = 0.25.
 * NEARER and BLEND need an input format that has alpha of the output's width: 8 bits with 8 (the byte layouts, GBRAP at depth 8), 10
 * with 10 (GBRAP at depth 10), 2 with 2 (the two 10-bit word layouts); the layouts themselves may differ (ARGB in, GBRAP out).  Any
 * other combination is FLDR_RGB_E_FORMAT.  With OPAQUE, or an out layout without alpha, a forward launches nothing for alpha.
 *
 * Contract (that of fldr_video.h):
 *   - fldr_rgb_to_planar, fldr_rgb_from_planar, fldr_rgb_alpha and fldr_rgb_forward enqueue on `stream`.  No allocation, no
 *     synchronisation, no host<->device copy: they can be captured into a graph.  Arguments are validated before anything is enqueued.
 *     A device fault flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS); no output frame is then written.
 *   - Output bytes between a row's end and its pitch are never written.
 *   - The session API (fldr_rgb_session_*) owns its device memory, pinned staging and stream, and synchronises in every push.
 * Every function returns 0, a negative FLDR_RGB_E_* code, a negative FLDR_MODEL_E_* code passed through from the model, or a positive
 * hipError_t from the runtime.
 *
 * Out of scope: 16-bit RGB (rgb48, rgba64: the model carries 10 bits), big-endian r210 / x2rgb10be, float formats, and premultiplied
 * alpha as such (colour is interpolated as given, whatever it was multiplied with).
 */
#ifndef FLDR_RGB_H
#define FLDR_RGB_H

#include <stdint.h>

#include "fldr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_RGB_VERSION 100             /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -900 and below; the ranges above belong to the model and the other libraries */
#define FLDR_RGB_E_ARG        (-900)     /* null pointer, bad size, n_t < 1, null model */
#define FLDR_RGB_E_FORMAT     (-901)     /* unknown layout / depth pair or alpha policy, a non-zero reserved word, or NEARER / BLEND
                                            from an input without alpha of the output's width */
#define FLDR_RGB_E_PITCH      (-902)     /* a pitch shorter than its row, or not a multiple of 4 (word layouts) / of 2 (planar, depth 10) */
#define FLDR_RGB_E_PLANE      (-903)     /* a null plane pointer, or an address that is not a multiple of 4 / of 2 (as for the pitch) */
#define FLDR_RGB_E_WORKSPACE  (-904)     /* workspace null, not 256-byte aligned or smaller than fldr_rgb_workspace_bytes */
#define FLDR_RGB_E_DEVICE     (-905)     /* session: no such device, or an allocation failed */

#define FLDR_RGB_API __attribute__((visibility("default")))

enum { FLDR_RGB_BGRA = 0,                /* bytes B, G, R, A */
       FLDR_RGB_RGBA = 1,                /* bytes R, G, B, A */
       FLDR_RGB_ARGB = 2,                /* bytes A, R, G, B */
       FLDR_RGB_ABGR = 3,                /* bytes A, B, G, R */
       FLDR_RGB_X2RGB10 = 4,             /* one word: B 0-9, G 10-19, R 20-29, alpha 30-31 */
       FLDR_RGB_X2BGR10 = 5,             /* one word: R 0-9, G 10-19, B 20-29, alpha 30-31 */
       FLDR_RGB_GBRP = 6,                /* planes G, B, R */
       FLDR_RGB_GBRAP = 7 };             /* planes G, B, R, A */
enum { FLDR_RGB_ALPHA_OPAQUE = 0,        /* write the largest code */
       FLDR_RGB_ALPHA_NEARER = 1,        /* the alpha of the input nearer in time */
       FLDR_RGB_ALPHA_BLEND = 2 };       /* the inputs' alpha blended at t, 16 fraction bits */

typedef struct fldr_rgb_format {
    int32_t layout;                      /* FLDR_RGB_BGRA .. FLDR_RGB_GBRAP */
    int32_t depth;                       /* byte layouts: 8 (0 means 8); X2RGB10 / X2BGR10: 10; GBRP / GBRAP: 8 or 10 */
    int32_t alpha;                       /* FLDR_RGB_ALPHA_*: read from the out format of a forward */
    int32_t reserved[5];                 /* zero */
} fldr_rgb_format;

/* One frame: plane p's row r is at plane[p] + r * pitch[p] (the pitch in bytes).  The word layouts read plane[0] only; GBRP reads
 * three entries (G, B, R), GBRAP four (G, B, R, A). */
typedef struct fldr_rgb_frame {
    void*   plane[4];
    int64_t pitch[4];
} fldr_rgb_frame;

/* One forward: all plane pointers and `t` are device pointers; `out` is a host array of n_t frames, read during the call. */
typedef struct fldr_rgb_io {
    int32_t               H, W;          /* frame size */
    fldr_rgb_format       in_format;
    fldr_rgb_frame        in[2];         /* I0, I1 */
    fldr_rgb_format       out_format;    /* may differ from in_format in everything (BGRA in, X2RGB10 out, with OPAQUE) */
    int32_t               n_t;           /* outputs: >= 1 */
    const float*          t;             /* n_t floats on the device (output k at t[k]); may be rewritten between graph replays */
    const fldr_rgb_frame* out;           /* n_t frames in out_format */
} fldr_rgb_io;

typedef struct fldr_rgb_session_config {
    int32_t         H, W;
    fldr_rgb_format in_format;           /* of the host frames pushed */
    fldr_rgb_format out_format;          /* of the host frames returned; its alpha policy is the session's */
    int32_t         n_t;                 /* interpolated frames per pushed frame: >= 1 */
    int32_t         device;              /* HIP device ordinal: the model's */
    const float*    t;                   /* host array of n_t times, copied at create; NULL: t[k] = (k + 1) / (n_t + 1) */
    int32_t         reserved[4];         /* zero */
} fldr_rgb_session_config;

typedef struct fldr_rgb_session fldr_rgb_session;

FLDR_RGB_API int         fldr_rgb_version(void);
FLDR_RGB_API const char* fldr_rgb_error_string(int code);
/* 0: sizeof(fldr_rgb_format), 1: fldr_rgb_frame, 2: fldr_rgb_io, 3: fldr_rgb_session_config — binding self-check; FLDR_RGB_E_ARG
 * otherwise */
FLDR_RGB_API int         fldr_rgb_sizeof(int which);

/* The two converters alone, for callers that feed fldr_model_forward themselves.  H, W >= 1.
 * to_planar: n_frames frames in `format` -> the model's planar BGR [n_frames,3,H,W] at `planar` (device memory; uint8, or uint16 code
 * values 0 .. 1023 at depth 10, 2-byte aligned).  Alpha is not read (the A plane of a GBRAP frame must be a valid plane all the same). */
FLDR_RGB_API int fldr_rgb_to_planar(const fldr_rgb_frame* frames, int n_frames, const fldr_rgb_format* format, void* planar, int H, int W,
                                    void* stream);
/* from_planar: one planar BGR frame [3,H,W] (uint8, or uint16 at depth 10: the low 10 bits are taken) -> out_frame in `format`.  Alpha
 * is written opaque whatever format->alpha says: the other policies need the two input frames, which only a forward has. */
FLDR_RGB_API int fldr_rgb_from_planar(const void* planar, const fldr_rgb_format* format, const fldr_rgb_frame* out_frame, int H, int W,
                                      void* stream);

/* The alpha pass alone, for callers that run the two converters and fldr_model_forward themselves: the alpha of the n_out frames `out`
 * in out_format (already written by fldr_rgb_from_planar, so opaque) becomes what out_format->alpha says, from the alpha of the two
 * frames in[0], in[1] in in_format at the same pixel and the n_out times `t` (device memory, read on the device).  Only alpha is
 * written: the A plane of GBRAP, the alpha field of the pixel words (a read-modify-write) otherwise.  With OPAQUE, or an out layout
 * without alpha, nothing is enqueued.  H, W >= 1; one launch per 64 outputs. */
FLDR_RGB_API int fldr_rgb_alpha(const fldr_rgb_frame* in, const fldr_rgb_format* in_format, const fldr_rgb_frame* out, int n_out,
                                const fldr_rgb_format* out_format, const float* t, int H, int W, void* stream);

/* Bytes of workspace one forward of an H x W pair with n_t outputs needs, whatever the formats, laid out as
 * fldr_video_workspace_bytes lays it out for 10-bit sides: fldr_model_workspace_bytes, then the planar BGR pair ([1,2,3,H,W]), then
 * n_t planar BGR outputs ([1,3,H,W] each), each part starting 256-byte aligned and sized for uint16: the pair at align(model bytes),
 * output k at pair + align(6 H W b_in) + k align(3 H W b_out), b = bytes per sample of that side of THIS forward.  After a forward the
 * planar frames stay there.  Negative on bad arguments. */
FLDR_RGB_API int64_t fldr_rgb_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* Enqueue one forward on `stream` (NULL = the null stream): the input conversion, one fldr_model_forward (planar 8- or 10-bit in,
 * planar 8- or 10-bit out, as the two depths say), n_t output conversions and, for NEARER / BLEND into a layout with alpha, one
 * alpha launch per 64 outputs.  ws: device memory of at least fldr_rgb_workspace_bytes, 256-byte aligned, not used by another forward
 * in flight.  H, W >= 2. */
FLDR_RGB_API int fldr_rgb_forward(const fldr_model* model, const fldr_rgb_io* io, void* ws, int64_t ws_bytes, void* stream);

/* ---- sessions: a stream of host frames; each frame is uploaded once and is the second frame of one pair and the first of the next */
FLDR_RGB_API int  fldr_rgb_session_create(const fldr_model* model, const fldr_rgb_session_config* cfg, fldr_rgb_session** out);
/* Upload `frame` (host planes in cfg->in_format); if a previous frame is held, interpolate n_t frames between it and this one into
 * host_outs[0 .. n_t-1] (host planes in cfg->out_format; bytes between a row's end and its pitch are not written).  Synchronises before
 * it returns.  *n_out: 0 on the first push and the first after a reset, n_t otherwise (host_outs may be NULL when no output is due). */
FLDR_RGB_API int  fldr_rgb_session_push(fldr_rgb_session* s, const fldr_rgb_frame* frame, const fldr_rgb_frame* host_outs, int* n_out);
/* Forget the previous frame (a scene cut): the next push returns no output. */
FLDR_RGB_API int  fldr_rgb_session_reset(fldr_rgb_session* s);
FLDR_RGB_API void fldr_rgb_session_destroy(fldr_rgb_session* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_RGB_H */
