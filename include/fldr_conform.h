/*
 * fldr_conform.h — conform API of libfldr_conform.so: direct YUV 4:2:0 -> YUV 4:2:0 conversion on the device between any two
 * fldr_video_format: matrix (BT.601 <-> BT.709), range (limited <-> full), depth (8 <-> 10, with optional ordered dither on the way
 * down) and layout (NV12 <-> I420, P010 <-> yuv420p10le), with the picture placed on a larger black canvas (pillarbox, letterbox), on
 * top of the rate API (include/fldr_rate.h).  576i50 material that has been deinterlaced and resized becomes a BT.709 10-bit HD frame
 * with bars left and right without a trip through RGB.
 *
 * Plain C99; no device header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Error codes.  This header defines no code of its own.  Its own argument errors — a null pointer, a size outside 1 .. 16384, a dst_x
 * or dst_y that is odd or negative, a picture that does not fit the canvas, a dither word out of range, a non-zero reserved word, an
 * output that overlaps the source, a view origin that is odd or negative, a null model where a forward runs — return FLDR_RATE_E_ARG;
 * a ratio of the rates the converter does not take returns FLDR_RATE_E_RATIO; no such device or a failed allocation returns
 * FLDR_RATE_E_DEVICE.  FLDR_RATE_E_STATE is not returned by this library's own checks.  Codes of the video and model libraries pass
 * through (FLDR_VIDEO_E_FORMAT, FLDR_VIDEO_E_PLANE, FLDR_VIDEO_E_PITCH for a bad format or frame), and so does a positive hipError_t.
 * fldr_conform_error_string is fldr_rate_error_string.
 *
 * THE RULE.  A side is a fldr_video_format with depth D (8 or 10), sh = D - 8 and mx = 2^D - 1.  The sample value s(.) is the byte at
 * depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le.  Per side
 *     yo = 16 << sh (limited) or 0 (full)          ys = 219 << sh (limited) or mx (full)
 *     cc = 2^(D-1)                                 cs = 224 << sh (limited) or mx (full)
 * and the subscripts s and d mean source and destination.
 *
 *   Matrix terms.  Kr, Kb: 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709); Kg = 1 - Kr - Kb.  A is the source matrix, B the
 *   destination's.  With equal matrices myu = myv = muv = mvu = 0 and muu = mvv = 1, exactly, by definition and not by evaluation.
 *   Otherwise
 *     myu = 2(1-KbA)(KbB - KgB KbA/KgA)      myv = 2(1-KrA)(KrB - KgB KrA/KgA)
 *     muu = (2(1-KbA) - myu) / (2(1-KbB))    muv = -myv / (2(1-KbB))
 *     mvv = (2(1-KrA) - myv) / (2(1-KrB))    mvu = -myu / (2(1-KrB))
 *   which is YCbCr(A) -> R'G'B' -> YCbCr(B) multiplied out: Y' = Y + myu Cb + myv Cr, Cb' = muu Cb + muv Cr, Cr' = mvu Cb + mvv Cr.
 *
 *   The integer table (fldr_conform_coefs, pure host arithmetic in double) has 14 fraction bits, r(v) = floor(v * 16384 + 0.5):
 *     KYY = r(ys_d/ys_s)      KYU = r(myu ys_d/cs_s)  KYV = r(myv ys_d/cs_s)
 *     KUU = r(muu cs_d/cs_s)  KUV = r(muv cs_d/cs_s)  KVU = r(mvu cs_d/cs_s)  KVV = r(mvv cs_d/cs_s)
 *   BT.601 -> BT.709, limited, 8 -> 8: 16384, -1893, -3407, 16689, 1878, 1230, 16799.
 *
 *   Arithmetic, all integer, arithmetic (floor) shifts, one clamp to [0, mx_d] at the end.
 *     chroma (at chroma sites; no resampling, no re-siting):
 *       U' = cc_d + ((KUU (U - cc_s) + KUV (V - cc_s) + RC) >> 14)
 *       V' = cc_d + ((KVU (U - cc_s) + KVV (V - cc_s) + RC) >> 14)
 *     luma:
 *       Y' = yo_d + ((8 KYY (Y - yo_s) + KYU cu + KYV cv + RY) >> 17)
 *   cu and cv are the source chroma upsampled to the luma site with the video library's taps, total weight 8, minus 8 cc_s: horizontal
 *   weight 2 on x/2 for even x and 1 + 1 on (x-1)/2, (x+1)/2 for odd x; vertical weights (1, 3) on rows y/2 - 1, y/2 for even y and
 *   (3, 1) on (y-1)/2, (y+1)/2 for odd y; indices clamp to the plane.  RY = 1 << 16 and RC = 1 << 13.
 *   Under FLDR_CONFORM_DITHER_ORDERED RY = (2 b + 1) << 10 and RC = (2 b + 1) << 7 with b = B8[y & 7][x & 7] at the OUTPUT plane's own
 *   coordinates (for NV12 chroma x is the chroma column, not the byte) and B8 the 8 x 8 Bayer matrix:
 *     b = sum over i = 0..2 of (((x>>i ^ y>>i) & 1) << (5 - 2i)) | (((y>>i) & 1) << (4 - 2i))             (its corner: 0 32 / 48 16)
 *   With equal formats every output equals its input sample, dither or not: an exact multiple of the divisor plus a rounding term below
 *   it.  Outputs are written in the container's canonical form: << 6 for P010, the high bits zero for yuv420p10le.  Every intermediate
 *   fits int32 with room: the worst luma sum over all 256 format pairs is 1.82e8.  tests/conform_oracle.py is the numpy statement.
 *
 *   Placement.  The output is an out_H x out_W canvas; the picture, in_H x in_W, sits with its top-left luma sample at (dst_x, dst_y),
 *   both even, and must fit.  A luma sample outside the picture is yo_d; a chroma sample whose index lies outside
 *   [dst/2, dst/2 + ceil(in/2)) on either axis is cc_d: black of the destination range and depth.  Everything else is the conversion
 *   of the source sample at the shifted index.  Cropping needs no kernel: fldr_conform_view returns the plane pointers of the window of
 *   a frame that starts at even (x, y), and since the conversion clamps chroma indices to the planes it is given — in_H x in_W — a view
 *   is a picture in its own right.
 *
 *   Limits: every luma size is 1 .. FLDR_CONFORM_MAX_SIZE = 16384.  Anything else is FLDR_RATE_E_ARG, before any device call.
 *
 * Three layers:
 *
 * 1. fldr_conform_coefs, fldr_conform_view: the table and the crop, on the host.
 *
 * 2. fldr_conform_frame: the kernel that conforms one device frame: one launch for all planes, the coefficients as kernel arguments (no
 *    map object, no device table).  With equal matrices the luma pass reads no chroma.
 *
 * 3. fldr_conform_* streams: host frames in the IN format at in_num / in_den per second in, host frames in the OUT format on the
 *    canvas at out_num / out_den out.  The schedule is fldr_rate.h's.
 *      Contract of the stream: output j is, byte for byte, the conform of output j of a fldr_rate of the same rates and scene settings
 *    at the in size and format, pushed the same frames — the outputs that land on an input frame and the ones replaced on a cut
 *    included.  With equal rates (B == 1) no forward ever runs: the model may then be NULL and no model workspace is allocated — a pure
 *    converter.  After a failed enqueue or wait the object is as after a reset.  Argument errors change nothing.  One thread drives a
 *    stream.
 *
 * Contract of fldr_conform_frame: fldr_scene_measure's.  It enqueues on `stream`; no allocation, no synchronisation, no host<->device
 * copy: it can be captured into a graph.  Every argument is validated before anything is enqueued.  Output bytes between a row's end
 * and its pitch are never written.  `out` must not overlap `in`.
 *
 * Known costs and limits:
 *   - BT.2020 is not in fldr_video_format and is out of scope;
 *   - no transfer-function or primaries conversion: 601 -> 709 here is the matrix only;
 *   - the fill is black only;
 *   - the clamp is to [0, mx], not to the nominal range;
 *   - chroma siting is "left" only;
 *   - 4:2:2, 4:4:4, packed and RGB formats are out of scope;
 *   - the stream is synchronous: it synchronises in every push, as the rate converter does.
 */
#ifndef FLDR_CONFORM_H
#define FLDR_CONFORM_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_CONFORM_VERSION 100         /* major*10000 + minor*100 + patch of this header */

#define FLDR_CONFORM_API __attribute__((visibility("default")))

#define FLDR_CONFORM_MAX_SIZE 16384      /* the largest luma size, either axis, either side */

#define FLDR_CONFORM_DITHER_NONE    0    /* RY = 1 << 16, RC = 1 << 13 */
#define FLDR_CONFORM_DITHER_ORDERED 1    /* the 8 x 8 Bayer matrix in the rounding term */

/* the order of the seven words fldr_conform_coefs writes */
#define FLDR_CONFORM_KYY 0
#define FLDR_CONFORM_KYU 1
#define FLDR_CONFORM_KYV 2
#define FLDR_CONFORM_KUU 3
#define FLDR_CONFORM_KUV 4
#define FLDR_CONFORM_KVU 5
#define FLDR_CONFORM_KVV 6

FLDR_CONFORM_API int         fldr_conform_version(void);
FLDR_CONFORM_API const char* fldr_conform_error_string(int code);
/* 0: sizeof(fldr_conform_config), 1: fldr_conform_stream_config — binding self-check; FLDR_RATE_E_ARG otherwise */
FLDR_CONFORM_API int         fldr_conform_sizeof(int which);

/* ---- host only: no device is touched ------------------------------------------------------------------------------------------------- */
/* The integer table of src -> dst: coef[FLDR_CONFORM_KYY .. FLDR_CONFORM_KVV].  Layouts do not enter.  FLDR_RATE_E_ARG for a null
 * pointer, FLDR_VIDEO_E_FORMAT for a bad format. */
FLDR_CONFORM_API int fldr_conform_coefs(const fldr_video_format* src, const fldr_video_format* dst, int32_t coef[7]);
/* *view = the window of `frame` (in *fmt) whose top-left luma sample is (x, y): plane 0 moved by y rows and x samples, the chroma
 * planes by y/2 rows and x/2 columns; the pitches are the frame's.  Checked in this order: a null pointer, x or y odd or negative
 * (FLDR_RATE_E_ARG); the format (FLDR_VIDEO_E_FORMAT); a null plane (FLDR_VIDEO_E_PLANE).  The caller picks a window that lies inside
 * the frame: its size is the in_H x in_W of the conform that reads it. */
FLDR_CONFORM_API int fldr_conform_view(const fldr_video_frame* frame, const fldr_video_format* fmt, int x, int y, fldr_video_frame* view);

/* ---- the kernel entry ------------------------------------------------------------------------------------------------------------------ */
typedef struct fldr_conform_config {
    int32_t           in_H, in_W;        /* luma size of the picture */
    fldr_video_format in_format;
    int32_t           out_H, out_W;      /* luma size of the canvas */
    fldr_video_format out_format;
    int32_t           dst_x, dst_y;      /* where the picture's top-left luma sample sits on the canvas: even, not negative */
    int32_t           dither;            /* FLDR_CONFORM_DITHER_NONE / _ORDERED */
    int32_t           reserved[3];       /* zero */
} fldr_conform_config;

/* Enqueue the conform of `in` (device planes, in_H x in_W in in_format) into `out` (device planes, out_H x out_W in out_format).
 * Checked in this order: cfg, in or out null, the four sizes, dst_x / dst_y odd or negative, a picture that does not fit, dither, the
 * reserved words (FLDR_RATE_E_ARG); in_format, then out_format (FLDR_VIDEO_E_FORMAT); the planes, then the pitches, of `in`, then of
 * `out` (FLDR_VIDEO_E_PLANE / FLDR_VIDEO_E_PITCH); an `out` that overlaps `in` (FLDR_RATE_E_ARG).  A lane owns 16 bytes of an output
 * row: it stores them as one 16-byte word where the address allows it and sample by sample otherwise, as a row's last, partial run
 * always is; the bytes are the same. */
FLDR_CONFORM_API int fldr_conform_frame(const fldr_conform_config* cfg, const fldr_video_frame* in, const fldr_video_frame* out, void* stream);

/* ---- the stream: host frames in the in format and rate in, host frames in the out format, on the canvas, at the out rate out ---------- */
typedef struct fldr_conform_stream_config {
    fldr_rate_config  rate;              /* as fldr_rate_create takes it; H, W, format: the IN side */
    int32_t           out_H, out_W;      /* luma size of the canvas */
    fldr_video_format out_format;
    int32_t           dst_x, dst_y;
    int32_t           dither;
    int32_t           reserved[4];       /* zero */
} fldr_conform_stream_config;

typedef struct fldr_conform fldr_conform;

/* Validation order: cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words,
 * thresholds, format, rate terms, the ratio of the rates: FLDR_RATE_E_RATIO); then this library's own words, as fldr_conform_frame
 * checks them: the sizes, dst_x / dst_y, the fit, dither, the reserved words (FLDR_RATE_E_ARG), out_format (FLDR_VIDEO_E_FORMAT); then a
 * null model with B != 1 (FLDR_RATE_E_ARG) and the model's code for a frame it does not take: all before any device call.  Then no
 * such device or a failed allocation (FLDR_RATE_E_DEVICE).  *cfg is never written. */
FLDR_CONFORM_API int  fldr_conform_create(const fldr_model* model, const fldr_conform_stream_config* cfg, fldr_conform** out);
/* ceil(B / A): the most frames one push can return; negative (FLDR_RATE_E_ARG) on a null handle */
FLDR_CONFORM_API int  fldr_conform_max_out(const fldr_conform* s);
/* Frame n of the stream, in_H x in_W in the in format.  host_outs: fldr_conform_max_out frames of out_H x out_W in the out format, of
 * which [0 .. *n_out - 1] are written (may be NULL when no output is due).  scene (may be NULL): as fldr_rate_push fills it.
 * Synchronises before it returns. */
FLDR_CONFORM_API int  fldr_conform_push(fldr_conform* s, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                        fldr_scene_result* scene);
/* End of the stream: the one output, if any, that lands exactly on the last pushed frame.  A second flush returns none. */
FLDR_CONFORM_API int  fldr_conform_flush(fldr_conform* s, const fldr_video_frame* host_outs, int* n_out);
/* Forget everything pushed: the next push is frame 0 of a new stream, output 0 included. */
FLDR_CONFORM_API int  fldr_conform_reset(fldr_conform* s);
FLDR_CONFORM_API void fldr_conform_destroy(fldr_conform* s);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_CONFORM_H */
