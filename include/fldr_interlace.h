/*
 * fldr_interlace.h — interlace API of libfldr_interlace.so: progressive video to interlaced video with TRUE fields.  Every output field
 * is put at its own instant by motion interpolation (24p becomes 59.94i with 59.94 distinct motion phases per second, not the repeated
 * fields of a 3:2 pulldown), vertically filtered against line twitter and woven into frames, on top of the rate API (include/fldr_rate.h).
 *
 * Plain C99; no device header is needed: the stream is a void* (a hipStream_t).  The library calls no fldr_* function but those of
 * fldr_rate.h, fldr_video.h and fldr_model.h.
 *
 * Error codes.  This header defines no code of its own.  Its own argument errors — a null pointer, a bad size, H not a multiple of 4, a
 * filter or parity out of range, a non-zero reserved word, a frame beyond the kernel's index (below), an output that overlaps a source,
 * a null model where a forward runs, a workspace that is null, misaligned or short — return FLDR_RATE_E_ARG; a state that is null or
 * misaligned returns FLDR_RATE_E_STATE; a ratio the converter does not take returns FLDR_RATE_E_RATIO; no such device or a failed
 * allocation returns FLDR_RATE_E_DEVICE.  Codes of the video and model libraries pass through, and so does a positive hipError_t.
 * fldr_interlace_error_string is fldr_rate_error_string.
 *
 * Terms.  A frame is H x W in a fldr_video_format: NV12 or I420 at depth 8 or 10 (P010 and yuv420p10le included).  H is a multiple of 4
 * and at least 4, so that the chroma planes also split into two fields of whole rows; W >= 1 for the kernel, and the model's own minimum
 * applies wherever a forward runs.  The sample value is the byte at depth 8, word >> 6 for P010, word & 0x3ff for yuv420p10le; mx is 255
 * or 1023.
 *
 * Three layers:
 *
 * 1. fldr_interlace_weave: two progressive frames holding two instants -> one woven frame.  In every plane, rows y % 2 == 0 of `out`
 *    come from `even` and rows y % 2 == 1 from `odd`.  Either source, but not both, may be NULL: the rows of that parity are then NEVER
 *    WRITTEN, so a caller fills a frame field by field as the fields become available, with no holding buffer.  Which instant goes to
 *    which parity (the field order) is the caller's business.  The rule is applied to every plane alike; it is purely vertical, so the
 *    interleaved NV12 chroma plane needs no special case.  With R the plane's rows and s(k) the sample value of the row's source at row
 *    clamp(k, 0, R - 1) in the same column, the output sample of row y is
 *        FLDR_INTERLACE_NONE     the row bytes of the source, copied as they are (P010: the low six bits included)
 *        FLDR_INTERLACE_LINEAR   (s(y-1) + 2 s(y) + s(y+1) + 2) >> 2
 *        FLDR_INTERLACE_COMPLEX  clamp((-s(y-2) + 2 s(y-1) + 6 s(y) + 2 s(y+1) - s(y+2) + 4) >> 3, 0, mx), the shift arithmetic (floor)
 *                                on the signed sum
 *    Filtered samples are written in the container's canonical form: o << 6 for P010, the high bits zero for yuv420p10le.  LINEAR and
 *    COMPLEX are the two customary anti-twitter filters: without one, a one-line-high detail lives in one field only and flickers at
 *    frame rate.
 *      Chroma siting.  Plain row selection is correctly sited for 4:2:0.  A progressive chroma row c sits at luma position 2c + 0.5.  In
 *    an interlaced 4:2:0 frame the top field's chroma row j (frame chroma row 2j) sits at 4j + 0.5 and the bottom field's (frame chroma
 *    row 2j + 1) at 4j + 2.5: exactly the progressive rows 2j and 2j + 1.  So, unlike in the deinterlacing library, no quarter-line error
 *    arises.
 *      The frame-size limit.  All offsets are 64-bit.  A work item is one 16-byte column group of one output row, numbered in 32 bits and
 *    split into (row, group) by a multiply-high that is exact while items x groups < 2^32.  With g = ceil(row bytes / 16) of a plane and
 *    R its rows, a frame is refused with FLDR_RATE_E_ARG when g x g x R >= 2^32 = 4294967296 in a plane, or when the planes' g x R sum to
 *    more than 2^31 - 1 = 2147483647.  7680 x 4320 at depth 10 has g = 960 in plane 0: 960 x 960 x 4320 = 3981312000, inside the limit.
 *
 * 2. fldr_interlace_forward: fldr_rate_forward (scene = 1) or fldr_video_forward (scene = 0) of a pair at n_t times into n_t temporary
 *    frames inside the workspace, then one fldr_interlace_weave launch per field from temporary k into the rows parity[k] of pair.out[k].
 *    fldr_interlace_field_frame says where temporary k lives: after a forward it holds, byte for byte, what fldr_rate_forward /
 *    fldr_video_forward gives for that pair and time.
 *
 * 3. fldr_interlace_* streams: progressive host frames at in_num / in_den per second in, woven host frames at out_num / out_den FRAMES
 *    per second out; fields come at twice that.
 *      Schedule.  With A / B = (in_num * out_den) / (in_den * 2 out_num) reduced, field m sits at input position m A / B, by
 *    fldr_rate.h's rule: i = floor(m A / B), r = m A mod B.  r == 0: the field is read straight from the uploaded input frame i, and no
 *    forward runs.  Otherwise it is interpolated from the pair (i, i + 1) at t = (float)r / (float)B; with scene = 1 and the pair a cut
 *    it is the nearer frame instead, as there.  Output frame k holds field 2k in the rows of parity (tff ? 0 : 1) and field 2k + 1 in the
 *    others.  The push of frame n uploads it once, enqueues one fldr_interlace_forward for the fields of the pair (n - 1, n) that need
 *    one and one weave for each field that lands on frame n - 1, and returns, in order, every frame whose second field was computed.
 *    With B == 1 (50p -> 25i, 59.94p -> 29.97i) no forward ever runs: the model may then be NULL, and no workspace is allocated.
 *    Contract of the stream: output frame k is, byte for byte, the weave (tests/interlace_oracle.py, the numpy statement of the table
 *    above) of outputs 2k and 2k + 1 of a fldr_rate of the same configuration with out_num doubled, pushed the same frames
 *    (tests/test_gpu_interlace.py holds the two together).  After a failed enqueue or wait the object is as after a reset.  Argument
 *    errors change nothing.  One thread drives a stream.
 *
 * Contract of fldr_interlace_weave and fldr_interlace_forward: fldr_scene_measure's.  They enqueue on `stream`; no allocation, no
 * synchronisation, no host<->device copy: they can be captured into a graph.  Every argument is validated before anything is enqueued.
 * Output bytes between a row's end and its pitch are never written.  `out` must not overlap a source.  fldr_interlace_forward: a device
 * fault flag of an earlier call is reported as the model reports it (FLDR_MODEL_E_STATUS), and no output row is then written; frames too
 * small for the model are refused with the model's code.
 *
 * Known costs and limits:
 *   - the filter is a fixed vertical one: it is not motion-adaptive, and softens still detail as much as moving detail;
 *   - the stream is synchronous: it synchronises in every push, as the rate converter does;
 *   - one weave launch per field;
 *   - fields are delivered woven only: there is no field-separated output;
 *   - 4:2:2, packed and RGB formats are out of scope;
 *   - no threshold is introduced here, so none was set on synthetic content: the scene thresholds are the rate library's.
 */
#ifndef FLDR_INTERLACE_H
#define FLDR_INTERLACE_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_INTERLACE_VERSION 100       /* major*10000 + minor*100 + patch of this header */

#define FLDR_INTERLACE_API __attribute__((visibility("default")))

#define FLDR_INTERLACE_NONE    0         /* rows copied as they are */
#define FLDR_INTERLACE_LINEAR  1         /* 1 2 1 / 4 */
#define FLDR_INTERLACE_COMPLEX 2         /* -1 2 6 2 -1 / 8, clamped */

FLDR_INTERLACE_API int         fldr_interlace_version(void);
FLDR_INTERLACE_API const char* fldr_interlace_error_string(int code);
/* 0: sizeof(fldr_interlace_io), 1: fldr_interlace_config, 2: fldr_interlace_schedule, 3: fldr_interlace_report — binding self-check;
 * FLDR_RATE_E_ARG otherwise */
FLDR_INTERLACE_API int         fldr_interlace_sizeof(int which);

/* Enqueue the weave of `out` (device planes in *fmt) from `even` and `odd` (device planes, H x W, progressive; one of them may be NULL).
 * Checked in this order: fmt / out null, both sources null, H, W, filter (FLDR_RATE_E_ARG); the format (FLDR_VIDEO_E_FORMAT); the
 * planes, then the pitches, of even, odd, out (FLDR_VIDEO_E_PLANE / FLDR_VIDEO_E_PITCH); then the frame-size limit and an `out` that
 * overlaps a source (FLDR_RATE_E_ARG). */
FLDR_INTERLACE_API int fldr_interlace_weave(int H, int W, const fldr_video_format* fmt, const fldr_video_frame* even, const fldr_video_frame* odd,
                                            int filter, const fldr_video_frame* out, void* stream);

typedef struct fldr_interlace_io {
    fldr_video_io     pair;              /* as fldr_rate_forward takes it: in[2], n_t (1 .. FLDR_RATE_MAX_OUT), t (device), in_format == out_format;
                                            pair.out[k] is the WOVEN frame that field k goes into (several k may name one frame) */
    const int32_t*    parity;            /* n_t words on the host, read during the call, 0 / 1: the rows of pair.out[k] that field k fills */
    int32_t           filter;            /* FLDR_INTERLACE_NONE / _LINEAR / _COMPLEX */
    fldr_scene_params scene_params;      /* 0, 0 = the defaults */
    int32_t           scene;             /* 0: fldr_video_forward; 1: fldr_rate_forward (measure + select on a cut) */
    int32_t           reserved[4];       /* zero */
} fldr_interlace_io;

/* fldr_rate_workspace_bytes(model, H, W, n_t) rounded up to 256, plus n_t temporary frames.  Negative on bad arguments: FLDR_RATE_E_ARG
 * for H not a multiple of 4 or n_t outside 1 .. FLDR_RATE_MAX_OUT, the video and model libraries' codes otherwise. */
FLDR_INTERLACE_API int64_t fldr_interlace_workspace_bytes(const fldr_model* model, int H, int W, int n_t);
/* *frame = temporary k (0 .. n_t - 1) of a forward with n_t outputs in the workspace ws: planes in *fmt, every pitch a multiple of 16. */
FLDR_INTERLACE_API int fldr_interlace_field_frame(const fldr_model* model, int H, int W, const fldr_video_format* fmt, int n_t, int k, void* ws,
                                                  fldr_video_frame* frame);
/* The scene state of a forward with n_t outputs in ws (it begins with the pair's fldr_scene_result when io->scene was 1); NULL on bad
 * arguments. */
FLDR_INTERLACE_API void* fldr_interlace_scene_state(const fldr_model* model, int H, int W, int n_t, void* ws);
/* Enqueue on `stream`, after all validation and nothing else: the forward of io->pair into the temporaries, then one weave per field.
 * Checked in this order: io null, H, W, n_t, t / out / parity null, filter, scene, the reserved words, every parity word, the scene
 * thresholds (FLDR_RATE_E_ARG); the formats (FLDR_VIDEO_E_FORMAT, FLDR_RATE_E_FORMAT where they differ); planes, then pitches, of
 * in[0], in[1] and every out[k]; a null model (FLDR_RATE_E_ARG); the workspace size (the model's code for a frame it does not take); ws
 * null, not 256-byte aligned or shorter than fldr_interlace_workspace_bytes, the frame-size limit, an out[k] inside ws
 * (FLDR_RATE_E_ARG). */
FLDR_INTERLACE_API int fldr_interlace_forward(const fldr_model* model, const fldr_interlace_io* io, void* ws, int64_t ws_bytes, void* stream);

/* ---- the stream: progressive host frames in, woven host frames out ------------------------------------------------------------------ */
typedef struct fldr_interlace_config {
    fldr_rate_config rate;               /* as fldr_rate_create takes it; out_num / out_den: interlaced FRAMES per second, fields come at twice that */
    int32_t          tff;                /* 1: the first field of a frame is its even rows (top field first); 0: its odd rows */
    int32_t          filter;             /* FLDR_INTERLACE_NONE / _LINEAR / _COMPLEX */
    int32_t          reserved[4];        /* zero */
} fldr_interlace_config;

typedef struct fldr_interlace_schedule { /* of output frame k; [0]: its first field in time (field 2k), [1]: its second (field 2k + 1) */
    int64_t frame;                       /* k */
    int64_t input[2];                    /* i: the field is input frame i (r == 0) or comes from the pair (i, i + 1) */
    int64_t r[2];                        /* 0 .. B - 1; t = r / B */
    int64_t B;
    int64_t push;                        /* the push (frame number n, from 0) that returns the frame: input[1] + 1; a stream that ends
                                            before it returns the frame at the flush if its first field exists by then */
    int32_t parity[2];                   /* the rows each field fills: parity[0] = tff ? 0 : 1, parity[1] = 1 - parity[0] */
    int32_t reserved[2];                 /* zero */
} fldr_interlace_schedule;

typedef struct fldr_interlace_report {   /* of one returned frame */
    int64_t  frame;                      /* k */
    int64_t  input[2];                   /* as in the schedule */
    int64_t  r[2];
    uint32_t cut[2];                     /* the field came from a pair measured as a cut: always 0 for r == 0 or scene = 0 */
    uint32_t held;                       /* 1: a flush filled the second field's rows from the last pushed frame (input[1] is that frame, r[1] = 0) */
    uint32_t reserved[3];                /* zero */
} fldr_interlace_report;

typedef struct fldr_interlace fldr_interlace;

/* Pure host arithmetic: the schedule of output frame k (0 .. 2^36) of a stream of cfg's rates and field order; H, W, format, device and
 * the scene words of cfg are not looked at.  FLDR_RATE_E_ARG on a null pointer, k out of range, tff or filter out of range or a non-zero
 * reserved word; FLDR_RATE_E_RATIO on a rate term not positive, out_num above 2^30 or a field ratio the converter does not take. */
FLDR_INTERLACE_API int  fldr_interlace_plan(const fldr_interlace_config* cfg, int64_t k, fldr_interlace_schedule* schedule);
/* Validation order: cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words,
 * thresholds, format, rate terms); then H a multiple of 4, tff, filter and the reserved words (FLDR_RATE_E_ARG); then out_num above 2^30
 * and the field ratio — it refuses exactly what fldr_rate_create refuses at the doubled rate — (FLDR_RATE_E_RATIO); then a null model
 * with B != 1 (FLDR_RATE_E_ARG): all before any device call. */
FLDR_INTERLACE_API int  fldr_interlace_create(const fldr_model* model, const fldr_interlace_config* cfg, fldr_interlace** out);
/* (ceil(B / A) + 1) / 2: the most frames one call can return; negative on a null handle */
FLDR_INTERLACE_API int  fldr_interlace_max_out(const fldr_interlace* c);
/* Frame n of the stream.  host_outs: fldr_interlace_max_out frames, of which [0 .. *n_out - 1] are written (may be NULL when no frame is
 * due); reports (may be NULL): as many entries.  Synchronises before it returns; woven frames only are downloaded, half the bytes the
 * rate converter returns at the field rate. */
FLDR_INTERLACE_API int  fldr_interlace_push(fldr_interlace* c, const fldr_video_frame* host_frame, const fldr_video_frame* host_outs, int* n_out,
                                            fldr_interlace_report* reports);
/* End of the stream: the field that lands exactly on the last pushed frame is computed, if one is due.  If a frame then has its first
 * field only, its other rows come from the last pushed frame through the same filter: the report has held = 1, and the frame is
 * returned.  At most one frame; a second flush returns none.  A stream pushed further goes on behind the fields the flush made. */
FLDR_INTERLACE_API int  fldr_interlace_flush(fldr_interlace* c, const fldr_video_frame* host_outs, int* n_out, fldr_interlace_report* reports);
/* Forget everything pushed: the next push is frame 0 of a new stream, field 0 included. */
FLDR_INTERLACE_API int  fldr_interlace_reset(fldr_interlace* c);
FLDR_INTERLACE_API void fldr_interlace_destroy(fldr_interlace* c);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_INTERLACE_H */
