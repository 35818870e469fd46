/*
 * fldr_pipe.h — pipe API of libfldr_pipe.so: the rate converter of include/fldr_rate.h with several pushed frames in flight, and
 * with host copies the caller may skip.
 *
 * Plain C99; no HIP header is needed.  The library calls no fldr_* function but those of fldr_rate.h, fldr_video.h and fldr_model.h,
 * launches no kernel of its own and changes nothing below it: the device work of a job is fldr_rate_forward (scene = 1, a pair with an
 * interpolated output), fldr_video_forward (scene = 0), fldr_scene_measure (scene = 1, a pair without one) or nothing, exactly what
 * fldr_rate_push enqueues for the same frame.
 *
 * fldr_rate_push uploads, computes, downloads and synchronises inside one call.  A pipe splits the call in two.  fldr_pipe_submit
 * enqueues one job and returns; fldr_pipe_receive waits for the oldest job and hands out its frames.  Up to `depth` jobs may be
 * outstanding (submitted, not yet received), so the upload of frame n + 1 and the download of job n - 1 run beside the forward of job n.
 *
 * Contract:
 *   1. One job per call, received in order.  Every fldr_pipe_submit and every fldr_pipe_flush creates exactly one job.  The k-th job
 *      received returns byte for byte what the k-th call of the same sequence of fldr_rate_push / fldr_rate_flush calls returns on a
 *      fldr_rate created with cfg.rate: the frames, n_out (0 for the first frame) and the fldr_scene_result — at every depth and for
 *      every interleaving of submit and receive.  (Which output j belongs to which push at which r is fldr_rate.h's rule; this
 *      library states it a second time and tests/test_gpu_pipe.py holds the two together.)
 *   2. Submit does not wait for the device.  It returns after the host copy (if any) and the enqueue; the caller's host_frame may then
 *      be overwritten.  With `depth` jobs outstanding it returns FLDR_PIPE_E_FULL and changes nothing.
 *   3. Receive waits for one job only: on that job's event, never with a stream or device synchronisation that would wait for
 *      younger jobs too.  With nothing outstanding it returns FLDR_PIPE_E_EMPTY.
 *   4. A view (fldr_pipe_receive_view) stays valid until the next fldr_pipe_receive, fldr_pipe_receive_view, fldr_pipe_reset or
 *      fldr_pipe_destroy on the pipe, whatever is submitted in between — and whatever is written into fldr_pipe_input's frame.
 *   5. fldr_pipe_reset waits for everything enqueued, drops all outstanding jobs and their outputs and starts a new stream: the next
 *      submit is frame 0.
 *   6. After any non-zero return of an enqueue or a wait the pipe waits for its streams, drops all jobs and is as after a reset; the
 *      code goes to the call that saw it.  A device fault flag comes back as the model reports it (FLDR_MODEL_E_STATUS).  Argument
 *      errors (a null pointer, a bad frame) change nothing.
 *   7. One thread drives a pipe.  The library starts no threads.
 *
 * What a pipe owns (F = the packed frame rounded up to 256 bytes, M = fldr_pipe_max_out, D = depth):
 *   streams  three, non-blocking: upload, compute, download; linked by events without timing (end of upload -> the job's compute, end
 *            of compute -> the job's download, end of download -> receive).  The compute stream runs the jobs one after another, so one
 *            workspace and one scene state serve them all; the 32-byte scene result is copied to the job's pinned slot on the compute
 *            stream right behind the job's work.  No graph capture.
 *   device   (D + 1) F  input frames, a ring by frame number.  Frame n lands on the slot of frame n - D - 1, read last by the job of
 *                       frame n - D, which has been received — so completed — before `depth` allows this submit.
 *            D M F      output sets, a ring by job number: job k writes where job k - D, received by now, was downloaded from.
 *            D x 256    t arrays, one per outstanding job (fldr_rate rewrites one array per push; with jobs queued that would race).
 *            4096       scene state for pairs that run the measure alone, and fldr_rate_workspace_bytes(model, H, W, M) of workspace.
 *   pinned   (D + 3) F  input frames, a ring by frame number.  While the view of the job of frame n is held, frame n - 1 (the bytes of
 *                       its r == 0 outputs, and of a flush) must survive; D - 1 younger jobs may be outstanding (frames up to
 *                       n + D - 1), one more may be submitted (n + D), and fldr_pipe_input's frame (n + D + 1) may be filled before
 *                       the next receive: D + 3 frames.
 *            (D + 1) M F output sets, a ring by job number: the viewed job's set and those of the D jobs that may follow it.
 *            D x 256    t arrays, D x 256 scene results.
 *   At 3840 x 2160 NV12 (F = 12.4 MB), 24 -> 60 (M = 3), D = 4: 211 MB of device memory beside the 2.4 GB workspace, 273 MB pinned.
 *
 * Every function returns 0, a negative FLDR_PIPE_E_* code, a negative FLDR_RATE_E_*, FLDR_VIDEO_E_* or FLDR_MODEL_E_* code passed
 * through, or a positive hipError_t from the runtime.
 */
#ifndef FLDR_PIPE_H
#define FLDR_PIPE_H

#include <stdint.h>

#include "fldr_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLDR_PIPE_VERSION 100            /* major*10000 + minor*100 + patch of this header */

/* codes of this library: -500 and below, apart from the ranges of the libraries below it (-1 .. -299) */
#define FLDR_PIPE_E_ARG         (-500)   /* null pointer, depth outside 1 .. FLDR_PIPE_MAX_DEPTH, non-zero reserved word, null model */
#define FLDR_PIPE_E_FULL        (-501)   /* submit / flush: `depth` jobs are outstanding; nothing changed */
#define FLDR_PIPE_E_EMPTY       (-502)   /* receive: no job is outstanding */
#define FLDR_PIPE_E_DEVICE      (-503)   /* no such device, or an allocation failed */

#define FLDR_PIPE_API __attribute__((visibility("default")))

#define FLDR_PIPE_MAX_DEPTH     8

typedef struct fldr_pipe_config {
    fldr_rate_config rate;               /* exactly what fldr_rate_create takes */
    int32_t          depth;              /* 1 .. 8: jobs that may be outstanding (submitted, not yet received) */
    int32_t          reserved[3];        /* zero */
} fldr_pipe_config;

typedef struct fldr_pipe fldr_pipe;

FLDR_PIPE_API int         fldr_pipe_version(void);
FLDR_PIPE_API const char* fldr_pipe_error_string(int code);
/* 0: sizeof(fldr_pipe_config) — binding self-check; FLDR_PIPE_E_ARG otherwise */
FLDR_PIPE_API int         fldr_pipe_sizeof(int which);

/* cfg->rate is checked in fldr_rate_create's order and refused with its codes (size / device / scene, reserved words, thresholds,
 * format, ratio), then depth and the reserved words (FLDR_PIPE_E_ARG), then a null model (FLDR_PIPE_E_ARG): all before any device
 * call. */
FLDR_PIPE_API int  fldr_pipe_create(const fldr_model* model, const fldr_pipe_config* cfg, fldr_pipe** out);
/* as fldr_rate_max_out: the most frames one job can return; negative on a null handle */
FLDR_PIPE_API int  fldr_pipe_max_out(const fldr_pipe* p);
/* jobs outstanding, 0 .. depth; negative on a null handle */
FLDR_PIPE_API int  fldr_pipe_pending(const fldr_pipe* p);
/* *frame: the pinned, packed frame (pitch = row bytes, planes one behind the other) that the next submit takes: fill it in place and
 * submit NULL.  The same frame until a submit succeeds; writing it disturbs neither a job in flight nor a view. */
FLDR_PIPE_API int  fldr_pipe_input(fldr_pipe* p, fldr_video_frame* frame);
/* Frame n of the stream.  host_frame != NULL: its planes (any pitches) are copied into fldr_pipe_input's frame first; NULL: that frame
 * is taken as filled.  Enqueues the upload and the work of the pair (n - 1, n) and returns. */
FLDR_PIPE_API int  fldr_pipe_submit(fldr_pipe* p, const fldr_video_frame* host_frame);
/* Wait for the OLDEST job and copy its *n_out frames into host_outs[0 .. *n_out - 1] (fldr_pipe_max_out frames; may be NULL when the
 * job has no output: the call then fails with FLDR_PIPE_E_ARG, and leaves the job where it is, only if it has one).  *scene (may be
 * NULL): as fldr_rate_push fills it; all zero for a flush job. */
FLDR_PIPE_API int  fldr_pipe_receive(fldr_pipe* p, const fldr_video_frame* host_outs, int* n_out, fldr_scene_result* scene);
/* The same without the copy: views[0 .. *n_out - 1] (an array of fldr_pipe_max_out frames, written by the call) point into the pipe's
 * pinned memory, packed as fldr_pipe_input's frame. */
FLDR_PIPE_API int  fldr_pipe_receive_view(fldr_pipe* p, fldr_video_frame* views, int* n_out, fldr_scene_result* scene);
/* The end-of-stream job: what fldr_rate_flush returns at this point of the stream (one frame or none), received like any job.  A
 * submit after it goes on as a fldr_rate_push after a fldr_rate_flush does. */
FLDR_PIPE_API int  fldr_pipe_flush(fldr_pipe* p);
FLDR_PIPE_API int  fldr_pipe_reset(fldr_pipe* p);
FLDR_PIPE_API void fldr_pipe_destroy(fldr_pipe* p);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_PIPE_H */
