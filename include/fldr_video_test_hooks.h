/* Converter hooks of libfldr_video_test.so (the build of libfldr_video.so's sources with -DFLDR_TEST_HOOKS; `make -C fldr-vfi_amd/video`
 * builds it beside the product).  NOT part of the video API: the product library libfldr_video.so exports none of these.  They run the
 * product's own converter kernels alone — no model, no workspace — so that tests/ can hand them any frame (tests/test_gpu_video_convert.py,
 * through fldr_video.test_hooks()).  Plain C99, like fldr_video.h.
 *
 * Both converters validate as fldr_video_forward validates a format and a frame (H, W >= 2, the format's enums, depth and reserved words,
 * null / odd plane pointers, short / odd pitches) and return its codes, before anything is enqueued.  The planar side must be 256-byte
 * aligned, as the workspace of a forward guarantees (the 8-bit kernels rely on it for their dword accesses): FLDR_VIDEO_E_ARG otherwise.
 * They enqueue one kernel on `stream` (NULL = the null stream) and do not synchronise. */
#ifndef FLDR_VIDEO_TEST_HOOKS_H
#define FLDR_VIDEO_TEST_HOOKS_H
#include "fldr_video.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Two device frames in `format` -> the planar BGR pair [2,3,H,W] at `pair` (device; uint8, or uint16 code values 0 .. 1023 at depth 10):
 * the input conversion of a forward (yuv420_to_planar_pair / yuv420_to_planar_pair10). */
FLDR_VIDEO_API int fldr_video_debug_to_planar(const fldr_video_frame in[2], const fldr_video_format* format, void* pair, int H, int W, void* stream);
/* One planar BGR frame [3,H,W] at `planar` (device; uint8, or uint16 code values 0 .. 1023 at depth 10) -> the device frame `out_frame` in
 * `format`: the output conversion of a forward (planar_to_yuv420 / planar_to_yuv420_10).  Bytes between a row's end and its pitch are not
 * written. */
FLDR_VIDEO_API int fldr_video_debug_from_planar(const void* planar, const fldr_video_frame* out_frame, const fldr_video_format* format, int H, int W, void* stream);
/* The form the most recent converter launch of this process took: 1 the wide-access form (W % 4 == 0 and every plane pointer and pitch
 * 4-byte aligned at depth 8, 8-byte aligned at depth 10), 0 the per-sample form, -1 when nothing has been launched yet. */
FLDR_VIDEO_API int fldr_video_debug_last_path(void);

#ifdef __cplusplus
}
#endif
#endif /* FLDR_VIDEO_TEST_HOOKS_H */
