/* fldr_slowmo — slow motion on raw I420 video with the video API (include/fldr_video.h); no Python, no HIP headers.
 *
 *   fldr_slowmo weights.npz W H FACTOR [bt601|bt709] [full] [p10] < in.yuv > out.yuv
 *
 * in.yuv / out.yuv: raw 8-bit I420 frames (ffmpeg -f rawvideo -pix_fmt yuv420p), W x H; with `p10`, raw 10-bit frames in 16-bit
 * little-endian words (ffmpeg -pix_fmt yuv420p10le) in and out, interpolated at 10 bits.  The output is the first frame, then for every
 * further frame FACTOR - 1 interpolated frames (at t = k / FACTOR) followed by the frame itself, byte for byte.  Colour: BT.709
 * limited range unless told otherwise.  Device 0, the shipped configuration.  For example:
 *
 *   ffmpeg -i in.mp4 -f rawvideo -pix_fmt yuv420p - | fldr_slowmo weights.npz 1920 1080 4 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 120 -i - out.mp4
 *
 *   ffmpeg -i in10.mkv -f rawvideo -pix_fmt yuv420p10le - | fldr_slowmo weights.npz 3840 2160 2 p10 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p10le -s 3840x2160 -r 120 -i - -c:v libx265 -pix_fmt yuv420p10le out10.mkv */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_video.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H FACTOR [bt601|bt709] [full] [p10] < in.yuv > out.yuv  (raw I420 frames; p10: yuv420p10le; FACTOR >= 2)\n", prog);
}

/* the three planes of one packed I420 frame in buf; bps: bytes per sample (1, or 2 for yuv420p10le) */
static fldr_video_frame i420(uint8_t* buf, int W, int H, int bps) {
    fldr_video_frame f;
    const int64_t cw = (W + 1) / 2, ch = (H + 1) / 2;
    memset(&f, 0, sizeof(f));
    f.plane[0] = buf;
    f.plane[1] = buf + (int64_t)W * H * bps;
    f.plane[2] = buf + ((int64_t)W * H + cw * ch) * bps;
    f.pitch[0] = (int64_t)W * bps;
    f.pitch[1] = f.pitch[2] = cw * bps;
    return f;
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_video_session_config cfg;
    fldr_model* model = NULL;
    fldr_video_session* s = NULL;
    fldr_video_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, factor, n_t, rc, k, n_out, first = 1, status = 0, bps = 1;
    size_t fsize;
    if (argc < 5 || argc > 8) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    factor = atoi(argv[4]);
    if (W < 2 || H < 2 || factor < 2) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    cfg.in_format.layout = cfg.out_format.layout = FLDR_VIDEO_I420;
    cfg.in_format.matrix = FLDR_VIDEO_BT709;
    cfg.in_format.range = FLDR_VIDEO_LIMITED;
    for (k = 5; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.in_format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.in_format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.in_format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.in_format.depth = 10; bps = 2; }
        else { usage(argv[0]); return 2; }
    }
    cfg.out_format = cfg.in_format;
    n_t = factor - 1;
    cfg.n_t = n_t;                                     /* t = NULL: k / FACTOR, k = 1 .. FACTOR - 1 */
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)n_t);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)n_t);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < n_t; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_video_session_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_video_session_create: %s (%d)\n", fldr_video_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_video_session_push(s, &in, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_video_session_push: %s (%d)\n", fldr_video_error_string(rc), rc); status = 1; break; }
        if (!first && n_out != n_t) { fprintf(stderr, "unexpected output count %d\n", n_out); status = 1; break; }
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        if (fwrite(frame, 1, fsize, stdout) != fsize) { status = 1; break; }
        first = 0;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (fflush(stdout)) status = 1;
    fldr_video_session_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
