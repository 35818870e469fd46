/* fldr_fps_async — fldr_fps with frames in flight: the pipe API (include/fldr_pipe.h); no Python, no device headers.
 *
 *   fldr_fps_async weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [bt601|bt709] [full] [p10] [noscd] [depth=N] < in.yuv > out.yuv
 *
 * The command line, the frames written and the lines on stderr are fldr_fps's (examples/fldr_fps.c); depth=N (1 .. 8, default 3) is
 * the number of pushed frames that may be in flight.  The program copies no frame itself: fread fills the pipe's pinned input frame
 * in place, fwrite writes from the views of the pipe's pinned output frames, and while the device works on `depth` frames the next
 * one is being read.  Device 0, the shipped configuration.  For example:
 *
 *   ffmpeg -i in.mp4 -f rawvideo -pix_fmt yuv420p - | fldr_fps_async weights.npz 1920 1080 24000/1001 60 depth=4 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 60 -i - out.mp4 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_pipe.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [bt601|bt709] [full] [p10] [noscd] [depth=N] < in.yuv > out.yuv"
                    "  (raw I420 frames; p10: yuv420p10le; rates like 24, 60 or 24000/1001; depth 1 .. 8)\n", prog);
}

/* "24000/1001" or "60" -> num, den; 0 when it is neither */
static int parse_rate(const char* s, int32_t* num, int32_t* den) {
    char* end;
    long n = strtol(s, &end, 10), d = 1;
    if (end == s) return 0;
    if (*end == '/') {
        const char* q = end + 1;
        d = strtol(q, &end, 10);
        if (end == q) return 0;
    }
    if (*end || n < 1 || d < 1 || n > 0x7fffffffL || d > 0x7fffffffL) return 0;
    *num = (int32_t)n;
    *den = (int32_t)d;
    return 1;
}

typedef struct counters {
    long received, cuts, written;      /* push jobs received (the frame number of the next one), cuts seen, frames written */
} counters;

/* Receive the oldest job and write its frames: a packed I420 frame is fsize bytes from plane[0] on.  push: the job is a frame's, not
 * the flush's.  0, or 1 after an error (reported). */
static int receive_one(fldr_pipe* p, fldr_video_frame* views, size_t fsize, int push, counters* c) {
    fldr_scene_result scene;
    int k, n_out;
    int rc = fldr_pipe_receive_view(p, views, &n_out, &scene);
    if (rc) { fprintf(stderr, "fldr_pipe_receive_view: %s (%d)\n", fldr_pipe_error_string(rc), rc); return 1; }
    if (push) {
        if (scene.cut) { fprintf(stderr, "cut at frame %ld\n", c->received); ++c->cuts; }
        ++c->received;
    }
    for (k = 0; k < n_out; ++k)
        if (fwrite(views[k].plane[0], fsize, 1, stdout) != 1) return 1;
    c->written += n_out;
    return 0;
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_pipe_config cfg;
    fldr_model* model = NULL;
    fldr_pipe* p = NULL;
    fldr_video_frame in, *views;
    counters c = { 0, 0, 0 };
    int W, H, rc, k, status = 0, bps = 1;
    long n = 0;
    size_t fsize;
    if (argc < 6 || argc > 11) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    if (W < 2 || H < 2 || !parse_rate(argv[4], &cfg.rate.in_num, &cfg.rate.in_den) || !parse_rate(argv[5], &cfg.rate.out_num, &cfg.rate.out_den)) {
        usage(argv[0]);
        return 2;
    }
    cfg.rate.H = H; cfg.rate.W = W;
    cfg.rate.format.layout = FLDR_VIDEO_I420;
    cfg.rate.format.matrix = FLDR_VIDEO_BT709;
    cfg.rate.format.range = FLDR_VIDEO_LIMITED;
    cfg.rate.scene = 1;                                /* scene_params 0, 0: the header's defaults */
    cfg.depth = 3;
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.rate.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.rate.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.rate.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.rate.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "noscd")) cfg.rate.scene = 0;
        else if (!strncmp(argv[k], "depth=", 6) && atoi(argv[k] + 6) >= 1 && atoi(argv[k] + 6) <= FLDR_PIPE_MAX_DEPTH) cfg.depth = atoi(argv[k] + 6);
        else { usage(argv[0]); return 2; }
    }
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_pipe_create(model, &cfg, &p);
    if (rc) { fprintf(stderr, "fldr_pipe_create: %s (%d)\n", fldr_pipe_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps;
    views = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)fldr_pipe_max_out(p));
    if (!views) { fprintf(stderr, "out of memory\n"); return 1; }
    for (;;) {
        /* the pinned frame the next submit takes: Y, U and V one behind the other, as in the file */
        rc = fldr_pipe_input(p, &in);
        if (rc) { fprintf(stderr, "fldr_pipe_input: %s (%d)\n", fldr_pipe_error_string(rc), rc); status = 1; break; }
        if (fread(in.plane[0], 1, fsize, stdin) != fsize) break;
        if (fldr_pipe_pending(p) == cfg.depth && receive_one(p, views, fsize, 1, &c)) { status = 1; break; }
        rc = fldr_pipe_submit(p, NULL);
        if (rc) { fprintf(stderr, "fldr_pipe_submit: %s (%d)\n", fldr_pipe_error_string(rc), rc); status = 1; break; }
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    while (!status && fldr_pipe_pending(p) > 0) status = receive_one(p, views, fsize, 1, &c);
    if (!status) {
        rc = fldr_pipe_flush(p);
        if (rc) { fprintf(stderr, "fldr_pipe_flush: %s (%d)\n", fldr_pipe_error_string(rc), rc); status = 1; }
        else status = receive_one(p, views, fsize, 0, &c);
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld frames out, %ld cuts\n", n, c.written, c.cuts);
    fldr_pipe_destroy(p);
    fldr_model_destroy(model);
    free(views);
    return status;
}
