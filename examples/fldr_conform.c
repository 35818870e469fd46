/* fldr_conform — frame-rate AND format conversion of raw I420 video with the conform API (include/fldr_conform.h); no Python, no device
 * headers.  It is fldr_fps with an output format and a canvas: the conversion from the input's matrix, range and depth to the output's
 * runs on the device, directly on the YUV samples, and the picture can sit on a larger black canvas (pillarbox, letterbox).
 *
 *   fldr_conform weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [bt601|bt709] [full] [p10] [noscd] [out=WxH] [at=X,Y] [to=bt601|bt709]
 *                [tofull|tolimited] [to8|to10] [dither] < in.yuv > out.yuv
 *
 * in.yuv: raw 8-bit I420 frames (ffmpeg -f rawvideo -pix_fmt yuv420p), W x H, or with `p10` raw 10-bit frames in 16-bit little-endian
 * words (ffmpeg -pix_fmt yuv420p10le); bt601 | bt709 and `full` name the input's matrix and range (BT.709 limited unless told
 * otherwise).  out.yuv: raw I420 frames of the size of out= (the input's size by default) with the picture's top-left sample at at=
 * (even numbers; 0,0 by default) and black elsewhere, in the matrix of to=, the range of tofull | tolimited and the depth of to8 | to10,
 * each the input's unless given.  `dither` turns the ordered dither on (it matters where the depth or the range shrinks).  A rate is
 * NUM/DEN or a plain integer.  Output frame j is the input at position j x (in rate / out rate), as fldr_fps makes it, conformed.  With
 * equal rates nothing is interpolated and the weights may be given as - : a pure converter.  The frame numbers of the detected cuts go to
 * stderr (`noscd` turns the detector off).  Device 0.  For example, 4:3 SD material in BT.601 to a 10-bit BT.709 frame with bars:
 *
 *   ffmpeg -i in.mpg -f rawvideo -pix_fmt yuv420p - | fldr_conform - 768 576 25 25 bt601 out=1024x576 at=128,0 to=bt709 to10 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p10le -s 1024x576 -r 25 -i - out.mov */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_conform.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [bt601|bt709] [full] [p10] [noscd] [out=WxH] [at=X,Y] [to=bt601|bt709]"
                    " [tofull|tolimited] [to8|to10] [dither] < in.yuv > out.yuv"
                    "  (raw I420 frames; p10 / to10: yuv420p10le; rates like 24, 60 or 24000/1001; W, H 2 .. %d as the rate converter asks, out= 1 .. %d;"
                    " at= even, and the picture must fit the canvas; weights.npz may be - when the rates are equal)\n",
            prog, FLDR_CONFORM_MAX_SIZE, FLDR_CONFORM_MAX_SIZE);
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

/* "1024x576" (sep 'x') or "128,0" (sep ','): two numbers lo .. FLDR_CONFORM_MAX_SIZE -> a, b; 0 when it is not that */
static int parse_two(const char* s, char sep, long lo, int32_t* a, int32_t* b) {
    char* end;
    long v = strtol(s, &end, 10), w;
    const char* q;
    if (end == s || *end != sep) return 0;
    q = end + 1;
    w = strtol(q, &end, 10);
    if (end == q || *end || v < lo || w < lo || v > FLDR_CONFORM_MAX_SIZE || w > FLDR_CONFORM_MAX_SIZE) return 0;
    *a = (int32_t)v;
    *b = (int32_t)w;
    return 1;
}

static size_t frame_size(int W, int H, int bps) { return ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps; }

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
    fldr_conform_stream_config cfg;
    fldr_scene_result scene;
    fldr_model* model = NULL;
    fldr_conform* s = NULL;
    fldr_video_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, max_out, status = 0, ibps, obps, equal_rates;
    int to_matrix = -1, to_range = -1, to_depth = -1, have_out = 0;
    long n = 0, cuts = 0, written = 0;
    size_t isize, osize;
    if (argc < 6 || argc > 16) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    if (W < 2 || H < 2 || W > FLDR_CONFORM_MAX_SIZE || H > FLDR_CONFORM_MAX_SIZE || !parse_rate(argv[4], &cfg.rate.in_num, &cfg.rate.in_den) ||
        !parse_rate(argv[5], &cfg.rate.out_num, &cfg.rate.out_den)) {
        usage(argv[0]);
        return 2;
    }
    cfg.rate.H = H; cfg.rate.W = W;
    cfg.rate.format.layout = FLDR_VIDEO_I420;
    cfg.rate.format.matrix = FLDR_VIDEO_BT709;
    cfg.rate.format.range = FLDR_VIDEO_LIMITED;
    cfg.rate.format.depth = 8;
    cfg.rate.scene = 1;                                /* scene_params 0, 0: the header's defaults */
    for (k = 6; k < argc; ++k) {
        const char* a = argv[k];
        if (!strcmp(a, "bt601")) cfg.rate.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(a, "bt709")) cfg.rate.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(a, "full")) cfg.rate.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(a, "p10")) cfg.rate.format.depth = 10;
        else if (!strcmp(a, "noscd")) cfg.rate.scene = 0;
        else if (!strncmp(a, "out=", 4)) { if (!parse_two(a + 4, 'x', 1, &cfg.out_W, &cfg.out_H)) { usage(argv[0]); return 2; } have_out = 1; }
        else if (!strncmp(a, "at=", 3)) { if (!parse_two(a + 3, ',', 0, &cfg.dst_x, &cfg.dst_y)) { usage(argv[0]); return 2; } }
        else if (!strcmp(a, "to=bt601")) to_matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(a, "to=bt709")) to_matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(a, "tofull")) to_range = FLDR_VIDEO_FULL;
        else if (!strcmp(a, "tolimited")) to_range = FLDR_VIDEO_LIMITED;
        else if (!strcmp(a, "to8")) to_depth = 8;
        else if (!strcmp(a, "to10")) to_depth = 10;
        else if (!strcmp(a, "dither")) cfg.dither = FLDR_CONFORM_DITHER_ORDERED;
        else { usage(argv[0]); return 2; }
    }
    if (!have_out) { cfg.out_W = W; cfg.out_H = H; }
    cfg.out_format = cfg.rate.format;
    if (to_matrix >= 0) cfg.out_format.matrix = to_matrix;
    if (to_range >= 0) cfg.out_format.range = to_range;
    if (to_depth >= 0) cfg.out_format.depth = to_depth;
    equal_rates = (int64_t)cfg.rate.in_num * cfg.rate.out_den == (int64_t)cfg.rate.out_num * cfg.rate.in_den;
    /* the placement is host arithmetic: a picture that does not fit is a bad command line, found before any device is touched */
    if ((cfg.dst_x & 1) || (cfg.dst_y & 1) || cfg.dst_x > cfg.out_W - W || cfg.dst_y > cfg.out_H - H || (!strcmp(argv[1], "-") && !equal_rates)) {
        usage(argv[0]);
        return 2;
    }
    ibps = cfg.rate.format.depth == 10 ? 2 : 1;
    obps = cfg.out_format.depth == 10 ? 2 : 1;
    if (strcmp(argv[1], "-")) {
        memset(&mcfg, 0, sizeof(mcfg));
        rc = fldr_model_create_npz(argv[1], &mcfg, &model);
        if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    }
    rc = fldr_conform_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_conform_create: %s (%d)\n", fldr_conform_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    max_out = fldr_conform_max_out(s);
    isize = frame_size(W, H, ibps);
    osize = frame_size(cfg.out_W, cfg.out_H, obps);
    frame = (uint8_t*)malloc(isize);
    obuf = (uint8_t*)malloc(osize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)max_out);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + osize * (size_t)k, cfg.out_W, cfg.out_H, obps);
    in = i420(frame, W, H, ibps);
    while (fread(frame, 1, isize, stdin) == isize) {
        rc = fldr_conform_push(s, &in, outs, &n_out, &scene);
        if (rc) { fprintf(stderr, "fldr_conform_push: %s (%d)\n", fldr_conform_error_string(rc), rc); status = 1; break; }
        if (scene.cut) { fprintf(stderr, "cut at frame %ld\n", n); ++cuts; }
        if (n_out > 0 && fwrite(obuf, osize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_conform_flush(s, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_conform_flush: %s (%d)\n", fldr_conform_error_string(rc), rc); status = 1; }
        else if (n_out > 0 && fwrite(obuf, osize, (size_t)n_out, stdout) != (size_t)n_out) status = 1;
        else written += n_out;
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld frames out, %ld cuts\n", n, written, cuts);
    fldr_conform_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
