/* fldr_scale — frame-rate AND size conversion of raw I420 video with the scale API (include/fldr_scale.h); no Python, no device headers.
 * It is fldr_fps with an output size: the resize runs on the device, on whichever side of the interpolation is cheaper.
 *
 *   fldr_scale weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN out=WxH [filter=bilinear|bicubic|lanczos] [where=auto|before|after]
 *              [bt601|bt709] [full] [p10] [noscd] < in.yuv > out.yuv
 *
 * in.yuv: raw 8-bit I420 frames (ffmpeg -f rawvideo -pix_fmt yuv420p), W x H; out.yuv: the same at the size of out=; with `p10`, raw
 * 10-bit frames in 16-bit little-endian words (ffmpeg -pix_fmt yuv420p10le) in and out.  A rate is NUM/DEN or a plain integer.  Output
 * frame j is the input at position j x (in rate / out rate), as fldr_fps makes it, scaled: where=before scales every input frame once and
 * interpolates at the output size, where=after interpolates at the input size and scales every output, where=auto (the default) picks
 * the one that runs the model on fewer pixels.  filter defaults to lanczos.  With equal rates nothing is interpolated and the weights may
 * be given as - : a pure scaler.  The frame numbers of the detected cuts go to stderr (`noscd` turns the detector off).  Colour: BT.709
 * limited range unless told otherwise; it only names the format, scaling is done on code values.  Device 0.  For example, 1080p24 to
 * 2160p60:
 *
 *   ffmpeg -i in.mp4 -f rawvideo -pix_fmt yuv420p - | fldr_scale weights.npz 1920 1080 24 60 out=3840x2160 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 3840x2160 -r 60 -i - out.mp4 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_scale.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN out=WxH [filter=bilinear|bicubic|lanczos] [where=auto|before|after]"
                    " [bt601|bt709] [full] [p10] [noscd] < in.yuv > out.yuv"
                    "  (raw I420 frames; p10: yuv420p10le; rates like 24, 60 or 24000/1001; W, H 2 .. %d as the rate converter asks, out= 1 .. %d, at most %d taps per axis;"
                    " weights.npz may be - when the rates are equal)\n", prog, FLDR_SCALE_MAX_SIZE, FLDR_SCALE_MAX_SIZE, FLDR_SCALE_MAX_TAPS);
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

/* "3840x2160" -> W, H; 0 when it is not two sizes */
static int parse_size(const char* s, int32_t* W, int32_t* H) {
    char* end;
    long w = strtol(s, &end, 10), h;
    const char* q;
    if (end == s || *end != 'x') return 0;
    q = end + 1;
    h = strtol(q, &end, 10);
    if (end == q || *end || w < 1 || h < 1 || w > FLDR_SCALE_MAX_SIZE || h > FLDR_SCALE_MAX_SIZE) return 0;
    *W = (int32_t)w;
    *H = (int32_t)h;
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
    fldr_scale_config cfg;
    fldr_scene_result scene;
    fldr_model* model = NULL;
    fldr_scale* s = NULL;
    fldr_video_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, max_out, status = 0, bps = 1, have_out = 0, equal_rates;
    long n = 0, cuts = 0, written = 0;
    size_t isize, osize;
    if (argc < 7 || argc > 13) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    if (W < 2 || H < 2 || W > FLDR_SCALE_MAX_SIZE || H > FLDR_SCALE_MAX_SIZE || !parse_rate(argv[4], &cfg.rate.in_num, &cfg.rate.in_den) ||
        !parse_rate(argv[5], &cfg.rate.out_num, &cfg.rate.out_den)) {
        usage(argv[0]);
        return 2;
    }
    cfg.rate.H = H; cfg.rate.W = W;
    cfg.rate.format.layout = FLDR_VIDEO_I420;
    cfg.rate.format.matrix = FLDR_VIDEO_BT709;
    cfg.rate.format.range = FLDR_VIDEO_LIMITED;
    cfg.rate.scene = 1;                                /* scene_params 0, 0: the header's defaults */
    cfg.filter = FLDR_SCALE_LANCZOS3;
    cfg.where = FLDR_SCALE_AUTO;
    for (k = 6; k < argc; ++k) {
        const char* a = argv[k];
        if (!strncmp(a, "out=", 4)) { if (!parse_size(a + 4, &cfg.out_W, &cfg.out_H)) { usage(argv[0]); return 2; } have_out = 1; }
        else if (!strcmp(a, "filter=bilinear")) cfg.filter = FLDR_SCALE_BILINEAR;
        else if (!strcmp(a, "filter=bicubic")) cfg.filter = FLDR_SCALE_BICUBIC;
        else if (!strcmp(a, "filter=lanczos")) cfg.filter = FLDR_SCALE_LANCZOS3;
        else if (!strcmp(a, "where=auto")) cfg.where = FLDR_SCALE_AUTO;
        else if (!strcmp(a, "where=before")) cfg.where = FLDR_SCALE_BEFORE;
        else if (!strcmp(a, "where=after")) cfg.where = FLDR_SCALE_AFTER;
        else if (!strcmp(a, "bt601")) cfg.rate.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(a, "bt709")) cfg.rate.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(a, "full")) cfg.rate.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(a, "p10")) { cfg.rate.format.depth = 10; bps = 2; }
        else if (!strcmp(a, "noscd")) cfg.rate.scene = 0;
        else { usage(argv[0]); return 2; }
    }
    equal_rates = (int64_t)cfg.rate.in_num * cfg.rate.out_den == (int64_t)cfg.rate.out_num * cfg.rate.in_den;
    /* the table builder is host arithmetic: a ratio beyond the tap limit is a bad command line, found before any device is touched */
    if (!have_out || fldr_scale_taps_count(W, cfg.out_W, cfg.filter) < 0 || fldr_scale_taps_count(H, cfg.out_H, cfg.filter) < 0 ||
        (!strcmp(argv[1], "-") && !equal_rates)) {
        usage(argv[0]);
        return 2;
    }
    if (strcmp(argv[1], "-")) {
        memset(&mcfg, 0, sizeof(mcfg));
        rc = fldr_model_create_npz(argv[1], &mcfg, &model);
        if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    }
    rc = fldr_scale_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_scale_create: %s (%d)\n", fldr_scale_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    fprintf(stderr, "scaling %s the interpolation\n", cfg.where == FLDR_SCALE_BEFORE ? "before" : "after");
    max_out = fldr_scale_max_out(s);
    isize = frame_size(W, H, bps);
    osize = frame_size(cfg.out_W, cfg.out_H, bps);
    frame = (uint8_t*)malloc(isize);
    obuf = (uint8_t*)malloc(osize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)max_out);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + osize * (size_t)k, cfg.out_W, cfg.out_H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, isize, stdin) == isize) {
        rc = fldr_scale_push(s, &in, outs, &n_out, &scene);
        if (rc) { fprintf(stderr, "fldr_scale_push: %s (%d)\n", fldr_scale_error_string(rc), rc); status = 1; break; }
        if (scene.cut) { fprintf(stderr, "cut at frame %ld\n", n); ++cuts; }
        if (n_out > 0 && fwrite(obuf, osize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_scale_flush(s, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_scale_flush: %s (%d)\n", fldr_scale_error_string(rc), rc); status = 1; }
        else if (n_out > 0 && fwrite(obuf, osize, (size_t)n_out, stdout) != (size_t)n_out) status = 1;
        else written += n_out;
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld frames out, %ld cuts\n", n, written, cuts);
    fldr_scale_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
