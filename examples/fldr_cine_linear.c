/* fldr_cine_linear — fldr_cine with the exposure integrated in linear light (include/fldr_light.h): motion-blurred frame-rate
 * down-conversion of raw I420 video; no Python, no device headers.
 *
 *   fldr_cine_linear weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [gamma|pq|hlg] [angle=180] [sub=4] [bt601|bt709] [full] [p10] [noscd]
 *       < in.yuv > out.yuv
 *
 * gamma (the default): BT.1886, L = V^2.4, for SDR video; pq: SMPTE ST 2084; hlg: BT.2100 HLG.  Every sample goes through the curve
 * before the frames of an exposure are averaged and back through it afterwards, so a moving highlight keeps the brightness and the
 * width a real exposure gives it; an exposure holds at most 255 points.  Everything else is fldr_cine's:
 *
 * in.yuv / out.yuv: raw 8-bit I420 frames (ffmpeg -f rawvideo -pix_fmt yuv420p), W x H; with `p10`, raw 10-bit frames in 16-bit
 * little-endian words (ffmpeg -pix_fmt yuv420p10le) in and out.  A rate is NUM/DEN or a plain integer (24, 120, 60000/1001).  Output
 * frame j is the average of what the source shows during its exposure: the input frames, and `sub` - 1 interpolated frames between
 * each two of them, that fall into [j, j + angle / 360) output intervals.  angle: the shutter angle in whole degrees, 1 .. 360 (180 is
 * the cinema default; 360 exposes the whole output interval).  No output mixes two scenes (`noscd` turns the cut detector off).  One
 * line per output frame goes to stderr: its number, how many points were averaged, how many of them were interpolated, and whether a
 * cut or the end of the stream shortened its exposure.  Colour: BT.709 limited range unless told otherwise.  Device 0, the shipped
 * configuration.  For example:
 *
 *   ffmpeg -i in120.mp4 -f rawvideo -pix_fmt yuv420p - | fldr_cine_linear weights.npz 1920 1080 120 24 gamma angle=180 sub=1 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 24 -i - out.mp4 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_light.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN [gamma|pq|hlg] [angle=180] [sub=4] [bt601|bt709] [full] [p10] [noscd]"
                    " < in.yuv > out.yuv  (raw I420 frames; p10: yuv420p10le; rates like 24, 120 or 60000/1001; angle 1 .. 360; sub 1 .. 64)\n",
            prog);
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

/* "name=123" -> the number when it lies in lo .. hi; -1 otherwise */
static long parse_option(const char* arg, const char* name, long lo, long hi) {
    const size_t len = strlen(name);
    char* end;
    long v;
    if (strncmp(arg, name, len) || arg[len] != '=') return -1;
    v = strtol(arg + len + 1, &end, 10);
    return (end == arg + len + 1 || *end || v < lo || v > hi) ? -1 : v;
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

static void report(const fldr_shutter_info* info, int n) {
    int k;
    for (k = 0; k < n; ++k)
        fprintf(stderr, "output %lld: %d points, %d interpolated%s\n", (long long)info[k].j, info[k].points, info[k].interpolated,
                info[k].truncated ? ", shortened" : "");
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_light_config lcfg;
    fldr_shutter_config cfg;
    fldr_light_curve* curve = NULL;
    fldr_scene_result scene;
    fldr_model* model = NULL;
    fldr_light* c = NULL;
    fldr_video_frame in, *outs;
    fldr_shutter_info* info;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, max_out, status = 0, bps = 1, transfer = FLDR_LIGHT_GAMMA24;
    long n = 0, cuts = 0, written = 0, v;
    size_t fsize;
    if (argc < 6 || argc > 13) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    if (W < 2 || H < 2 || !parse_rate(argv[4], &cfg.in_num, &cfg.in_den) || !parse_rate(argv[5], &cfg.out_num, &cfg.out_den)) {
        usage(argv[0]);
        return 2;
    }
    cfg.H = H; cfg.W = W;
    cfg.format.layout = FLDR_VIDEO_I420;
    cfg.format.matrix = FLDR_VIDEO_BT709;
    cfg.format.range = FLDR_VIDEO_LIMITED;
    cfg.shutter_num = 180; cfg.shutter_den = 360;
    cfg.sub = 4;
    cfg.scene = 1;                                     /* scene_params 0, 0: the defaults of fldr_rate.h */
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "noscd")) cfg.scene = 0;
        else if (!strcmp(argv[k], "gamma")) transfer = FLDR_LIGHT_GAMMA24;
        else if (!strcmp(argv[k], "pq")) transfer = FLDR_LIGHT_PQ;
        else if (!strcmp(argv[k], "hlg")) transfer = FLDR_LIGHT_HLG;
        else if ((v = parse_option(argv[k], "angle", 1, 360)) > 0) cfg.shutter_num = (int32_t)v;
        else if ((v = parse_option(argv[k], "sub", 1, FLDR_SHUTTER_MAX_SUB)) > 0) cfg.sub = (int32_t)v;
        else { usage(argv[0]); return 2; }
    }
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_light_curve_create(transfer, cfg.format.depth, NULL, cfg.device, &curve);
    if (rc) { fprintf(stderr, "fldr_light_curve_create: %s (%d)\n", fldr_light_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    lcfg.shutter = cfg;
    lcfg.curve = curve;
    rc = fldr_light_create(model, &lcfg, &c);
    if (rc) {
        fprintf(stderr, "fldr_light_create: %s (%d)\n", fldr_light_error_string(rc), rc);
        fldr_light_curve_destroy(curve);
        fldr_model_destroy(model);
        return 1;
    }
    max_out = fldr_light_max_out(c);
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)max_out);
    info = (fldr_shutter_info*)malloc(sizeof(fldr_shutter_info) * (size_t)max_out);
    if (!frame || !obuf || !outs || !info) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_light_push(c, &in, outs, info, &n_out, &scene);
        if (rc) { fprintf(stderr, "fldr_light_push: %s (%d)\n", fldr_light_error_string(rc), rc); status = 1; break; }
        if (scene.cut) { fprintf(stderr, "cut at frame %ld\n", n); ++cuts; }
        report(info, n_out);
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_light_flush(c, outs, info, &n_out);
        if (rc) { fprintf(stderr, "fldr_light_flush: %s (%d)\n", fldr_light_error_string(rc), rc); status = 1; }
        else if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) status = 1;
        else { report(info, n_out); written += n_out; }
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld frames out, %ld cuts\n", n, written, cuts);
    fldr_light_destroy(c);
    fldr_light_curve_destroy(curve);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs); free(info);
    return status;
}
