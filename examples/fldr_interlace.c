/* fldr_interlace — progressive raw I420 video to interlaced video with true fields, with the interlace API (include/fldr_interlace.h);
 * no Python, no device headers.
 *
 *   fldr_interlace weights.npz H W IN_FPS OUT_FPS in.yuv out.yuv [p10] [bff] [filter=none|linear|complex] [scene=0|1]
 *
 * in.yuv: raw progressive frames, yuv420p, or yuv420p10le with p10, H x W at IN_FPS; "-" is stdin.  out.yuv: woven interlaced frames
 * of the same format at OUT_FPS FRAMES per second (25 for 1080i25 / 576i, 30000/1001 for 1080i29.97 / 480i); "-" is stdout.  A rate is
 * NUM/DEN or a plain integer.  H must be a multiple of 4.  Every field sits at its own instant: field m at input position
 * m x IN_FPS / (2 OUT_FPS), an input frame's own rows where that is a whole number, interpolated rows otherwise, the nearer frame's at a
 * scene cut (scene=0 turns the cut measure off).  Top field first unless bff is given.  filter: the vertical anti-twitter filter,
 * linear (1 2 1) unless told otherwise.  Where no field needs interpolating (50 -> 25, 60000/1001 -> 30000/1001) no model is needed, and
 * weights.npz may be "-".  One line per frame goes to stderr: where its two fields come from.  Colour: BT.709 limited range.  Device 0.
 * For example:
 *
 *   ffmpeg -i film_24p.mov -f rawvideo -pix_fmt yuv420p - | fldr_interlace weights.npz 1080 1920 24000/1001 30000/1001 - - | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 30000/1001 -i - -flags +ilme+ildct -top 1 broadcast.mxf */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_interlace.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz H W IN_FPS OUT_FPS in.yuv out.yuv [p10] [bff] [filter=none|linear|complex] [scene=0|1]"
                    "  (raw progressive I420 frames in, woven interlaced frames out; H a multiple of 4; p10: yuv420p10le; rates like 24, 25 or"
                    " 30000/1001, OUT_FPS in frames; in.yuv / out.yuv: a file or - ; weights.npz may be - where no field is interpolated)\n", prog);
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

static void print_frames(const fldr_interlace_report* rep, int n, long long B) {
    int k, f;
    for (k = 0; k < n; ++k) {
        fprintf(stderr, "frame %lld:", (long long)rep[k].frame);
        for (f = 0; f < 2; ++f) {
            if (rep[k].r[f]) fprintf(stderr, " %lld+%lld/%lld%s", (long long)rep[k].input[f], (long long)rep[k].r[f], B, rep[k].cut[f] ? " (cut)" : "");
            else fprintf(stderr, " %lld%s", (long long)rep[k].input[f], f && rep[k].held ? " (held)" : "");
        }
        fprintf(stderr, "\n");
    }
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_interlace_config cfg;
    fldr_interlace_schedule first;
    fldr_interlace_report* rep = NULL;
    fldr_model* model = NULL;
    fldr_interlace* c = NULL;
    fldr_video_frame in, *outs = NULL;
    FILE *fin, *fout;
    uint8_t *frame = NULL, *obuf = NULL;
    int W, H, rc, k, n_out, max_out, status = 0, bps = 1;
    long n = 0, written = 0;
    size_t fsize;
    if (argc < 8 || argc > 12) { usage(argv[0]); return 2; }
    H = atoi(argv[2]);
    W = atoi(argv[3]);
    if (W < 2 || H < 4 || H % 4) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.rate.H = H; cfg.rate.W = W;
    cfg.rate.format.layout = FLDR_VIDEO_I420;
    cfg.rate.format.matrix = FLDR_VIDEO_BT709;
    cfg.rate.format.range = FLDR_VIDEO_LIMITED;
    cfg.rate.scene = 1;                                /* scene_params 0, 0: the rate header's defaults */
    cfg.tff = 1;
    cfg.filter = FLDR_INTERLACE_LINEAR;
    if (!parse_rate(argv[4], &cfg.rate.in_num, &cfg.rate.in_den) || !parse_rate(argv[5], &cfg.rate.out_num, &cfg.rate.out_den)) { usage(argv[0]); return 2; }
    for (k = 8; k < argc; ++k) {
        if (!strcmp(argv[k], "p10")) { cfg.rate.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "bff")) cfg.tff = 0;
        else if (!strcmp(argv[k], "filter=none")) cfg.filter = FLDR_INTERLACE_NONE;
        else if (!strcmp(argv[k], "filter=linear")) cfg.filter = FLDR_INTERLACE_LINEAR;
        else if (!strcmp(argv[k], "filter=complex")) cfg.filter = FLDR_INTERLACE_COMPLEX;
        else if (!strcmp(argv[k], "scene=0")) cfg.rate.scene = 0;
        else if (!strcmp(argv[k], "scene=1")) cfg.rate.scene = 1;
        else { usage(argv[0]); return 2; }
    }
    /* the schedule is host arithmetic: a ratio the converter does not take, or "-" for weights that are needed, ends here */
    if (fldr_interlace_plan(&cfg, 0, &first)) { usage(argv[0]); return 2; }
    if (!strcmp(argv[1], "-") && first.B != 1) { usage(argv[0]); return 2; }
    if (strcmp(argv[1], "-")) {
        memset(&mcfg, 0, sizeof(mcfg));
        rc = fldr_model_create_npz(argv[1], &mcfg, &model);
        if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    }
    rc = fldr_interlace_create(model, &cfg, &c);
    if (rc) { fprintf(stderr, "fldr_interlace_create: %s (%d)\n", fldr_interlace_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    max_out = fldr_interlace_max_out(c);
    fin = strcmp(argv[6], "-") ? fopen(argv[6], "rb") : stdin;
    fout = strcmp(argv[7], "-") ? fopen(argv[7], "wb") : stdout;
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * (H / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(*outs) * (size_t)max_out);
    rep = (fldr_interlace_report*)malloc(sizeof(*rep) * (size_t)max_out);
    if (!fin || !fout || !frame || !obuf || !outs || !rep) {
        fprintf(stderr, !fin || !fout ? "cannot open %s\n" : "out of memory\n", !fin ? argv[6] : argv[7]);
        fldr_interlace_destroy(c);
        fldr_model_destroy(model);
        free(frame); free(obuf); free(outs); free(rep);
        return 1;
    }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, fin) == fsize) {
        rc = fldr_interlace_push(c, &in, outs, &n_out, rep);
        if (rc) { fprintf(stderr, "fldr_interlace_push: %s (%d)\n", fldr_interlace_error_string(rc), rc); status = 1; break; }
        print_frames(rep, n_out, (long long)first.B);
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, fout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(fin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_interlace_flush(c, outs, &n_out, rep);
        if (rc) { fprintf(stderr, "fldr_interlace_flush: %s (%d)\n", fldr_interlace_error_string(rc), rc); status = 1; }
        else {
            print_frames(rep, n_out, (long long)first.B);
            if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, fout) != (size_t)n_out) status = 1;
            else written += n_out;
        }
    }
    if (fflush(fout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld interlaced frames out\n", n, written);
    fldr_interlace_destroy(c);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs); free(rep);
    return status;
}
