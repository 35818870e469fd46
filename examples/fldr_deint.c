/* fldr_deint — motion-compensated deinterlacing of raw interlaced I420 video (1080i, 576i, 480i) with the field API
 * (include/fldr_field.h); no Python, no device headers.
 *
 *   fldr_deint weights.npz W H IN OUT [bff] [rate=1|2] [bt601|bt709] [full] [p10] [noscd] [still=N] [slack=N]
 *
 * IN: raw woven frames (both fields in one frame, as a decoder hands them out), yuv420p, or yuv420p10le with p10; "-" is stdin.
 * OUT: progressive frames of the same format; "-" is stdout.  H must be a multiple of 4.  The field order is declared, not detected:
 * top field first unless bff is given.  rate=2 (the default) writes one frame per field, twice the frame rate; rate=1 one per frame,
 * the even fields only.  still=N and slack=N set the two guards of the weave in the format's code units (still=off switches the
 * static rule off); the defaults are the header's.  noscd switches the cut measure off.  Every cut goes to stderr with its field.
 * At rate 2 outputs arrive one frame late.  For example:
 *
 *   ffmpeg -i tape_1080i.mxf -f rawvideo -pix_fmt yuv420p - | fldr_deint weights.npz 1920 1080 - - | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 50 -i - progressive.mp4
 *
 * (1080 is a multiple of 4; 1088-row coded frames should be cropped first.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_field.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN OUT [bff] [rate=1|2] [bt601|bt709] [full] [p10] [noscd] [still=N|still=off] [slack=N]"
                    "  (raw woven I420 frames, H a multiple of 4; p10: yuv420p10le; IN / OUT: a file or - ; rate=2: one frame per field)\n", prog);
}

/* "key=123" -> 123 in *v; 0 when s does not begin with key or no whole number follows */
static int parse_word(const char* s, const char* key, int32_t* v) {
    const size_t n = strlen(key);
    char* end;
    long x;
    if (strncmp(s, key, n)) return 0;
    x = strtol(s + n, &end, 10);
    if (end == s + n || *end || x < 0 || x > 0x7fffffffL) return 0;
    *v = (int32_t)x;
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

static void print_cuts(const fldr_field_report* rep, int n, long* cuts) {
    int k;
    for (k = 0; k < n; ++k)
        if (rep[k].cut) { fprintf(stderr, "cut at field %lld\n", (long long)rep[k].field); ++*cuts; }
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_field_config cfg;
    fldr_field_params params;
    fldr_field_report rep[2];
    fldr_model* model = NULL;
    fldr_field* d = NULL;
    fldr_video_frame in, outs[2];
    FILE *fin, *fout;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, status = 0, bps = 1, have_params = 0;
    int32_t still = -2, slack = -1;
    long n = 0, cuts = 0, written = 0;
    size_t fsize;
    if (argc < 6 || argc > 14) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    if (W < 2 || H < 4 || H % 4) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    cfg.format.layout = FLDR_VIDEO_I420;
    cfg.format.matrix = FLDR_VIDEO_BT709;
    cfg.format.range = FLDR_VIDEO_LIMITED;
    cfg.tff = 1;
    cfg.rate = 2;
    cfg.scene = 1;                                     /* scene_params 0, 0: the header's defaults */
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bff")) cfg.tff = 0;
        else if (!strcmp(argv[k], "bt601")) cfg.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "noscd")) cfg.scene = 0;
        else if (!strcmp(argv[k], "still=off")) { still = -1; have_params = 1; }
        else if (parse_word(argv[k], "rate=", &cfg.rate)) continue;
        else if (parse_word(argv[k], "still=", &still)) have_params = 1;
        else if (parse_word(argv[k], "slack=", &slack)) have_params = 1;
        else { usage(argv[0]); return 2; }
    }
    if (cfg.rate != 1 && cfg.rate != 2) { usage(argv[0]); return 2; }
    if (have_params) {                                 /* a word not given keeps the header's default */
        const int up = bps == 2 ? 2 : 0;
        memset(&params, 0, sizeof(params));
        params.still = still == -2 ? FLDR_FIELD_STILL_DEFAULT8 << up : still;
        params.slack = slack < 0 ? FLDR_FIELD_SLACK_DEFAULT8 << up : slack;
        cfg.params = &params;
    }
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_field_create(model, &cfg, &d);
    if (rc) { fprintf(stderr, "fldr_field_create: %s (%d)\n", fldr_field_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    fin = strcmp(argv[4], "-") ? fopen(argv[4], "rb") : stdin;
    fout = strcmp(argv[5], "-") ? fopen(argv[5], "wb") : stdout;
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * (H / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * 2);
    if (!fin || !fout || !frame || !obuf) {
        fprintf(stderr, !fin || !fout ? "cannot open %s\n" : "out of memory\n", !fin ? argv[4] : argv[5]);
        fldr_field_destroy(d);
        fldr_model_destroy(model);
        free(frame); free(obuf);
        return 1;
    }
    for (k = 0; k < 2; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, fin) == fsize) {
        rc = fldr_field_push(d, &in, outs, &n_out, rep);
        if (rc) { fprintf(stderr, "fldr_field_push: %s (%d)\n", fldr_field_error_string(rc), rc); status = 1; break; }
        print_cuts(rep, n_out, &cuts);
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, fout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(fin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_field_flush(d, outs, &n_out, rep);
        if (rc) { fprintf(stderr, "fldr_field_flush: %s (%d)\n", fldr_field_error_string(rc), rc); status = 1; }
        else if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, fout) != (size_t)n_out) status = 1;
        else written += n_out;
    }
    if (fflush(fout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld frames out, %ld cuts\n", n, written, cuts);
    fldr_field_destroy(d);
    fldr_model_destroy(model);
    free(frame); free(obuf);
    return status;
}
