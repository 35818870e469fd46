/* fldr_probe — what a raw I420 stream carries: progressive frames (with or without repeats), film in interlaced video with its pulldown
 * cadence, or true interlaced video with its field order, by the probe API (include/fldr_probe.h); no Python, no device headers, no
 * weights.
 *
 *   fldr_probe W H IN [p10] [window=N] [anchor=top|bottom] [quiet]
 *
 * IN: raw frames as a decoder hands them out (both fields woven into one frame), yuv420p, or yuv420p10le with p10; "-" is stdin.  H must
 * be a multiple of 4.  window=N (3 .. 64, default 32): the verdict is taken on the last N measured frames.  anchor: the field whose
 * repeats give a film's cadence, and the anchor the ivtc command line is printed with.  Every measured frame's class goes to stdout
 * unless quiet is given; then the verdict, and the command line of the example that converts such a stream.  For example:
 *
 *   ffmpeg -i tape.mxf -frames 40 -f rawvideo -pix_fmt yuv420p - | fldr_probe 1920 1080 -
 *
 * (1080 is a multiple of 4; 1088-row coded frames should be cropped first.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_probe.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s W H IN [p10] [window=N] [anchor=top|bottom] [quiet]"
                    "  (raw woven I420 frames, H a multiple of 4; p10: yuv420p10le; IN: a file or - ; window: 3 .. 64)\n", prog);
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

int main(int argc, char** argv) {
    static const char* const CLASS[4] = { "still", "progressive", "film", "video" };
    static const char* const KIND[5] = { "unknown", "progressive", "film", "interlaced", "mixed" };
    fldr_probe_config cfg;
    fldr_probe_verdict v;
    fldr_probe_result res;
    fldr_probe* c = NULL;
    fldr_video_frame in;
    FILE* fin;
    uint8_t* frame;
    int W, H, rc, k, status = 0, bps = 1, quiet = 0;
    const char* p10 = "";
    long n = 0;
    size_t fsize;
    if (argc < 4 || argc > 8) { usage(argv[0]); return 2; }
    W = atoi(argv[1]);
    H = atoi(argv[2]);
    if (W < 1 || H < 4 || H % 4) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    cfg.format.layout = FLDR_VIDEO_I420;
    cfg.window = 32;
    for (k = 4; k < argc; ++k) {
        if (!strcmp(argv[k], "p10")) { cfg.format.depth = 10; bps = 2; p10 = " p10"; }
        else if (!strcmp(argv[k], "quiet")) quiet = 1;
        else if (!strcmp(argv[k], "anchor=top")) cfg.params.anchor = 0;
        else if (!strcmp(argv[k], "anchor=bottom")) cfg.params.anchor = 1;
        else if (parse_word(argv[k], "window=", &cfg.window)) continue;
        else { usage(argv[0]); return 2; }
    }
    if (cfg.window < FLDR_PROBE_MIN_WINDOW || cfg.window > FLDR_PROBE_MAX_WINDOW) { usage(argv[0]); return 2; }
    rc = fldr_probe_create(&cfg, &c);
    if (rc) { fprintf(stderr, "fldr_probe_create: %s (%d)\n", fldr_probe_error_string(rc), rc); return 1; }
    fin = strcmp(argv[3], "-") ? fopen(argv[3], "rb") : stdin;
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * (H / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    if (!fin || !frame) {
        fprintf(stderr, !fin ? "cannot open %s\n" : "out of memory\n", argv[3]);
        fldr_probe_destroy(c);
        free(frame);
        return 1;
    }
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, fin) == fsize) {
        rc = fldr_probe_push(c, &in);
        if (rc) { fprintf(stderr, "fldr_probe_push: %s (%d)\n", fldr_probe_error_string(rc), rc); status = 1; break; }
        ++n;
        if (!quiet && n >= 3) {                        /* the push of frame n - 1 measured frame n - 2: the newest result of the ring */
            int64_t number = 0;
            const int held = n - 2 < cfg.window ? (int)(n - 2) : cfg.window;
            rc = fldr_probe_result_get(c, held - 1, &res, &number);
            if (rc) { fprintf(stderr, "fldr_probe_result_get: %s (%d)\n", fldr_probe_error_string(rc), rc); status = 1; break; }
            printf("frame %lld: %s  comb C %u/%u P %u/%u N %u/%u  field moving %u/%u  order sums %llu/%llu\n", (long long)number,
                   CLASS[fldr_probe_frame_class(&res, &cfg.params)], res.max_tile_comb[0][0], res.max_tile_comb[1][0], res.max_tile_comb[0][1],
                   res.max_tile_comb[1][1], res.max_tile_comb[0][2], res.max_tile_comb[1][2], res.field_moving_tiles[0],
                   res.field_moving_tiles[1], (unsigned long long)res.tff_sum, (unsigned long long)res.bff_sum);
        }
    }
    if (!status && ferror(fin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_probe_verdict_get(c, &v);
        if (rc) { fprintf(stderr, "fldr_probe_verdict_get: %s (%d)\n", fldr_probe_error_string(rc), rc); status = 1; }
    }
    if (!status) {
        printf("%ld frames in, %d measured: %d still, %d progressive, %d film, %d video (votes tff %d, bff %d)\n", n, v.n_frames, v.n_still,
               v.n_prog, v.n_film, v.n_video, v.votes_tff, v.votes_bff);
        printf("verdict: %s", KIND[v.kind]);
        if (v.kind == FLDR_PROBE_PROGRESSIVE || v.kind == FLDR_PROBE_FILM)
            printf(", cycle %d drop %d%s, %d repeats confirmed", v.cycle, v.drop, v.irregular ? " (irregular)" : "", v.confirmed);
        if (v.kind == FLDR_PROBE_INTERLACED)
            printf(", %s%s", v.tff > 0 ? "top field first" : v.tff == 0 ? "bottom field first" : "field order undecided", v.mixed ? ", progressive frames among it" : "");
        printf("\n");
        if (v.kind == FLDR_PROBE_PROGRESSIVE && v.drop == 0 && !v.irregular) printf("use: fldr_fps weights.npz %d %d IN_RATE OUT_RATE%s < in.yuv > out.yuv\n", W, H, p10);
        else if (v.kind == FLDR_PROBE_PROGRESSIVE && !v.irregular) printf("use: fldr_film weights.npz %d %d IN_RATE OUT_RATE cycle=%d drop=%d%s < in.yuv > out.yuv\n", W, H, v.cycle, v.drop, p10);
        else if (v.kind == FLDR_PROBE_FILM && !v.irregular)
            printf("use: fldr_ivtc weights.npz %d %d IN_RATE OUT_RATE cycle=%d drop=%d anchor=%s%s < in.yuv > out.yuv\n", W, H, v.cycle, v.drop, v.anchor ? "bottom" : "top", p10);
        else if (v.kind == FLDR_PROBE_INTERLACED && v.tff >= 0) printf("use: fldr_deint weights.npz %d %d IN OUT%s%s   (tff=%d)\n", W, H, v.tff ? "" : " bff", p10, v.tff);
        else printf("use: no single converter fits; look at the frames above\n");
    }
    fldr_probe_destroy(c);
    free(frame);
    if (fin && fin != stdin) fclose(fin);
    return status;
}
