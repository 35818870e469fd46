/* fldr_film — frame-rate conversion of raw I420 video that carries repeated frames (film in a 60p container, 25 fps in 50p, animation
 * on twos), with the cadence API (include/fldr_cadence.h); no Python, no device headers.
 *
 *   fldr_film weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN cycle=N drop=D [bt601|bt709] [full] [p10] [noscd] [tile=T] < in.yuv > out.yuv
 *
 * It is fldr_fps with a declared cadence: of every N container frames the D that differ least from their predecessors are taken out,
 * and the others are converted from IN x (N - D) / N to OUT as fldr_fps converts them.  3:2 pulldown in 60p is cycle=5 drop=3, 2:2 is
 * cycle=2 drop=1, 24 fps in 30p is cycle=5 drop=1.  tile=T sets tile_sad_min (1 .. 261120; default 2048).  One line per cycle goes
 * to stderr: its first frame, which frames were dropped ('x') and kept ('.'), how many dropped frames were moving (a wrong or broken
 * cadence) and how many kept frames were still, and the survivors that began a new scene.  in.yuv / out.yuv, rates, colour and the
 * other words are fldr_fps's.  Outputs arrive one cycle late.  For example:
 *
 *   ffmpeg -i telecined_60p.mp4 -f rawvideo -pix_fmt yuv420p - | fldr_film weights.npz 1920 1080 60000/1001 60000/1001 cycle=5 drop=3 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 1920x1080 -r 60000/1001 -i - smooth.mp4 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_cadence.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN cycle=N drop=D [bt601|bt709] [full] [p10] [noscd] [tile=T]"
                    " < in.yuv > out.yuv  (raw I420 frames; p10: yuv420p10le; rates like 24, 60 or 24000/1001; of every N frames D are"
                    " repeats: 3:2 in 60p is cycle=5 drop=3)\n", prog);
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

static void print_report(const fldr_cadence_report* rep, long* dropped, long* cuts) {
    uint32_t k;
    int survivor = 0;
    if (!rep->n_frames) return;
    fprintf(stderr, "cycle at frame %lld: ", (long long)rep->first_frame);
    for (k = 0; k < rep->n_frames; ++k) {
        const int gone = (int)(rep->dropped_mask >> k & 1u);
        fputc(gone ? 'x' : '.', stderr);
        *dropped += gone;
    }
    fprintf(stderr, ", %u moving dropped, %u still kept", (unsigned)rep->moving_dropped, (unsigned)rep->still_kept);
    for (k = 0; k < rep->n_frames; ++k) {
        if (rep->dropped_mask >> k & 1u) continue;
        if (rep->cut_mask >> survivor & 1u) { fprintf(stderr, ", cut at frame %lld", (long long)rep->first_frame + k); ++*cuts; }
        ++survivor;
    }
    fputc('\n', stderr);
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_cadence_config cfg;
    fldr_cadence_report rep;
    fldr_model* model = NULL;
    fldr_cadence* c = NULL;
    fldr_video_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, max_out, status = 0, bps = 1, have_cycle = 0, have_drop = 0;
    long n = 0, cuts = 0, dropped = 0, written = 0;
    size_t fsize;
    if (argc < 8 || argc > 13) { usage(argv[0]); return 2; }
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
    cfg.rate.scene = 1;                                /* scene_params 0, 0 and repeat 0: the headers' defaults */
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.rate.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.rate.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.rate.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.rate.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "noscd")) cfg.rate.scene = 0;
        else if (parse_word(argv[k], "cycle=", &cfg.cycle)) have_cycle = 1;
        else if (parse_word(argv[k], "drop=", &cfg.drop)) have_drop = 1;
        else if (parse_word(argv[k], "tile=", &cfg.repeat.tile_sad_min)) continue;
        else { usage(argv[0]); return 2; }
    }
    if (!have_cycle || !have_drop || cfg.cycle < 1 || cfg.cycle > FLDR_CADENCE_MAX_CYCLE || cfg.drop >= cfg.cycle) { usage(argv[0]); return 2; }
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_cadence_create(model, &cfg, &c);
    if (rc) { fprintf(stderr, "fldr_cadence_create: %s (%d)\n", fldr_cadence_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    max_out = fldr_cadence_max_out(c);
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)max_out);
    if (!frame || !obuf || !outs) {
        fprintf(stderr, "out of memory\n");
        fldr_cadence_destroy(c);
        fldr_model_destroy(model);
        free(frame); free(obuf); free(outs);
        return 1;
    }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_cadence_push(c, &in, outs, &n_out, &rep);
        if (rc) { fprintf(stderr, "fldr_cadence_push: %s (%d)\n", fldr_cadence_error_string(rc), rc); status = 1; break; }
        print_report(&rep, &dropped, &cuts);
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_cadence_flush(c, outs, &n_out, &rep);
        if (rc) { fprintf(stderr, "fldr_cadence_flush: %s (%d)\n", fldr_cadence_error_string(rc), rc); status = 1; }
        else {
            print_report(&rep, &dropped, &cuts);
            if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) status = 1;
            else written += n_out;
        }
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld dropped, %ld frames out, %ld cuts\n", n, dropped, written, cuts);
    fldr_cadence_destroy(c);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
