/* fldr_ivtc — inverse telecine and frame-rate conversion of raw interlaced I420 video that carries film (24 fps in 60i by 3:2 pulldown,
 * 25 fps in 50i with the fields out of phase), with the pulldown API (include/fldr_pulldown.h); no Python, no device headers.
 *
 *   fldr_ivtc weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN cycle=N drop=D [anchor=top|bottom] [post=keep|average]
 *             [bt601|bt709] [full] [p10] [noscd] < in.yuv > out.yuv
 *
 * It is fldr_fps with field matching in front: every woven frame keeps its anchor field (anchor=top, the default, or bottom) and takes
 * the other field from itself, the previous or the next frame, whichever weaves with the least combing; of every N matched frames the D
 * whose anchor field repeats the frame before are taken out, and the others are converted from IN x (N - D) / N to OUT as fldr_fps
 * converts them.  IN is the container's FRAME rate.  3:2 pulldown is cycle=5 drop=1; 2:2 out of phase, or progressive frames in an
 * interlaced container, cycle=1 drop=0.  post=average rebuilds the other field of a frame that stays combed (true video, an orphan
 * field at an edit) from the anchor field's line average; post=keep (the default) leaves it woven.  H must be a multiple of 4.  One
 * line per cycle goes to stderr: its first frame, each frame's match ('c', 'p', 'n'; in capitals where the frame stayed combed), which
 * frames were dropped ('x') and kept ('.'), and the survivors that began a new scene.  in.yuv / out.yuv, rates, colour and the other
 * words are fldr_fps's.  Outputs arrive a frame plus a cycle late.  For example:
 *
 *   ffmpeg -i ntsc_master.mov -f rawvideo -pix_fmt yuv420p - | fldr_ivtc weights.npz 720 480 30000/1001 60000/1001 cycle=5 drop=1 | \
 *       ffmpeg -f rawvideo -pix_fmt yuv420p -s 720x480 -r 60000/1001 -i - smooth.mp4 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_pulldown.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H IN_NUM/IN_DEN OUT_NUM/OUT_DEN cycle=N drop=D [anchor=top|bottom] [post=keep|average]"
                    " [bt601|bt709] [full] [p10] [noscd] < in.yuv > out.yuv  (raw woven I420 frames, H a multiple of 4; p10: yuv420p10le;"
                    " rates like 30, 60 or 30000/1001, IN the container's frame rate; of every N matched frames D are duplicates: 3:2"
                    " pulldown is cycle=5 drop=1)\n", prog);
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

static void print_report(const fldr_pulldown_report* rep, long* dropped, long* combed, long* cuts) {
    uint32_t k;
    int survivor = 0;
    if (!rep->n_frames) return;
    fprintf(stderr, "cycle at frame %lld: match ", (long long)rep->first_frame);
    for (k = 0; k < rep->n_frames; ++k) {
        const int stays = (int)(rep->combed_mask >> k & 1u);
        const char* names = stays ? "CPN" : "cpn";
        fputc(rep->match[k] >= 0 && rep->match[k] <= 2 ? names[rep->match[k]] : '?', stderr);
        *combed += stays;
    }
    fputc(' ', stderr);
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
    fldr_pulldown_config cfg;
    fldr_pulldown_report rep;
    fldr_model* model = NULL;
    fldr_pulldown* c = NULL;
    fldr_video_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, rc, k, n_out, max_out, status = 0, bps = 1, have_cycle = 0, have_drop = 0;
    long n = 0, cuts = 0, dropped = 0, combed = 0, written = 0;
    size_t fsize;
    if (argc < 8 || argc > 14) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    if (W < 2 || H < 4 || H % 4 || !parse_rate(argv[4], &cfg.rate.in_num, &cfg.rate.in_den) ||
        !parse_rate(argv[5], &cfg.rate.out_num, &cfg.rate.out_den)) {
        usage(argv[0]);
        return 2;
    }
    cfg.rate.H = H; cfg.rate.W = W;
    cfg.rate.format.layout = FLDR_VIDEO_I420;
    cfg.rate.format.matrix = FLDR_VIDEO_BT709;
    cfg.rate.format.range = FLDR_VIDEO_LIMITED;
    cfg.rate.scene = 1;                                /* scene_params and params zero: the headers' defaults */
    cfg.anchor = 0;
    cfg.post = FLDR_PULLDOWN_POST_KEEP;
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.rate.format.matrix = FLDR_VIDEO_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.rate.format.matrix = FLDR_VIDEO_BT709;
        else if (!strcmp(argv[k], "full")) cfg.rate.format.range = FLDR_VIDEO_FULL;
        else if (!strcmp(argv[k], "p10")) { cfg.rate.format.depth = 10; bps = 2; }
        else if (!strcmp(argv[k], "noscd")) cfg.rate.scene = 0;
        else if (!strcmp(argv[k], "anchor=top")) cfg.anchor = 0;
        else if (!strcmp(argv[k], "anchor=bottom")) cfg.anchor = 1;
        else if (!strcmp(argv[k], "post=keep")) cfg.post = FLDR_PULLDOWN_POST_KEEP;
        else if (!strcmp(argv[k], "post=average")) cfg.post = FLDR_PULLDOWN_POST_AVERAGE;
        else if (parse_word(argv[k], "cycle=", &cfg.cycle)) have_cycle = 1;
        else if (parse_word(argv[k], "drop=", &cfg.drop)) have_drop = 1;
        else { usage(argv[0]); return 2; }
    }
    if (!have_cycle || !have_drop || cfg.cycle < 1 || cfg.cycle > FLDR_PULLDOWN_MAX_CYCLE || cfg.drop >= cfg.cycle) { usage(argv[0]); return 2; }
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_pulldown_create(model, &cfg, &c);
    if (rc) { fprintf(stderr, "fldr_pulldown_create: %s (%d)\n", fldr_pulldown_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    max_out = fldr_pulldown_max_out(c);
    fsize = ((size_t)W * H + 2 * (size_t)((W + 1) / 2) * ((H + 1) / 2)) * (size_t)bps;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)max_out);
    outs = (fldr_video_frame*)malloc(sizeof(fldr_video_frame) * (size_t)max_out);
    if (!frame || !obuf || !outs) {
        fprintf(stderr, "out of memory\n");
        fldr_pulldown_destroy(c);
        fldr_model_destroy(model);
        free(frame); free(obuf); free(outs);
        return 1;
    }
    for (k = 0; k < max_out; ++k) outs[k] = i420(obuf + fsize * (size_t)k, W, H, bps);
    in = i420(frame, W, H, bps);
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_pulldown_push(c, &in, outs, &n_out, &rep);
        if (rc) { fprintf(stderr, "fldr_pulldown_push: %s (%d)\n", fldr_pulldown_error_string(rc), rc); status = 1; break; }
        print_report(&rep, &dropped, &combed, &cuts);
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        written += n_out;
        ++n;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (!status) {
        rc = fldr_pulldown_flush(c, outs, &n_out, &rep);
        if (rc) { fprintf(stderr, "fldr_pulldown_flush: %s (%d)\n", fldr_pulldown_error_string(rc), rc); status = 1; }
        else {
            print_report(&rep, &dropped, &combed, &cuts);
            if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) status = 1;
            else written += n_out;
        }
    }
    if (fflush(stdout)) status = 1;
    fprintf(stderr, "%ld frames in, %ld dropped, %ld stayed combed, %ld frames out, %ld cuts\n", n, dropped, combed, written, cuts);
    fldr_pulldown_destroy(c);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
