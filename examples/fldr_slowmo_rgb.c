/* fldr_slowmo_rgb — slow motion on raw RGB video (four bytes per pixel, 10-bit RGB words, planar GBR) with the API of
 * include/fldr_rgb.h; no Python, no HIP headers.
 *
 *   fldr_slowmo_rgb weights.npz W H FACTOR <bgra|rgba|argb|abgr|x2rgb10le|x2bgr10le|gbrp|gbrap|gbrp10le|gbrap10le>
 *                   [alpha=opaque|nearer|blend] < in.raw > out.raw
 *
 * The frames on stdin and stdout are what ffmpeg's rawvideo muxer writes for the pixel format of that name: tight rows, the planes of
 * gbrp / gbrap one after the other (G, B, R, A).  The output is the first frame, then for every further frame FACTOR - 1 interpolated
 * frames (at t = k / FACTOR) followed by the frame itself, byte for byte.  Alpha of the interpolated frames: opaque unless told
 * otherwise (nearer: that of the input frame nearer in time; blend: the two inputs' alpha blended at t).  Device 0, the shipped
 * configuration.  For example:
 *
 *   ffmpeg -i capture.mkv -pix_fmt bgra -f rawvideo - | fldr_slowmo_rgb weights.npz 1920 1080 2 bgra alpha=blend | \
 *       ffmpeg -f rawvideo -pix_fmt bgra -s 1920x1080 -r 120 -i - -c:v qtrle out.mov */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_rgb.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H FACTOR <bgra|rgba|argb|abgr|x2rgb10le|x2bgr10le|gbrp|gbrap|gbrp10le|gbrap10le> "
                    "[alpha=opaque|nearer|blend] < in.raw > out.raw  (raw frames; FACTOR >= 2)\n", prog);
}

static const struct { const char* name; int layout, depth; } FORMATS[] = {
    {"bgra", FLDR_RGB_BGRA, 8},         {"rgba", FLDR_RGB_RGBA, 8},         {"argb", FLDR_RGB_ARGB, 8},   {"abgr", FLDR_RGB_ABGR, 8},
    {"x2rgb10le", FLDR_RGB_X2RGB10, 10}, {"x2bgr10le", FLDR_RGB_X2BGR10, 10}, {"gbrp", FLDR_RGB_GBRP, 8},   {"gbrap", FLDR_RGB_GBRAP, 8},
    {"gbrp10le", FLDR_RGB_GBRP, 10},    {"gbrap10le", FLDR_RGB_GBRAP, 10}};

/* planes and bytes per row of a tight frame */
static int planes_of(const fldr_rgb_format* f) { return f->layout < FLDR_RGB_GBRP ? 1 : f->layout == FLDR_RGB_GBRP ? 3 : 4; }
static int64_t pitch_of(const fldr_rgb_format* f, int W) { return f->layout < FLDR_RGB_GBRP ? 4 * (int64_t)W : (int64_t)W * (f->depth == 10 ? 2 : 1); }

static fldr_rgb_frame frame_at(uint8_t* buf, const fldr_rgb_format* f, int W, int H) {
    fldr_rgb_frame fr;
    int p;
    memset(&fr, 0, sizeof(fr));
    for (p = 0; p < planes_of(f); ++p) {
        fr.plane[p] = buf + (size_t)p * (size_t)pitch_of(f, W) * (size_t)H;
        fr.pitch[p] = pitch_of(f, W);
    }
    return fr;
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_rgb_session_config cfg;
    fldr_model* model = NULL;
    fldr_rgb_session* s = NULL;
    fldr_rgb_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, factor, n_t, rc, k, n_out, first = 1, status = 0, found = 0;
    size_t fsize;
    if (argc < 6 || argc > 7) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    factor = atoi(argv[4]);
    if (W < 2 || H < 2 || factor < 2) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    for (k = 0; k < (int)(sizeof(FORMATS) / sizeof(FORMATS[0])); ++k)
        if (!strcmp(argv[5], FORMATS[k].name)) { cfg.in_format.layout = FORMATS[k].layout; cfg.in_format.depth = FORMATS[k].depth; found = 1; }
    if (!found) { usage(argv[0]); return 2; }
    cfg.in_format.alpha = FLDR_RGB_ALPHA_OPAQUE;
    if (argc == 7) {
        if (!strcmp(argv[6], "alpha=opaque")) cfg.in_format.alpha = FLDR_RGB_ALPHA_OPAQUE;
        else if (!strcmp(argv[6], "alpha=nearer")) cfg.in_format.alpha = FLDR_RGB_ALPHA_NEARER;
        else if (!strcmp(argv[6], "alpha=blend")) cfg.in_format.alpha = FLDR_RGB_ALPHA_BLEND;
        else { usage(argv[0]); return 2; }
    }
    cfg.out_format = cfg.in_format;                    /* the policy is read from the out format */
    n_t = factor - 1;
    cfg.n_t = n_t;                                     /* t = NULL: k / FACTOR, k = 1 .. FACTOR - 1 */
    fsize = (size_t)pitch_of(&cfg.in_format, W) * (size_t)H * (size_t)planes_of(&cfg.in_format);
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)calloc(fsize, (size_t)n_t);
    outs = (fldr_rgb_frame*)malloc(sizeof(fldr_rgb_frame) * (size_t)n_t);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < n_t; ++k) outs[k] = frame_at(obuf + fsize * (size_t)k, &cfg.out_format, W, H);
    in = frame_at(frame, &cfg.in_format, W, H);
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_rgb_session_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_rgb_session_create: %s (%d)\n", fldr_rgb_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_rgb_session_push(s, &in, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_rgb_session_push: %s (%d)\n", fldr_rgb_error_string(rc), rc); status = 1; break; }
        if (!first && n_out != n_t) { fprintf(stderr, "unexpected output count %d\n", n_out); status = 1; break; }
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        if (fwrite(frame, 1, fsize, stdout) != fsize) { status = 1; break; }
        first = 0;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (fflush(stdout)) status = 1;
    fldr_rgb_session_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
