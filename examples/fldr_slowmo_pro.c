/* fldr_slowmo_pro — slow motion on raw 4:2:2 / 4:4:4 video with the API of include/fldr_chroma.h; no Python, no HIP headers.
 *
 *   fldr_slowmo_pro weights.npz W H FACTOR PIXFMT [bt601|bt709] [full] < in.yuv > out.yuv
 *
 * PIXFMT is ffmpeg's name of the raw frames on stdin and stdout: yuv422p10le, yuv422p, uyvy422 or yuv444p.  The output is the first
 * frame, then for every further frame FACTOR - 1 interpolated frames (at t = k / FACTOR) followed by the frame itself, byte for byte.
 * Colour: BT.709 limited range unless told otherwise.  Device 0, the shipped configuration.  For example:
 *
 *   ffmpeg -i in.mov -f rawvideo -pix_fmt yuv422p10le - | fldr_slowmo_pro weights.npz 3840 2160 2 yuv422p10le | \
 *       ffmpeg -f rawvideo -pix_fmt yuv422p10le -s 3840x2160 -r 100 -i - -c:v prores_ks -profile:v 3 out.mov */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_chroma.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H FACTOR yuv422p10le|yuv422p|uyvy422|yuv444p [bt601|bt709] [full] < in.yuv > out.yuv  (raw frames; FACTOR >= 2)\n",
            prog);
}

/* bytes per row of plane p (0 when the layout has no such plane) */
static int64_t row_bytes(const fldr_chroma_format* f, int p, int W) {
    const int64_t half = (W + 1) / 2, bps = f->depth == 10 ? 2 : 1;
    if (f->layout == FLDR_CHROMA_UYVY) return p == 0 ? 4 * half : 0;
    return bps * (p == 0 ? W : f->sampling == FLDR_CHROMA_444 ? W : half);
}

/* the planes of one packed frame in buf */
static fldr_chroma_frame frame_at(uint8_t* buf, const fldr_chroma_format* f, int W, int H) {
    fldr_chroma_frame fr;
    int64_t off = 0;
    int p;
    memset(&fr, 0, sizeof(fr));
    for (p = 0; p < 3; ++p) {
        const int64_t rb = row_bytes(f, p, W);
        if (!rb) continue;
        fr.plane[p] = buf + off;
        fr.pitch[p] = rb;
        off += rb * H;
    }
    return fr;
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_chroma_session_config cfg;
    fldr_model* model = NULL;
    fldr_chroma_session* s = NULL;
    fldr_chroma_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, factor, n_t, rc, k, n_out, first = 1, status = 0;
    size_t fsize;
    if (argc < 6 || argc > 8) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    factor = atoi(argv[4]);
    if (W < 2 || H < 2 || factor < 2) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    cfg.in_format.matrix = FLDR_CHROMA_BT709;
    cfg.in_format.range = FLDR_CHROMA_LIMITED;
    cfg.in_format.sampling = FLDR_CHROMA_422;
    cfg.in_format.layout = FLDR_CHROMA_PLANAR;
    cfg.in_format.depth = 8;
    if (!strcmp(argv[5], "yuv422p10le")) cfg.in_format.depth = 10;
    else if (!strcmp(argv[5], "uyvy422")) cfg.in_format.layout = FLDR_CHROMA_UYVY;
    else if (!strcmp(argv[5], "yuv444p")) cfg.in_format.sampling = FLDR_CHROMA_444;
    else if (strcmp(argv[5], "yuv422p")) { usage(argv[0]); return 2; }
    for (k = 6; k < argc; ++k) {
        if (!strcmp(argv[k], "bt601")) cfg.in_format.matrix = FLDR_CHROMA_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.in_format.matrix = FLDR_CHROMA_BT709;
        else if (!strcmp(argv[k], "full")) cfg.in_format.range = FLDR_CHROMA_FULL;
        else { usage(argv[0]); return 2; }
    }
    cfg.out_format = cfg.in_format;
    n_t = factor - 1;
    cfg.n_t = n_t;                                     /* t = NULL: k / FACTOR, k = 1 .. FACTOR - 1 */
    fsize = 0;
    for (k = 0; k < 3; ++k) fsize += (size_t)row_bytes(&cfg.in_format, k, W) * (size_t)H;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)malloc(fsize * (size_t)n_t);
    outs = (fldr_chroma_frame*)malloc(sizeof(fldr_chroma_frame) * (size_t)n_t);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < n_t; ++k) outs[k] = frame_at(obuf + fsize * (size_t)k, &cfg.in_format, W, H);
    in = frame_at(frame, &cfg.in_format, W, H);
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_chroma_session_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_chroma_session_create: %s (%d)\n", fldr_chroma_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_chroma_session_push(s, &in, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_chroma_session_push: %s (%d)\n", fldr_chroma_error_string(rc), rc); status = 1; break; }
        if (!first && n_out != n_t) { fprintf(stderr, "unexpected output count %d\n", n_out); status = 1; break; }
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        if (fwrite(frame, 1, fsize, stdout) != fsize) { status = 1; break; }
        first = 0;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (fflush(stdout)) status = 1;
    fldr_chroma_session_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
