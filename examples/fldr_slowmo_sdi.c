/* fldr_slowmo_sdi — slow motion on raw packed 10-bit video (v210, Y210, Y410) with the API of include/fldr_pack10.h; no Python, no HIP
 * headers.
 *
 *   fldr_slowmo_sdi weights.npz W H FACTOR [v210|y210|y410] [bt601|bt709] [full] < in.raw > out.raw
 *
 * The frames on stdin and stdout are what SDI capture and uncompressed QuickTime deliver and what ffmpeg's rawvideo muxer writes:
 * v210 rows at the customary pitch 128 ceil(W/48), y210 (ffmpeg: y210le) rows of 8 ceil(W/2) bytes, y410 (ffmpeg: xv30le) rows of 4 W
 * bytes.  The output is the first frame, then for every further frame FACTOR - 1 interpolated frames (at t = k / FACTOR) followed by
 * the frame itself, byte for byte; the bytes between a row's end and its pitch are zero in interpolated frames.  Colour: BT.709 limited
 * range unless told otherwise.  Device 0, the shipped configuration.  For example:
 *
 *   ffmpeg -i capture.mov -c:v v210 -f rawvideo - | fldr_slowmo_sdi weights.npz 1920 1080 2 | \
 *       ffmpeg -f rawvideo -c:v v210 -s 1920x1080 -r 100 -i - -c:v prores_ks -profile:v 3 out.mov */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_pack10.h"

static void usage(const char* prog) {
    fprintf(stderr, "usage: %s weights.npz W H FACTOR [v210|y210|y410] [bt601|bt709] [full] < in.raw > out.raw  (raw frames; FACTOR >= 2)\n", prog);
}

/* the pitch of the raw frames: v210 rows are padded to 128 bytes (48 pixels), the others are tight */
static int64_t pitch_of(int container, int W) {
    if (container == FLDR_PACK10_V210) return 128 * (((int64_t)W + 47) / 48);
    if (container == FLDR_PACK10_Y210) return 8 * (((int64_t)W + 1) / 2);
    return 4 * (int64_t)W;
}

static fldr_pack10_frame frame_at(uint8_t* buf, int64_t pitch) {
    fldr_pack10_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.plane[0] = buf;
    fr.pitch[0] = pitch;
    return fr;
}

int main(int argc, char** argv) {
    fldr_model_config mcfg;
    fldr_pack10_session_config cfg;
    fldr_model* model = NULL;
    fldr_pack10_session* s = NULL;
    fldr_pack10_frame in, *outs;
    uint8_t *frame, *obuf;
    int W, H, factor, n_t, rc, k, n_out, first = 1, status = 0;
    int64_t pitch;
    size_t fsize;
    if (argc < 5 || argc > 8) { usage(argv[0]); return 2; }
    W = atoi(argv[2]);
    H = atoi(argv[3]);
    factor = atoi(argv[4]);
    if (W < 2 || H < 2 || factor < 2) { usage(argv[0]); return 2; }
    memset(&cfg, 0, sizeof(cfg));
    cfg.H = H; cfg.W = W;
    cfg.in_format.container = FLDR_PACK10_V210;
    cfg.in_format.matrix = FLDR_PACK10_BT709;
    cfg.in_format.range = FLDR_PACK10_LIMITED;
    cfg.in_format.depth = 10;
    for (k = 5; k < argc; ++k) {
        if (k == 5 && !strcmp(argv[k], "v210")) cfg.in_format.container = FLDR_PACK10_V210;
        else if (k == 5 && !strcmp(argv[k], "y210")) cfg.in_format.container = FLDR_PACK10_Y210;
        else if (k == 5 && !strcmp(argv[k], "y410")) cfg.in_format.container = FLDR_PACK10_Y410;
        else if (!strcmp(argv[k], "bt601")) cfg.in_format.matrix = FLDR_PACK10_BT601;
        else if (!strcmp(argv[k], "bt709")) cfg.in_format.matrix = FLDR_PACK10_BT709;
        else if (!strcmp(argv[k], "full")) cfg.in_format.range = FLDR_PACK10_FULL;
        else { usage(argv[0]); return 2; }
    }
    cfg.out_format = cfg.in_format;
    n_t = factor - 1;
    cfg.n_t = n_t;                                     /* t = NULL: k / FACTOR, k = 1 .. FACTOR - 1 */
    pitch = pitch_of(cfg.in_format.container, W);
    fsize = (size_t)pitch * (size_t)H;
    frame = (uint8_t*)malloc(fsize);
    obuf = (uint8_t*)calloc(fsize, (size_t)n_t);       /* zero: the library never writes between a row's end and its pitch */
    outs = (fldr_pack10_frame*)malloc(sizeof(fldr_pack10_frame) * (size_t)n_t);
    if (!frame || !obuf || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (k = 0; k < n_t; ++k) outs[k] = frame_at(obuf + fsize * (size_t)k, pitch);
    in = frame_at(frame, pitch);
    memset(&mcfg, 0, sizeof(mcfg));
    rc = fldr_model_create_npz(argv[1], &mcfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    rc = fldr_pack10_session_create(model, &cfg, &s);
    if (rc) { fprintf(stderr, "fldr_pack10_session_create: %s (%d)\n", fldr_pack10_error_string(rc), rc); fldr_model_destroy(model); return 1; }
    while (fread(frame, 1, fsize, stdin) == fsize) {
        rc = fldr_pack10_session_push(s, &in, outs, &n_out);
        if (rc) { fprintf(stderr, "fldr_pack10_session_push: %s (%d)\n", fldr_pack10_error_string(rc), rc); status = 1; break; }
        if (!first && n_out != n_t) { fprintf(stderr, "unexpected output count %d\n", n_out); status = 1; break; }
        if (n_out > 0 && fwrite(obuf, fsize, (size_t)n_out, stdout) != (size_t)n_out) { status = 1; break; }
        if (fwrite(frame, 1, fsize, stdout) != fsize) { status = 1; break; }
        first = 0;
    }
    if (!status && ferror(stdin)) { fprintf(stderr, "read error\n"); status = 1; }
    if (fflush(stdout)) status = 1;
    fldr_pack10_session_destroy(s);
    fldr_model_destroy(model);
    free(frame); free(obuf); free(outs);
    return status;
}
