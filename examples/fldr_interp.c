/* fldr_interp — interpolate one frame between two images with the C model API (include/fldr_model.h); no Python, no HIP headers.
 *
 *   fldr_interp weights.npz a.ppm b.ppm t out.ppm
 *
 * a.ppm, b.ppm: binary PPM (P6, maxval 255) of the same size; t in [0, 1]; out.ppm: the frame at time t.  Device 0, the shipped
 * configuration (5 pyramid levels below the frame).  Build: cc -std=c99 -Iinclude examples/fldr_interp.c -Lfldr-vfi_amd -l:libfldr_model.so */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fldr_model.h"

static int next_token(FILE* f, long* v) {
    int c = fgetc(f);
    for (;;) {
        while (c == ' ' || c == '\t' || c == '\n' || c == '\r') c = fgetc(f);
        if (c != '#') break;
        while (c != '\n' && c != EOF) c = fgetc(f);
    }
    if (c < '0' || c > '9') return -1;
    *v = 0;
    while (c >= '0' && c <= '9') { *v = *v * 10 + (c - '0'); if (*v > 1000000) return -1; c = fgetc(f); }
    return 0;                                          /* the single whitespace after the token is consumed */
}

static uint8_t* read_ppm(const char* path, int* W, int* H) {
    FILE* f = fopen(path, "rb");
    long w, h, mx;
    uint8_t* px = NULL;
    if (!f) { fprintf(stderr, "%s: cannot open\n", path); return NULL; }
    if (fgetc(f) != 'P' || fgetc(f) != '6' || next_token(f, &w) || next_token(f, &h) || next_token(f, &mx) || mx != 255 || w < 2 || h < 2) {
        fprintf(stderr, "%s: not a binary 8-bit PPM (P6, maxval 255)\n", path);
    } else {
        px = (uint8_t*)malloc((size_t)w * (size_t)h * 3);
        if (px && fread(px, 3, (size_t)w * (size_t)h, f) != (size_t)w * (size_t)h) {
            fprintf(stderr, "%s: truncated\n", path);
            free(px);
            px = NULL;
        }
        *W = (int)w;
        *H = (int)h;
    }
    fclose(f);
    return px;
}

int main(int argc, char** argv) {
    fldr_model_config cfg;
    fldr_model* model = NULL;
    uint8_t *a, *b, *out;
    int wa, ha, wb, hb, rc;
    float t;
    FILE* f;
    if (argc != 6) {
        fprintf(stderr, "usage: %s weights.npz a.ppm b.ppm t out.ppm\n", argv[0]);
        return 2;
    }
    t = (float)atof(argv[4]);
    a = read_ppm(argv[2], &wa, &ha);
    b = read_ppm(argv[3], &wb, &hb);
    if (!a || !b) return 1;
    if (wa != wb || ha != hb) { fprintf(stderr, "the two frames differ in size\n"); return 1; }
    memset(&cfg, 0, sizeof(cfg));
    rc = fldr_model_create_npz(argv[1], &cfg, &model);
    if (rc) { fprintf(stderr, "fldr_model_create_npz: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    out = (uint8_t*)malloc((size_t)wa * (size_t)ha * 3);
    rc = out ? fldr_model_interpolate_host(model, a, b, ha, wa, 3 * (int64_t)wa, FLDR_MODEL_RGB, &t, 1, &out) : FLDR_MODEL_E_ARG;
    fldr_model_destroy(model);
    if (rc) { fprintf(stderr, "fldr_model_interpolate_host: %s (%d)\n", fldr_model_error_string(rc), rc); return 1; }
    f = fopen(argv[5], "wb");
    if (!f) { fprintf(stderr, "%s: cannot create\n", argv[5]); return 1; }
    fprintf(f, "P6\n%d %d\n255\n", wa, ha);
    rc = fwrite(out, 3, (size_t)wa * (size_t)ha, f) == (size_t)wa * (size_t)ha ? 0 : 1;
    if (fclose(f) || rc) { fprintf(stderr, "%s: write failed\n", argv[5]); return 1; }
    free(a); free(b); free(out);
    return 0;
}
