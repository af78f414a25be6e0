/* Stand-alone check of soc_png_encode_bits under the host sanitizers: every size and mask kind of tests/test_png_bits.py, the
 * smallest legal row stride (so a read past ceil(w / 8) bytes of the last row lands outside the allocation), a wider stride and
 * garbage in the padding bits; each file must equal what soc_png_encode_u8(binarize = 1) writes for the unpacked mask.
 *
 *   gcc -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
 *       -o /tmp/png_bits_sanitize tools/png_bits_sanitize.c neurips2023_soc_amd/csrc_host/png_runs.c && /tmp/png_bits_sanitize
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "soc_host.h"

static uint32_t rng_state = 12345;
static uint32_t rnd(void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int pixel(int kind, int y, int x, int h, int w) {
    switch (kind) {
        case 0: { const long dy = 2 * y - h, dx = 2 * x - w, r = (h < w ? h : w) * 2 / 3 + 2;
                  return dy * dy + dx * dx < r * r || x % 11 == 3 || y % 13 == 5; }
        case 1: return 0;
        case 2: return 1;
        case 3: return (int)(rnd() & 1);
        case 4: return (y + x) % 2 == 0;
        case 5: return y == h - 1 && x == w - 1;
        default: return ((y / 2) * 31 + x / 5) % 3 == 0;          /* rows equal to the row above */
    }
}

static int check(int h, int w, int kind, long stride, int garbage) {
    const size_t cap = soc_png_bound(h, w);
    uint8_t* mask = malloc((size_t)h * w);
    uint8_t* bits = malloc((size_t)h * stride);                    /* exactly h * stride bytes: nothing to spare behind the last row */
    uint8_t* a = malloc(cap);
    uint8_t* b = malloc(cap);
    if (!mask || !bits || !a || !b) return 1;
    memset(bits, garbage ? 0xFF : 0, (size_t)h * stride);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int v = pixel(kind, y, x, h, w);
            mask[(size_t)y * w + x] = (uint8_t)v;
            uint8_t* byte = bits + (size_t)y * stride + x / 8;
            *byte = (uint8_t)((*byte & ~(1u << (x % 8))) | ((unsigned)v << (x % 8)));
        }
    const long na = soc_png_encode_u8(mask, h, w, w, 1, NULL, 0, a, cap);
    const long nb = soc_png_encode_bits(bits, h, w, stride, b, cap);
    const int bad = na <= 0 || na != nb || memcmp(a, b, (size_t)na) != 0;
    if (bad) printf("MISMATCH h=%d w=%d kind=%d stride=%ld garbage=%d (%ld vs %ld bytes)\n", h, w, kind, stride, garbage, na, nb);
    free(mask); free(bits); free(a); free(b);
    return bad;
}

int main(void) {
    static const int sizes[8][2] = {{1, 1}, {1, 7}, {3, 5}, {7, 300}, {64, 64}, {65, 129}, {361, 641}, {720, 1280}};
    int bad = 0, n = 0;
    for (int s = 0; s < 8; ++s)
        for (int kind = 0; kind < 7; ++kind) {
            const int h = sizes[s][0], w = sizes[s][1];
            const long tight = (w + 7) / 8, padded = 8 * ((w + 63) / 64);
            bad += check(h, w, kind, tight, 0);
            bad += check(h, w, kind, tight, 1);                    /* garbage in the bits of the last byte at x >= w */
            bad += check(h, w, kind, padded, 1);                   /* ... and in the padding bytes of the 64-bit rows */
            bad += check(h, w, kind, padded + 24, 1);              /* a wider stride */
            n += 4;
        }
    uint8_t one = 0, out[2048];
    bad += soc_png_encode_bits(NULL, 1, 1, 1, out, sizeof out) != -1;
    bad += soc_png_encode_bits(&one, 1, 9, 1, out, sizeof out) != -1;
    bad += soc_png_encode_bits(&one, 1, 1, 1, out, 16) != -2;
    printf("%d encodes, %d failures\n", n, bad);
    return bad != 0;
}
