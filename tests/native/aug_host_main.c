/*
 * aug_host_main.c -- TEST INFRASTRUCTURE ONLY: a stand-alone program around csrc/host/y2_aug.c, the device-free half of the
 * detection loader, meant to be built with -fsanitize=address,undefined (tests/test_aug_host.py).  Frames and the packed
 * buffer are heap blocks of exactly their size, so a read or write past either is reported.  It packs windows that hang
 * over every edge of frames with and without a padded pitch and 3 or 4 bytes per pixel, checks every packed byte against
 * the frame and that every tap of crop_image lands inside the packed rectangle, and runs the draws and the truth.
 * Prints "aug_host ok" and returns 0, or says what differs and returns 1.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

void y2_fail(const char *fmt, ...)          /* the engine's, which y2_aug.c reports through */
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

static int clampi(long a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : (int)a); }

typedef struct { int w, h, c, pad; } frame_spec;
typedef struct { int pleft, ptop, swidth, sheight; } window;

static int run(const frame_spec *fs, const window *wins, int n)
{
    const int step = fs->w * fs->c + fs->pad;
    const size_t frame_bytes = (size_t)step * (fs->h - 1) + (size_t)fs->w * fs->c;     /* the last row has no padding behind it */
    unsigned char *frame = malloc(frame_bytes), *pixels;
    y2_aug_item *items = calloc(n, sizeof *items);
    y2h_aug *desc = malloc((size_t)n * sizeof *desc);
    float boxes[3][5] = { { 1, .5f, .5f, .2f, .3f }, { 0, 0, 0, .1f, .1f }, { 4, .02f, .9f, .03f, .1f } };
    int swaps[3] = { 2, 0, 1 };
    float truth[150];
    size_t bytes, i;
    int k, x, y, bad = 0;
    for (i = 0; i < frame_bytes; ++i) frame[i] = (unsigned char)(i * 131 + 7);
    for (k = 0; k < n; ++k) {
        y2_aug_item *it = &items[k];
        it->data = frame; it->h = fs->h; it->w = fs->w; it->c = fs->c; it->step = step;
        it->pleft = wins[k].pleft; it->ptop = wins[k].ptop; it->swidth = wins[k].swidth; it->sheight = wins[k].sheight;
        it->flip = k & 1; it->dhue = .1f; it->dsat = 1.5f; it->dexp = 1.f / 1.5f;
        it->boxes = &boxes[0][0]; it->nboxes = 3; it->swaps = (k & 2) ? swaps : NULL;
    }
    if (y2_aug_check("aug_host", items, n) != 0) return 1;
    bytes = y2_aug_pack_bytes(items, n);
    pixels = malloc(bytes ? bytes : 1);
    y2_aug_pack(items, n, 13, 11, desc, pixels);
    for (k = 0; k < n && !bad; ++k) {
        const y2h_aug *d = &desc[k];
        if (d->src < 0 || (size_t)d->src + (size_t)d->pitch * d->rh > bytes || d->pitch != d->rw * d->c) { fprintf(stderr, "item %d: rectangle outside the packed buffer\n", k); bad = 1; break; }
        for (y = 0; y < d->rh && !bad; ++y)
            if (memcmp(pixels + d->src + (size_t)y * d->pitch, frame + (size_t)(d->y0 + y) * step + (size_t)d->x0 * fs->c, (size_t)d->rw * d->c)) {
                fprintf(stderr, "item %d: packed row %d differs from the frame\n", k, y);
                bad = 1;
            }
        /* the clamp is monotonic: the window's corners bound every tap; small windows are walked whole */
        for (y = 0; y < d->sheight && !bad; y += (d->sheight > 64 && y == 0) ? d->sheight - 1 : 1)
            for (x = 0; x < d->swidth; x += (d->swidth > 64 && x == 0) ? d->swidth - 1 : 1) {
                const int r = clampi((long)y + d->ptop, 0, d->oh - 1) - d->y0, c = clampi((long)x + d->pleft, 0, d->ow - 1) - d->x0;
                if (r < 0 || r >= d->rh || c < 0 || c >= d->rw) { fprintf(stderr, "item %d: tap (%d, %d) falls outside the packed rectangle\n", k, x, y); bad = 1; break; }
            }
        if (y2_aug_truth_detection(&items[k], 30, truth) != 0) bad = 1;
    }
    free(pixels); free(desc); free(items); free(frame);
    return bad;
}

int main(void)
{
    static const frame_spec frames[] = { { 37, 53, 3, 0 }, { 37, 53, 3, 5 }, { 7, 5, 4, 0 }, { 1, 9, 3, 2 }, { 9, 1, 3, 0 }, { 500, 375, 3, 0 } };
    size_t f;
    int swaps[40], paths[8], k;
    y2_aug_item item;
    for (f = 0; f < sizeof frames / sizeof frames[0]; ++f) {
        const int w = frames[f].w, h = frames[f].h;
        const window wins[] = {
            { 0, 0, w, h },                         /* the whole frame */
            { -7, -9, w + 14, h + 18 },             /* over every edge at once */
            { -w, 0, w, h }, { w, 0, w, h },        /* wholly left of it, wholly right of it */
            { 0, -h, w, h }, { 0, h, w, h },        /* wholly above, wholly below */
            { w / 2, h / 2, w, h },                 /* past right and bottom */
            { -3, -2, 4, 3 },                       /* past left and top */
            { w - 1, h - 1, 1, 1 }, { 0, 0, 1, 1 }, /* one pixel */
            { -1000000, -1000000, 2000001, 2000001 },
            { 2147483000, 2147483000, 600, 600 },   /* pleft + swidth does not fit an int */
        };
        if (run(&frames[f], wins, (int)(sizeof wins / sizeof wins[0])) != 0) { fprintf(stderr, "frame %zu failed\n", f); return 1; }
    }
    srand(11);
    y2_aug_random_paths(8, 5, paths);
    memset(&item, 0, sizeof item);
    for (k = 0; k < 8; ++k) y2_aug_draw_detection(500, 375, .3f, .1f, 1.5f, 1.5f, 35, &item, swaps);
    y2_aug_draw_detection(37, 53, .2f, 0, 1, 1, 0, &item, NULL);
    if (y2_aug_random_dim() % 32 != 0) return 1;
    puts("aug_host ok");
    return 0;
}
