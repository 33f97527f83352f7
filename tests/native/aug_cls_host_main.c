/*
 * aug_cls_host_main.c -- TEST INFRASTRUCTURE ONLY: a stand-alone program around csrc/host/y2_aug.c, the device-free half of
 * the classifier loader, meant to be built with -fsanitize=address,undefined (tests/test_aug_cls_host.py).  Frames and the
 * packed buffer are heap blocks of exactly their size, so a read or write past either is reported.  It packs crops that are
 * rotated by every quarter and by odd angles, stretched, shrunk until they hang over every edge and pushed wholly out of
 * the frame, of frames with and without a padded pitch and 3 or 4 bytes per pixel; checks every packed byte against the
 * frame and that every tap of every output pixel lands inside the packed rectangle; runs the draws (a frame whose
 * shorter side truncates to 0 among them) and y2_aug_labels flat, with a tree, with no match and with NULL names.
 * Prints "aug_cls_host ok" and returns 0, or says what differs and returns 1.
 */
#include <math.h>
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

/* floorf as an int the way get_pixel_extend sees it: far outside the frame every value clamps alike */
static long tap_of(float v)
{
    float f = floorf(v);
    if (!(f >= -4)) return -4;
    if (f > 1e6f) return 1000000;
    return (long)f;
}

typedef struct { int w, h, c, pad; } frame_spec;
typedef struct { float deg, aspect, scale, dx, dy; } crop;

static int run(const frame_spec *fs, const crop *crops, int n, int size)
{
    const int step = fs->w * fs->c + fs->pad;
    const size_t frame_bytes = (size_t)step * (fs->h - 1) + (size_t)fs->w * fs->c;     /* the last row has no padding behind it */
    unsigned char *frame = malloc(frame_bytes), *pixels;
    y2_aug_cls_item *items = calloc(n, sizeof *items);
    y2h_aug_cls *desc = malloc((size_t)n * sizeof *desc);
    size_t bytes, i;
    int k, x, y, bad = 0;
    for (i = 0; i < frame_bytes; ++i) frame[i] = (unsigned char)(i * 131 + 7);
    for (k = 0; k < n; ++k) {
        y2_aug_cls_item *it = &items[k];
        it->data = frame; it->h = fs->h; it->w = fs->w; it->c = fs->c; it->step = step;
        it->aspect = crops[k].aspect; it->scale = crops[k].scale; it->rad = crops[k].deg * 6.2831853071795864769 / 360.;
        it->dx = crops[k].dx; it->dy = crops[k].dy;
        it->flip = k & 1; it->dhue = .1f; it->dsat = 1.5f; it->dexp = 1.f / 1.5f;
    }
    if (y2_aug_cls_check("aug_cls_host", items, n) != 0) return 1;
    bytes = y2_aug_cls_pack_bytes(items, n, size);
    pixels = malloc(bytes ? bytes : 1);
    y2_aug_cls_pack(items, n, size, desc, pixels);
    for (k = 0; k < n && !bad; ++k) {
        const y2h_aug_cls *d = &desc[k];
        const double half = size / 2.;
        if (d->src < 0 || (size_t)d->src + (size_t)d->pitch * d->rh > bytes || d->pitch != d->rw * d->c || d->rw < 1 || d->rh < 1 ||
            d->x0 < 0 || d->y0 < 0 || d->x0 + d->rw > fs->w || d->y0 + d->rh > fs->h) {
            fprintf(stderr, "item %d: rectangle outside the frame or the packed buffer\n", k);
            bad = 1;
            break;
        }
        for (y = 0; y < d->rh && !bad; ++y)
            if (memcmp(pixels + d->src + (size_t)y * d->pitch, frame + (size_t)(d->y0 + y) * step + (size_t)d->x0 * fs->c, (size_t)d->rw * d->c)) {
                fprintf(stderr, "item %d: packed row %d differs from the frame\n", k, y);
                bad = 1;
            }
        for (y = 0; y < size && !bad; ++y)
            for (x = 0; x < size; ++x) {
                const double ux = (x - half) / d->s * d->aspect + d->ax, vy = (y - half) / d->s + d->ay;
                const float rx = (float)(d->cosr * ux - d->sinr * vy + (double)d->cx);
                const float ry = (float)(d->sinr * ux + d->cosr * vy + (double)d->cy);
                const long ix = tap_of(rx), iy = tap_of(ry);
                const int c0 = clampi(ix, 0, d->ow - 1) - d->x0, c1 = clampi(ix + 1, 0, d->ow - 1) - d->x0;
                const int r0 = clampi(iy, 0, d->oh - 1) - d->y0, r1 = clampi(iy + 1, 0, d->oh - 1) - d->y0;
                if (c0 < 0 || c1 >= d->rw || r0 < 0 || r1 >= d->rh) {
                    fprintf(stderr, "item %d: a tap of (%d, %d) falls outside the packed rectangle\n", k, x, y);
                    bad = 1;
                    break;
                }
            }
    }
    free(pixels); free(desc); free(items); free(frame);
    return bad;
}

static int labels(void)
{
    char *names[8] = { "animal", "vehicle", "cat", "dog", "car", "bus", "tabby", "siamese" };
    int parent[8] = { -1, -1, 0, 0, 1, 1, 2, 2 }, group_size[4] = { 2, 2, 2, 2 };
    tree t;
    float *truth = malloc(8 * sizeof(float));
    int bad = 0;
    memset(&t, 0, sizeof t);
    t.n = 8; t.parent = parent; t.groups = 4; t.group_size = group_size;
    bad |= y2_aug_labels("set/tabby_a.jpg", names, 8, NULL, truth) != 1 || truth[6] != 1 || truth[2] != 0;
    bad |= y2_aug_labels("set/tabby_a.jpg", names, 8, &t, truth) != 1 || truth[6] != 1 || truth[2] != 1 || truth[0] != 1 || truth[4] != -1234;
    bad |= y2_aug_labels("set/plain_b.jpg", names, 8, &t, truth) != 0 || truth[0] != -1234 || truth[7] != -1234;
    bad |= y2_aug_labels("set/dog_bus_c.jpg", names, 8, &t, truth) != 2 || truth[3] != 1 || truth[5] != 1 || truth[6] != -1234;
    bad |= y2_aug_labels("", names, 8, NULL, truth) != 0;
    names[3] = NULL;
    bad |= y2_aug_labels("set/dog_bus_c.jpg", names, 8, NULL, truth) != 1;
    bad |= y2_aug_labels("x", names, 0, NULL, truth) != 0;
    free(truth);
    if (bad) fprintf(stderr, "y2_aug_labels: a row differs\n");
    return bad;
}

int main(void)
{
    static const frame_spec frames[] = { { 37, 53, 3, 0 }, { 37, 53, 3, 5 }, { 7, 5, 4, 0 }, { 1, 9, 3, 2 }, { 9, 1, 3, 0 }, { 1, 1, 3, 0 }, { 500, 375, 3, 0 } };
    static const int sizes[] = { 1, 5, 8, 33 };
    size_t f, s;
    int paths[8], k;
    y2_aug_cls_item item;
    for (f = 0; f < sizeof frames / sizeof frames[0]; ++f)
        for (s = 0; s < sizeof sizes / sizeof sizes[0]; ++s) {
            const float w = frames[f].w, h = frames[f].h;
            const crop crops[] = {
                { 0, 1, 1, 0, 0 }, { 90, 1, 1, 0, 0 }, { 180, 1, 1, 0, 0 }, { -90, 1, 1, 0, 0 }, { 7, .75f, 1.3f, 2, -3 }, { -7, 4.f / 3, .7f, -2, 3 },
                { 45, 1, .05f, 0, 0 }, { 133, 2, .2f, 0, 0 },                           /* over every edge at once */
                { 0, 1, 1, 4 * w, 0 }, { 0, 1, 1, -4 * w, 0 }, { 0, 1, 1, 0, 4 * h }, { 0, 1, 1, 0, -4 * h },     /* wholly beside the frame */
                { 30, .5f, 4, w, h }, { -150, 1, 4, -w, -h },
                { 0, 1, 1e-30f, 0, 0 }, { 11, 1, 1e30f, 0, 0 }, { 0, 1, 1, 1e30f, -1e30f },       /* coordinates beyond any int */
            };
            if (run(&frames[f], crops, (int)(sizeof crops / sizeof crops[0]), sizes[s]) != 0) { fprintf(stderr, "frame %zu size %d failed\n", f, sizes[s]); return 1; }
        }
    if (labels() != 0) return 1;
    srand(11);
    y2_aug_random_paths(8, 5, paths);
    memset(&item, 0, sizeof item);
    for (k = 0; k < 8; ++k)
        if (y2_aug_draw_classification(500, 375, 224, 320, 224, 7, .75f, .1f, .75f, .75f, &item) != 0) return 1;
    if (y2_aug_draw_classification(37, 53, 16, 16, 16, 0, 1, 0, 1, 1, NULL) != 0) return 1;
    if (y2_aug_draw_classification(37, 0, 16, 32, 16, 0, 1, 0, 1, 1, &item) != -1) return 1;
    for (k = 0; k < 8; ++k) {               /* 1 * aspect truncates to 0 exactly when the drawn aspect is below 1 */
        item.aspect = 0;
        if (y2_aug_draw_classification(1, 53, 16, 32, 16, 0, .4f, 0, 1, 1, &item) != (item.aspect >= 1 ? 0 : -1)) return 1;
    }
    puts("aug_cls_host ok");
    return 0;
}
