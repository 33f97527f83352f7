/*
 * aug_cls_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * A small driver, written for this repository, around the reference's own compiled load_data_augment (data.c:870-879 of
 * oracle/_ref/libdarknet_ref.so), run WHOLE: get_random_paths, load_image_augment_paths' per-image call order with the flip
 * draw between the two image calls, load_labels_paths with fill_truth and fill_hierarchy.  The reference's image.c is not
 * in that library (it does not compile without OpenCV), so the symbols that function needs from it are DEFINED HERE as
 * recording stubs and exported from the executable (-rdynamic), where the shared object's unresolved references bind:
 *     load_image_color      a blank image of the size the list names for that path; notes which path was chosen
 *     random_augment_image  makes its five draws through the reference's own compiled rand_scale / rand_int / rand_uniform
 *                           (utils.c), in the order and with the arithmetic of image.c:1686-1700 RESTATED in this
 *                           project's words (that function has no compiled form here), and records what it would hand to
 *                           rotate_crop_image
 *     flip_image            records that it was called
 *     random_distort_image  its three draws through the compiled rand_uniform_strong / rand_scale, recorded
 *     free_image
 * Pinned to compiled code by this: the rand primitives, the sequence around them, the paths, the label and hierarchy rows.
 * Restated: the order of the five and the three draws inside the two stubs and the arithmetic between them.
 *
 *   aug_cls_ref <list> <labels> <tree | -> <seed> <n> <min> <max> <size> <angle> <aspect> <hue> <saturation> <exposure> <out>
 *       <list>: one line per path, "<path> <ow> <oh>" (the files are never opened); <labels>: one name per line; <tree>: the
 *       reference's tree file, or - for none.  srand(seed), one load_data_augment(paths, n, m, labels, k, tree, ...), then
 *       one line per image to <out>:
 *           path aspect scale rad dx dy flip dhue dsat dexp | k truth words
 *       floats as the hexadecimal of their bits.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "data.h"
#include "image.h"
#include "tree.h"
#include "utils.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

#define MAX_PATHS 64
#define MAX_IMAGES 256
#define MAX_LABELS 64

static char *g_paths[MAX_PATHS];
static int g_ow[MAX_PATHS], g_oh[MAX_PATHS], g_m;

typedef struct {
    int path, flip;
    float aspect, scale, rad, dx, dy, dhue, dsat, dexp;
} record;
static record g_rec[MAX_IMAGES];
static int g_cur = -1;

static image blank(int w, int h, int c)
{
    image im;
    im.w = w; im.h = h; im.c = c;
    im.data = calloc((size_t)w * h * c, sizeof(float));
    return im;
}

image load_image_color(char *filename, int w, int h)
{
    int i;
    for (i = 0; i < g_m; ++i) if (!strcmp(filename, g_paths[i])) break;
    if (i == g_m || g_cur + 1 >= MAX_IMAGES) { fprintf(stderr, "aug_cls_ref: unexpected path %s\n", filename); exit(2); }
    ++g_cur;
    memset(&g_rec[g_cur], 0, sizeof g_rec[g_cur]);
    g_rec[g_cur].path = i;
    return blank(g_ow[i], g_oh[i], 3);
}

/* the frame's shorter side after the aspect stretch sets the scale; the crop may slide by half of what the scaled frame
 * has beyond `size`, nothing when it is narrower */
image random_augment_image(image im, float angle, float aspect, int low, int high, int size)
{
    record *r = &g_rec[g_cur];
    float stretch = rand_scale(aspect);
    int side = rand_int(low, high);
    int shorter = (im.h < im.w * stretch) ? im.h : im.w * stretch;
    float scale = (float)side / shorter;
    float rad = rand_uniform(-angle, angle) * TWO_PI / 360.;
    float room_x = (im.w * scale / stretch - size) / 2.;
    float room_y = (im.h * scale - size) / 2.;
    if (room_x < 0) room_x = 0;
    if (room_y < 0) room_y = 0;
    r->aspect = stretch; r->scale = scale; r->rad = rad;
    r->dx = rand_uniform(-room_x, room_x);
    r->dy = rand_uniform(-room_y, room_y);
    return blank(size, size, im.c);
}

void flip_image(image a) { g_rec[g_cur].flip = 1; }

void random_distort_image(image im, float hue, float saturation, float exposure)
{
    record *r = &g_rec[g_cur];
    r->dhue = rand_uniform_strong(-hue, hue);
    r->dsat = rand_scale(saturation);
    r->dexp = rand_scale(exposure);
}

void free_image(image m) { free(m.data); }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
    FILE *f;
    char path[4096], *labels[MAX_LABELS];
    int ow, oh, i, j, k = 0, seed, n, lo, hi, size;
    float angle, aspect, hue, saturation, exposure;
    tree *hier = NULL;
    data d;
    if (argc != 15) { fprintf(stderr, "usage: aug_cls_ref <list> <labels> <tree|-> <seed> <n> <min> <max> <size> <angle> <aspect> <hue> <saturation> <exposure> <out>\n"); return 2; }
    f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    while (g_m < MAX_PATHS && fscanf(f, "%4095s %d %d", path, &ow, &oh) == 3) {
        g_paths[g_m] = strdup(path); g_ow[g_m] = ow; g_oh[g_m] = oh; ++g_m;
    }
    fclose(f);
    f = fopen(argv[2], "r");
    if (!f) { perror(argv[2]); return 2; }
    while (k < MAX_LABELS && fscanf(f, "%4095s", path) == 1) labels[k++] = strdup(path);
    fclose(f);
    if (strcmp(argv[3], "-")) hier = read_tree(argv[3]);
    seed = atoi(argv[4]); n = atoi(argv[5]); lo = atoi(argv[6]); hi = atoi(argv[7]); size = atoi(argv[8]);
    angle = atof(argv[9]); aspect = atof(argv[10]); hue = atof(argv[11]); saturation = atof(argv[12]); exposure = atof(argv[13]);
    if (n > MAX_IMAGES || (hier && hier->n != k)) return 2;
    srand(seed);
    d = load_data_augment(g_paths, n, g_m, labels, k, hier, lo, hi, size, angle, aspect, hue, saturation, exposure);
    if (g_cur + 1 != n) { fprintf(stderr, "aug_cls_ref: %d images loaded, %d asked for\n", g_cur + 1, n); return 2; }
    f = fopen(argv[14], "w");
    if (!f) { perror(argv[14]); return 2; }
    for (i = 0; i < n; ++i) {
        const record *r = &g_rec[i];
        fprintf(f, "%d %08x %08x %08x %08x %08x %d %08x %08x %08x |", r->path, bits(r->aspect), bits(r->scale), bits(r->rad), bits(r->dx),
                bits(r->dy), r->flip, bits(r->dhue), bits(r->dsat), bits(r->dexp));
        for (j = 0; j < k; ++j) fprintf(f, " %08x", bits(d.y.vals[i][j]));
        fprintf(f, "\n");
    }
    fclose(f);
    return 0;
}
