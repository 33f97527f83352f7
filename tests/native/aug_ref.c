/*
 * aug_ref.c -- TEST INFRASTRUCTURE ONLY (never linked by the product).
 *
 * A small driver, written for this repository, around the reference's own compiled load_data_detection (data.c:664-714 of
 * oracle/_ref/libdarknet_ref.so).  The reference's image.c is not in that library (it does not compile without OpenCV), so
 * the symbols load_data_detection needs from it are DEFINED HERE as recording stubs and exported from the executable
 * (-rdynamic), where the shared object's unresolved references bind to them:
 *     load_image_color      a blank image of the size the list names for that path; notes which path was chosen
 *     crop_image            records (dx, dy, w, h), allocates
 *     resize_image          allocates
 *     flip_image            records that it was called
 *     random_distort_image  makes its three draws through the reference's own rand_uniform_strong / rand_scale, records them
 *     free_image
 * rand() is interposed the same way (it forwards to libc's, found with dlsym): the values drawn between an image's
 * random_distort_image and the next load_image_color are the reference's randomize_boxes draws, logged raw.
 * Everything else -- get_random_paths, the window arithmetic, read_boxes, randomize_boxes, correct_boxes,
 * fill_truth_detection -- is the reference's compiled code, called whole.
 *
 *   aug_ref <list> <seed> <n> <w> <h> <jitter> <hue> <saturation> <exposure> <out>
 *       <list>: one line per path, "<path> <ow> <oh>"; the label file of a path is where the reference looks for it
 *       (images -> labels, .jpg -> .txt).  srand(seed), one load_data_detection(n, paths, m, w, h, 30, 20, ...), then one
 *       line per image to <out>:
 *           path pleft ptop swidth sheight flip dhue dsat dexp nswaps swap_0 .. | 150 truth words
 *       floats as the hexadecimal of their bits.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "data.h"
#include "image.h"
#include "utils.h"

int gpu_index = -1;      /* cuda.h: defined by the reference's CLI */

#define MAX_PATHS 64
#define MAX_IMAGES 256
#define MAX_DRAWS 256

static char *g_paths[MAX_PATHS];
static int g_ow[MAX_PATHS], g_oh[MAX_PATHS], g_m;

typedef struct {
    int path, dx, dy, w, h, flip, ndraws;
    float dhue, dsat, dexp;
    int draws[MAX_DRAWS];
} record;
static record g_rec[MAX_IMAGES];
static int g_cur = -1, g_log_draws;

int rand(void)
{
    static int (*real)(void);
    int v;
    if (!real) real = (int (*)(void))dlsym(RTLD_NEXT, "rand");
    v = real();
    if (g_log_draws && g_cur >= 0 && g_rec[g_cur].ndraws < MAX_DRAWS) g_rec[g_cur].draws[g_rec[g_cur].ndraws++] = v;
    return v;
}

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
    g_log_draws = 0;
    for (i = 0; i < g_m; ++i) if (!strcmp(filename, g_paths[i])) break;
    if (i == g_m || g_cur + 1 >= MAX_IMAGES) { fprintf(stderr, "aug_ref: unexpected path %s\n", filename); exit(2); }
    ++g_cur;
    memset(&g_rec[g_cur], 0, sizeof g_rec[g_cur]);
    g_rec[g_cur].path = i;
    return blank(g_ow[i], g_oh[i], 3);
}

image crop_image(image im, int dx, int dy, int w, int h)
{
    record *r = &g_rec[g_cur];
    r->dx = dx; r->dy = dy; r->w = w; r->h = h;
    return blank(w > 0 ? w : 1, h > 0 ? h : 1, im.c);
}

image resize_image(image im, int w, int h) { return blank(w, h, im.c); }

void flip_image(image a) { g_rec[g_cur].flip = 1; }

void random_distort_image(image im, float hue, float saturation, float exposure)
{
    record *r = &g_rec[g_cur];
    r->dhue = rand_uniform_strong(-hue, hue);
    r->dsat = rand_scale(saturation);
    r->dexp = rand_scale(exposure);
    g_log_draws = 1;         /* what follows until the next image are randomize_boxes' draws */
}

void free_image(image m) { free(m.data); }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
    FILE *f;
    char path[4096];
    int ow, oh, i, k, seed, n, w, h;
    float jitter, hue, saturation, exposure;
    data d;
    if (argc != 11) { fprintf(stderr, "usage: aug_ref <list> <seed> <n> <w> <h> <jitter> <hue> <saturation> <exposure> <out>\n"); return 2; }
    f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    while (g_m < MAX_PATHS && fscanf(f, "%4095s %d %d", path, &ow, &oh) == 3) {
        g_paths[g_m] = strdup(path); g_ow[g_m] = ow; g_oh[g_m] = oh; ++g_m;
    }
    fclose(f);
    seed = atoi(argv[2]); n = atoi(argv[3]); w = atoi(argv[4]); h = atoi(argv[5]);
    jitter = atof(argv[6]); hue = atof(argv[7]); saturation = atof(argv[8]); exposure = atof(argv[9]);
    if (n > MAX_IMAGES) return 2;
    srand(seed);
    d = load_data_detection(n, g_paths, g_m, w, h, 30, 20, jitter, hue, saturation, exposure);
    g_log_draws = 0;
    if (g_cur + 1 != n) { fprintf(stderr, "aug_ref: %d images loaded, %d asked for\n", g_cur + 1, n); return 2; }
    f = fopen(argv[10], "w");
    if (!f) { perror(argv[10]); return 2; }
    for (i = 0; i < n; ++i) {
        const record *r = &g_rec[i];
        fprintf(f, "%d %d %d %d %d %d %08x %08x %08x %d", r->path, r->dx, r->dy, r->w, r->h, r->flip, bits(r->dhue), bits(r->dsat),
                bits(r->dexp), r->ndraws);
        for (k = 0; k < r->ndraws; ++k) fprintf(f, " %d", r->draws[k]);
        fprintf(f, " |");
        for (k = 0; k < 150; ++k) fprintf(f, " %08x", bits(d.y.vals[i][k]));
        fprintf(f, "\n");
    }
    fclose(f);
    return 0;
}
