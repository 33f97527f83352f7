/*
 * The host half of the detection loader, device-free: the draws of load_data_detection (src_yolo2/data.c:664-714, utils.c:614-661)
 * in the reference's rand() order, the truth row (randomize_boxes, correct_boxes, fill_truth_detection: data.c:161-207,
 * :295-331) in the reference's float / double promotions, and the packer that lays the source pixels each window touches
 * and the y2h_aug table out for one upload.  The pixel work itself is y2h_augment_to_input (y2_augment.hip); what calls it
 * is y2_train_load_detection (y2_train.c).  Nothing here needs a device or an engine: only y2_fail.
 * The second half of the file is the same for the classifier loader (load_data_augment, data.c:870-879): the draws of
 * random_augment_image, the flip and random_distort_image, the label row of load_labels_paths, and the packer of
 * y2h_augment_cls_to_input, called by y2_train_load_classification.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

/* ---- utils.c:633-661 ---- */
static unsigned int random_gen(void) { return (unsigned int)rand(); }
static float random_float(void) { return (float)random_gen() / (float)RAND_MAX; }

static float rand_uniform_strong(float min, float max)
{
    if (max < min) { float swap = min; min = max; max = swap; }
    return (random_float() * (max - min)) + min;
}

static float rand_scale(float s)        /* utils.c:614 */
{
    float scale = rand_uniform_strong(1, s);
    if (random_gen() % 2) return scale;
    return 1. / scale;
}

void y2_aug_random_paths(int n, int m, int *out)
{
    int i;
    for (i = 0; i < n; ++i) {
        int index = random_gen() % m;
        if (out) out[i] = index;
    }
}

int y2_aug_random_dim(void)
{
    return (rand() % 10 + 10) * 32;
}

void y2_aug_draw_detection(int ow, int oh, float jitter, float hue, float saturation, float exposure, int nboxes,
                           y2_aug_item *item, int *swaps)
{
    int dw = (ow * jitter);
    int dh = (oh * jitter);
    int pleft = rand_uniform_strong(-dw, dw);
    int pright = rand_uniform_strong(-dw, dw);
    int ptop = rand_uniform_strong(-dh, dh);
    int pbot = rand_uniform_strong(-dh, dh);
    int flip = random_gen() % 2;
    float dhue = rand_uniform_strong(-hue, hue);        /* image.c:1918 random_distort_image */
    float dsat = rand_scale(saturation);
    float dexp = rand_scale(exposure);
    int i;
    for (i = 0; i < nboxes; ++i) {                      /* data.c:161 randomize_boxes */
        int index = random_gen() % nboxes;
        if (swaps) swaps[i] = index;
    }
    if (!item) return;
    item->pleft = pleft; item->ptop = ptop;
    item->swidth = ow - pleft - pright;
    item->sheight = oh - ptop - pbot;
    item->flip = flip;
    item->dhue = dhue; item->dsat = dsat; item->dexp = dexp;
    item->swaps = swaps;
}

/* ---- data.c:69-73, :135-207, :295-331 ---- */
typedef struct { int id; float x, y, w, h; float left, right, top, bottom; } box_label;

static float constrain(float min, float max, float a)
{
    if (a < min) return min;
    if (a > max) return max;
    return a;
}

static void correct_boxes(box_label *boxes, int n, float dx, float dy, float sx, float sy, int flip)
{
    int i;
    for (i = 0; i < n; ++i) {
        if (boxes[i].x == 0 && boxes[i].y == 0) {
            boxes[i].x = 999999;
            boxes[i].y = 999999;
            boxes[i].w = 999999;
            boxes[i].h = 999999;
            continue;
        }
        boxes[i].left = boxes[i].left * sx - dx;
        boxes[i].right = boxes[i].right * sx - dx;
        boxes[i].top = boxes[i].top * sy - dy;
        boxes[i].bottom = boxes[i].bottom * sy - dy;
        if (flip) {
            float swap = boxes[i].left;
            boxes[i].left = 1. - boxes[i].right;
            boxes[i].right = 1. - swap;
        }
        boxes[i].left = constrain(0, 1, boxes[i].left);
        boxes[i].right = constrain(0, 1, boxes[i].right);
        boxes[i].top = constrain(0, 1, boxes[i].top);
        boxes[i].bottom = constrain(0, 1, boxes[i].bottom);
        boxes[i].x = (boxes[i].left + boxes[i].right) / 2;
        boxes[i].y = (boxes[i].top + boxes[i].bottom) / 2;
        boxes[i].w = (boxes[i].right - boxes[i].left);
        boxes[i].h = (boxes[i].bottom - boxes[i].top);
        boxes[i].w = constrain(0, 1, boxes[i].w);
        boxes[i].h = constrain(0, 1, boxes[i].h);
    }
}

static int item_check(const char *who, const y2_aug_item *it, int i)
{
    int k;
    if (!it->data) { y2_fail("%s: item %d: data is NULL", who, i); return -1; }
    if (it->h <= 0 || it->w <= 0) { y2_fail("%s: item %d: bad frame geometry %d x %d", who, i, it->h, it->w); return -1; }
    if (it->c < 3) { y2_fail("%s: item %d: the frame has %d channels, the loader reads 3", who, i, it->c); return -1; }
    if ((long)it->step < (long)it->w * it->c) { y2_fail("%s: item %d: step %d is less than w*c = %ld", who, i, it->step, (long)it->w * it->c); return -1; }
    if (it->swidth < 1 || it->sheight < 1) { y2_fail("%s: item %d: the window is %d x %d", who, i, it->swidth, it->sheight); return -1; }
    if (it->nboxes < 0) { y2_fail("%s: item %d: nboxes is %d", who, i, it->nboxes); return -1; }
    if (it->nboxes > 0 && !it->boxes) { y2_fail("%s: item %d: %d label rows and boxes is NULL", who, i, it->nboxes); return -1; }
    for (k = 0; it->swaps && k < it->nboxes; ++k)
        if (it->swaps[k] < 0 || it->swaps[k] >= it->nboxes) {
            y2_fail("%s: item %d: swap %d is %d, outside its %d label rows", who, i, k, it->swaps[k], it->nboxes);
            return -1;
        }
    return 0;
}

int y2_aug_check(const char *who, const y2_aug_item *items, int n)
{
    int i;
    if (!items) { y2_fail("%s: no items", who); return -1; }
    for (i = 0; i < n; ++i)
        if (item_check(who, &items[i], i) != 0) return -1;
    return 0;
}

int y2_aug_truth_detection(const y2_aug_item *item, int num_boxes, float *truth)
{
    box_label *boxes;
    int i, count;
    float sx, sy, dx, dy;
    if (!item || !truth || num_boxes < 0) { y2_fail("y2_aug_truth_detection: NULL item or truth"); return -1; }
    if (item->h <= 0 || item->w <= 0) { y2_fail("y2_aug_truth_detection: bad frame geometry %d x %d", item->h, item->w); return -1; }
    if (item->nboxes < 0 || (item->nboxes > 0 && !item->boxes)) { y2_fail("y2_aug_truth_detection: %d label rows, boxes %s", item->nboxes, item->boxes ? "given" : "NULL"); return -1; }
    for (i = 0; item->swaps && i < item->nboxes; ++i)
        if (item->swaps[i] < 0 || item->swaps[i] >= item->nboxes) { y2_fail("y2_aug_truth_detection: swap %d is %d, outside its %d label rows", i, item->swaps[i], item->nboxes); return -1; }
    memset(truth, 0, (size_t)5 * num_boxes * sizeof(float));
    count = item->nboxes;
    boxes = calloc(count > 0 ? count : 1, sizeof(box_label));
    for (i = 0; i < count; ++i) {                       /* read_boxes (data.c:135) */
        const float *r = item->boxes + (size_t)5 * i;
        float x = r[1], y = r[2], w = r[3], h = r[4];
        boxes[i].id = (int)r[0];
        boxes[i].x = x;
        boxes[i].y = y;
        boxes[i].h = h;
        boxes[i].w = w;
        boxes[i].left = x - w / 2;
        boxes[i].right = x + w / 2;
        boxes[i].top = y - h / 2;
        boxes[i].bottom = y + h / 2;
    }
    for (i = 0; item->swaps && i < count; ++i) {        /* randomize_boxes (data.c:161) */
        box_label swap = boxes[i];
        int index = item->swaps[i];
        boxes[i] = boxes[index];
        boxes[index] = swap;
    }
    sx = (float)item->swidth / item->w;                 /* data.c:693-700 */
    sy = (float)item->sheight / item->h;
    dx = ((float)item->pleft / item->w) / sx;
    dy = ((float)item->ptop / item->h) / sy;
    correct_boxes(boxes, count, dx, dy, 1. / sx, 1. / sy, item->flip);
    if (count > num_boxes) count = num_boxes;
    for (i = 0; i < count; ++i) {                       /* fill_truth_detection (data.c:315-329) */
        float x = boxes[i].x, y = boxes[i].y, w = boxes[i].w, h = boxes[i].h;
        int id = boxes[i].id;
        if ((w < .01 || h < .01)) continue;             /* skipped, and its slot stays zero: the list ends here for the region layer */
        truth[i * 5 + 0] = x;
        truth[i * 5 + 1] = y;
        truth[i * 5 + 2] = w;
        truth[i * 5 + 3] = h;
        truth[i * 5 + 4] = id;
    }
    free(boxes);
    return 0;
}

/* ---- the packer ---- */
static int clamp_l(long a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : (int)a); }

/* the frame rectangle a window touches after constrain_int: columns clamp(pleft .. pleft + swidth - 1), rows likewise */
void y2_aug_rect(const y2_aug_item *it, int *x0, int *y0, int *rw, int *rh)
{
    const int xa = clamp_l(it->pleft, 0, it->w - 1), xb = clamp_l((long)it->pleft + it->swidth - 1, 0, it->w - 1);
    const int ya = clamp_l(it->ptop, 0, it->h - 1), yb = clamp_l((long)it->ptop + it->sheight - 1, 0, it->h - 1);
    *x0 = xa; *y0 = ya;
    *rw = xb - xa + 1; *rh = yb - ya + 1;
}

size_t y2_aug_pack_bytes(const y2_aug_item *items, int n)
{
    size_t bytes = 0;
    int i, x0, y0, rw, rh;
    for (i = 0; i < n; ++i) {
        y2_aug_rect(&items[i], &x0, &y0, &rw, &rh);
        bytes += (size_t)rw * rh * items[i].c;
    }
    return bytes;
}

/* desc[n] and the rectangles back to back in `pixels` (y2_aug_pack_bytes of room); descriptor offsets count from `pixels` */
void y2_aug_pack(const y2_aug_item *items, int n, int net_w, int net_h, y2h_aug *desc, unsigned char *pixels)
{
    size_t off = 0;
    int i, r;
    memset(desc, 0, (size_t)n * sizeof *desc);
    for (i = 0; i < n; ++i) {
        const y2_aug_item *it = &items[i];
        y2h_aug *d = &desc[i];
        size_t row;
        y2_aug_rect(it, &d->x0, &d->y0, &d->rw, &d->rh);
        row = (size_t)d->rw * it->c;
        d->src = (long long)off;
        d->pitch = (int)row;
        d->c = it->c;
        d->ow = it->w; d->oh = it->h;
        d->pleft = it->pleft; d->ptop = it->ptop; d->swidth = it->swidth; d->sheight = it->sheight;
        d->flip = it->flip != 0;
        d->dhue = it->dhue; d->dsat = it->dsat; d->dexp = it->dexp;
        d->w_scale = (float)(it->swidth - 1) / (net_w - 1);          /* as y2h_resize_chw */
        d->h_scale = (float)(it->sheight - 1) / (net_h - 1);
        for (r = 0; r < d->rh; ++r)
            memcpy(pixels + off + (size_t)r * row, it->data + (size_t)(d->y0 + r) * it->step + (size_t)d->x0 * it->c, row);
        off += row * d->rh;
    }
}

/* ================================================================== */
/* the classifier loader's host half (data.c:107-132, :387-444, :870)  */
/* ================================================================== */
#define Y2_TWO_PI 6.2831853071795864769252866       /* utils.h:12 */
#define Y2_SECRET_NUM -1234                         /* utils.h:11 */

static int rand_int(int min, int max)               /* utils.c:547 */
{
    if (max < min) { int s = min; min = max; max = s; }
    return (rand() % (max - min + 1)) + min;
}

static float rand_uniform(float min, float max)     /* utils.c:603 */
{
    if (max < min) { float swap = min; min = max; max = swap; }
    return ((float)rand() / RAND_MAX * (max - min)) + min;
}

int y2_aug_draw_classification(int ow, int oh, int min, int max, int size, float angle, float aspect, float hue,
                               float saturation, float exposure, y2_aug_cls_item *item)
{
    int r, m, flip;
    float scale, rad, dx, dy, dhue, dsat, dexp;
    aspect = rand_scale(aspect);                        /* image.c:1688-1700 random_augment_image */
    r = rand_int(min, max);
    m = (oh < ow * aspect) ? oh : ow * aspect;
    scale = (float)r / m;
    rad = rand_uniform(-angle, angle) * Y2_TWO_PI / 360.;
    dx = (ow * scale / aspect - size) / 2.;
    dy = (oh * scale - size) / 2.;
    if (dx < 0) dx = 0;
    if (dy < 0) dy = 0;
    dx = rand_uniform(-dx, dx);
    dy = rand_uniform(-dy, dy);
    flip = random_gen() % 2;                            /* data.c:118 */
    dhue = rand_uniform_strong(-hue, hue);              /* image.c:1918 random_distort_image */
    dsat = rand_scale(saturation);
    dexp = rand_scale(exposure);
    if (m == 0) { y2_fail("y2_aug_draw_classification: a %d x %d frame with aspect %g: the shorter side truncates to 0", ow, oh, aspect); return -1; }
    if (!item) return 0;
    item->aspect = aspect; item->scale = scale; item->rad = rad; item->dx = dx; item->dy = dy;
    item->flip = flip;
    item->dhue = dhue; item->dsat = dsat; item->dexp = dexp;
    return 0;
}

int y2_aug_labels(const char *path, char **labels, int k, const tree *hierarchy, float *truth)
{
    int i, j, count = 0;
    if (!path || !labels || !truth || k < 0) { y2_fail("y2_aug_labels: NULL path, labels or truth"); return -1; }
    memset(truth, 0, (size_t)k * sizeof(float));        /* data.c:387 fill_truth */
    for (i = 0; i < k; ++i) {
        if (labels[i] && strstr(path, labels[i])) {
            truth[i] = 1;
            ++count;
        }
    }
    if (!hierarchy) return count;
    for (j = 0; j < k && j < hierarchy->n; ++j) {       /* data.c:401 fill_hierarchy */
        if (truth[j]) {
            int parent = hierarchy->parent[j];
            while (parent >= 0 && parent < k) {
                truth[parent] = 1;
                parent = hierarchy->parent[parent];
            }
        }
    }
    for (j = 0, i = 0; j < hierarchy->groups; ++j) {
        const int gs = hierarchy->group_size[j];
        int mask = 1, g;
        if (i + gs > k) break;                          /* a tree wider than the row: the reference would write past it */
        for (g = 0; g < gs; ++g)
            if (truth[i + g]) { mask = 0; break; }
        if (mask)
            for (g = 0; g < gs; ++g) truth[i + g] = Y2_SECRET_NUM;
        i += gs;
    }
    return count;
}

static int finite_f(float v) { return v - v == 0; }

int y2_aug_cls_check(const char *who, const y2_aug_cls_item *items, int n)
{
    int i;
    if (!items) { y2_fail("%s: no items", who); return -1; }
    for (i = 0; i < n; ++i) {
        const y2_aug_cls_item *it = &items[i];
        if (!it->data) { y2_fail("%s: item %d: data is NULL", who, i); return -1; }
        if (it->h <= 0 || it->w <= 0) { y2_fail("%s: item %d: bad frame geometry %d x %d", who, i, it->h, it->w); return -1; }
        if (it->c < 3) { y2_fail("%s: item %d: the frame has %d channels, the loader reads 3", who, i, it->c); return -1; }
        if ((long)it->step < (long)it->w * it->c) { y2_fail("%s: item %d: step %d is less than w*c = %ld", who, i, it->step, (long)it->w * it->c); return -1; }
        if (!finite_f(it->scale) || !(it->scale > 0)) { y2_fail("%s: item %d: scale %g is not finite and positive", who, i, it->scale); return -1; }
        if (!finite_f(it->aspect) || !(it->aspect > 0)) { y2_fail("%s: item %d: aspect %g is not finite and positive", who, i, it->aspect); return -1; }
        if (!finite_f(it->rad)) { y2_fail("%s: item %d: rad %g is not finite", who, i, it->rad); return -1; }
        if (!finite_f(it->dx)) { y2_fail("%s: item %d: dx %g is not finite", who, i, it->dx); return -1; }
        if (!finite_f(it->dy)) { y2_fail("%s: item %d: dy %g is not finite", who, i, it->dy); return -1; }
    }
    return 0;
}

/* everything of the descriptor that does not depend on the rectangle */
static void cls_terms(const y2_aug_cls_item *it, y2h_aug_cls *d)
{
    d->cosr = cos((double)it->rad);
    d->sinr = sin((double)it->rad);
    d->s = it->scale;
    d->aspect = it->aspect;
    d->ax = (float)((float)(it->dx / it->scale) * it->aspect);      /* dx/s*aspect: three floats, float operations */
    d->ay = (float)(it->dy / it->scale);                             /* dy/s */
    d->cx = it->w / 2.;
    d->cy = it->h / 2.;
    d->c = it->c;
    d->ow = it->w; d->oh = it->h;
    d->flip = it->flip != 0;
    d->dhue = it->dhue; d->dsat = it->dsat; d->dexp = it->dexp;
}

/* floorf of a coordinate as an int; outside [-1, hi] every value clamps like the nearest of the two */
static int floor_tap(float v, int hi)
{
    float f = floorf(v);
    if (!(f >= -1)) return -1;          /* also a NaN, which the kernel reads as 0 */
    if (f > hi) return hi;
    return (int)f;
}

/* The frame rectangle the taps of a size x size crop can touch, into d->x0 .. d->rh of a descriptor whose terms are
 * filled.  (x, y) -> (rx, ry) is affine, so the extremes lie at the four output corners: the kernel's own formula there,
 * floorf and the + 1 tap, get_pixel_extend's clamp, and one pixel more on every side for the rounding of the points in
 * between. */
static void cls_rect(y2h_aug_cls *d, int size)
{
    const double half = size / 2.;
    int k, xa = d->ow - 1, xb = 0, ya = d->oh - 1, yb = 0;
    for (k = 0; k < 4; ++k) {
        const int x = (k & 1) ? size - 1 : 0, y = (k & 2) ? size - 1 : 0;
        const double ux = (x - half) / d->s * d->aspect + d->ax;
        const double vy = (y - half) / d->s + d->ay;
        const float rx = (float)(d->cosr * ux - d->sinr * vy + (double)d->cx);
        const float ry = (float)(d->sinr * ux + d->cosr * vy + (double)d->cy);
        const int ix = floor_tap(rx, d->ow), iy = floor_tap(ry, d->oh);
        const int lx = clamp_l(ix, 0, d->ow - 1), hx = clamp_l((long)ix + 1, 0, d->ow - 1);
        const int ly = clamp_l(iy, 0, d->oh - 1), hy = clamp_l((long)iy + 1, 0, d->oh - 1);
        if (lx < xa) xa = lx;
        if (hx > xb) xb = hx;
        if (ly < ya) ya = ly;
        if (hy > yb) yb = hy;
    }
    xa = clamp_l((long)xa - 1, 0, d->ow - 1); xb = clamp_l((long)xb + 1, 0, d->ow - 1);
    ya = clamp_l((long)ya - 1, 0, d->oh - 1); yb = clamp_l((long)yb + 1, 0, d->oh - 1);
    d->x0 = xa; d->y0 = ya;
    d->rw = xb - xa + 1; d->rh = yb - ya + 1;
}

void y2_aug_cls_rect(const y2_aug_cls_item *it, int size, int *x0, int *y0, int *rw, int *rh)
{
    y2h_aug_cls d;
    cls_terms(it, &d);
    cls_rect(&d, size);
    *x0 = d.x0; *y0 = d.y0; *rw = d.rw; *rh = d.rh;
}

/* desc[n] whole -- terms, rectangle, and where the rectangle will lie behind `pixels` -- with one cos / sin and one
 * rectangle per image; returns the bytes the rectangles take back to back */
size_t y2_aug_cls_describe(const y2_aug_cls_item *items, int n, int size, y2h_aug_cls *desc)
{
    size_t off = 0;
    int i;
    memset(desc, 0, (size_t)n * sizeof *desc);
    for (i = 0; i < n; ++i) {
        y2h_aug_cls *d = &desc[i];
        cls_terms(&items[i], d);
        cls_rect(d, size);
        d->src = (long long)off;
        d->pitch = d->rw * d->c;
        off += (size_t)d->pitch * d->rh;
    }
    return off;
}

/* the rectangles of a described batch, row by row out of the frames */
void y2_aug_cls_copy(const y2_aug_cls_item *items, int n, const y2h_aug_cls *desc, unsigned char *pixels)
{
    int i, r;
    for (i = 0; i < n; ++i) {
        const y2_aug_cls_item *it = &items[i];
        const y2h_aug_cls *d = &desc[i];
        for (r = 0; r < d->rh; ++r)
            memcpy(pixels + d->src + (size_t)r * d->pitch, it->data + (size_t)(d->y0 + r) * it->step + (size_t)d->x0 * it->c, (size_t)d->pitch);
    }
}

size_t y2_aug_cls_pack_bytes(const y2_aug_cls_item *items, int n, int size)
{
    size_t bytes = 0;
    int i, x0, y0, rw, rh;
    for (i = 0; i < n; ++i) {
        y2_aug_cls_rect(&items[i], size, &x0, &y0, &rw, &rh);
        bytes += (size_t)rw * rh * items[i].c;
    }
    return bytes;
}

/* desc[n] and the rectangles back to back in `pixels` (y2_aug_cls_pack_bytes of room); offsets count from `pixels` */
void y2_aug_cls_pack(const y2_aug_cls_item *items, int n, int size, y2h_aug_cls *desc, unsigned char *pixels)
{
    y2_aug_cls_describe(items, n, size, desc);
    y2_aug_cls_copy(items, n, desc, pixels);
}
