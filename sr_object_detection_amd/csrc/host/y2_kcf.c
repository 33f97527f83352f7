/*
 * The KCF trackers of the Kinect loop on the host side: what KinectUtil_with_cam.cpp:764-803 (InitialTracker,
 * test_tracker_img) does per frame over kcf.cpp -- one KCF_Tracker per detected object, tracked under an OpenMP loop --
 * backed by the kernels of y2_kcf.hip, all trackers in one batch.  This file plans (init's arithmetic, the arena, the
 * labels, the window and the twiddles), stages the frame rows the windows touch, checks and launches; there is no CPU
 * implementation of the tracker.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

_Static_assert(Y2_KCF_MAX_TRACKERS == Y2H_KCF_MAX_TRACKERS && Y2_KCF_MAX_CELLS == Y2H_KCF_MAX_CELLS, "one set of limits");

#define KCF_PADDING 3.0
#define KCF_OUTPUT_SIGMA_FACTOR 0.1
#define KCF_CELL 4
#define KCF_PI 3.14159265358979323846

typedef struct y2_kcf_state {
    int n, fh, fw, fc;
    y2_kcf_geometry geo[Y2_KCF_MAX_TRACKERS];
    double pose[Y2_KCF_MAX_TRACKERS][2];     /* the stored pose, mirrored: it sizes the frame band */
    y2h_kcf_desc desc[Y2_KCF_MAX_TRACKERS];
    unsigned char *d_arena, *h_stage;        /* [desc | pose | rec | labels, windows, twiddles] is what init uploads */
    size_t arena_cap, h_stage_cap, off_pose, off_rec;
    unsigned char *h_frame, *d_frame;        /* the frame band, pinned and in HBM, grow-only */
    size_t h_frame_cap, d_frame_cap;
    y2h_kcf_rec *h_rec;                      /* pinned: all trackers come back in one copy */
    long max_pixels, max_cells;
    int max_side;
    object objs[Y2_KCF_MAX_TRACKERS];        /* tracking_objects */
    int have_objs;
} y2_kcf_state;

static int grow_dev(unsigned char **p, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    y2h_free(*p); *p = NULL; *cap = 0;
    if (y2h_malloc((void **)p, need) != 0) return -1;
    *cap = need;
    return 0;
}

static int grow_pinned(unsigned char **p, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    y2h_host_free(*p); *p = NULL; *cap = 0;
    if (y2h_host_alloc((void **)p, need) != 0) return -1;
    *cap = need;
    return 0;
}

void y2_kcf_free_engine(y2_engine *e)
{
    y2_kcf_state *s = e->kcf;
    if (!s) return;
    y2h_free(s->d_arena); y2h_host_free(s->h_stage);
    y2h_free(s->d_frame); y2h_host_free(s->h_frame);
    y2h_host_free(s->h_rec);
    free(s);
    e->kcf = NULL;
}

void y2_kcf_free(network net)
{
    y2_engine *e = y2_engine_of(&net);
    if (!e || !e->kcf) return;
    y2h_set_device(e->device);
    y2h_stream_sync(e->stream);
    y2_kcf_free_engine(e);
}

int y2_kcf_count(network net)
{
    const y2_engine *e = y2_engine_of(&net);
    return e && e->kcf ? e->kcf->n : 0;
}

/* ------------------------------------------------------------------ */
/* the plan                                                            */
/* ------------------------------------------------------------------ */
static int plan_box(const char *who, int i, const y2_kcf_box *b, y2_kcf_geometry *g)
{
    double cx, cy, w, h, ww, wh;
    if (!isfinite(b->cx) || !isfinite(b->cy) || !isfinite(b->w) || !isfinite(b->h)) { y2_fail("%s: box %d is not finite", who, i); return -1; }
    if (!(b->w > 0) || !(b->h > 0)) { y2_fail("%s: box %d has w <= 0 or h <= 0 (%g x %g)", who, i, b->w, b->h); return -1; }
    cx = b->cx; cy = b->cy; w = b->w; h = b->h;
    g->resized = w * h > 100. * 100.;
    if (g->resized) { cx *= 0.5; cy *= 0.5; w *= 0.5; h *= 0.5; }
    ww = floor(w * (1. + KCF_PADDING)); wh = floor(h * (1. + KCF_PADDING));
    if (ww / KCF_CELL >= Y2_KCF_MAX_CELLS + 1 || wh / KCF_CELL >= Y2_KCF_MAX_CELLS + 1) {
        y2_fail("%s: box %d (%g x %g) gives a feature map above Y2_KCF_MAX_CELLS = %d cells per side", who, i, b->w, b->h, Y2_KCF_MAX_CELLS);
        return -1;
    }
    g->win_w = (int)ww; g->win_h = (int)wh;
    g->cells_w = g->win_w / KCF_CELL; g->cells_h = g->win_h / KCF_CELL;
    if (g->cells_w < 2 || g->cells_h < 2) {
        y2_fail("%s: box %d (%g x %g) gives a feature map below 2 x 2 cells", who, i, b->w, b->h);
        return -1;
    }
    g->cx = cx; g->cy = cy; g->w = w; g->h = h;
    g->output_sigma = sqrt(w * h) * KCF_OUTPUT_SIGMA_FACTOR / (double)KCF_CELL;
    return 0;
}

int y2_kcf_plan(const y2_kcf_box *b, y2_kcf_geometry *g)
{
    if (!b || !g) { y2_fail("y2_kcf_plan: box or geometry is NULL"); return -1; }
    return plan_box("y2_kcf_plan", 0, b, g);
}

static int frame_check(const char *who, const unsigned char *frame, int h, int w, int c, int step)
{
    if (!frame) { y2_fail("%s: the frame is NULL", who); return -1; }
    if (c != 1 && c != 3 && c != 4) { y2_fail("%s: a frame has 1, 3 (BGR) or 4 (BGRA) channels, not %d", who, c); return -1; }
    if (h < 1 || w < 1 || h > 32767 || w > 32767) { y2_fail("%s: bad frame size %d x %d", who, w, h); return -1; }
    if (step < w * c) { y2_fail("%s: step %d is less than w*c = %d", who, step, w * c); return -1; }
    return 0;
}

/* the buffers of one tracker from float offset `off` on: first what init uploads, then (consts == 0) the work buffers */
static size_t lay_out(y2h_kcf_desc *d, size_t off, int consts)
{
    const size_t R = d->cells_h, C = d->cells_w, P = R * C, px = (size_t)d->win_w * d->win_h;
#define TAKE(field, n) do { d->field = (long long)off; off += align_up((n), 64); } while (0)
    if (consts) {
        TAKE(lab, P); TAKE(win, R + C); TAKE(cc, C * C); TAKE(nsc, C * C); TAKE(cr, R * R); TAKE(sr, R * R); TAKE(nsr, R * R);
    } else {
        TAKE(patch, px); TAKE(mag, px); TAKE(bin, px); TAKE(hist, 18 * P); TAKE(ssum, P); TAKE(feat, Y2H_KCF_CHANNELS * P);
        TAKE(x, Y2H_KCF_CHANNELS * P); TAKE(y, 2 * Y2H_KCF_CHANNELS * P); TAKE(xf, 2 * Y2H_KCF_CHANNELS * P);
        TAKE(model_xf, 2 * Y2H_KCF_CHANNELS * P);
        TAKE(z, 2 * P); TAKE(t, 2 * P); TAKE(gy, 2 * P); TAKE(kf, 2 * P); TAKE(p, 2 * P); TAKE(model_alphaf, 2 * P); TAKE(yf, 2 * P);
        TAKE(xy, P); TAKE(g, P); TAKE(resp, P); TAKE(part, 2 * Y2H_KCF_CHUNKS);
    }
#undef TAKE
    return off;
}

/* cos / sin / -sin of 2*pi*((j*k) mod n)/n: the argument stays in [0, 2*pi) whatever the index */
static void twiddles(int n, float *c, float *s, float *ns)
{
    int j, k;
    for (j = 0; j < n; ++j)
        for (k = 0; k < n; ++k) {
            const double a = 2. * KCF_PI * (double)(((long)j * k) % n) / (double)n;
            c[(size_t)j * n + k] = (float)cos(a);
            if (s) s[(size_t)j * n + k] = (float)sin(a);
            ns[(size_t)j * n + k] = (float)-sin(a);
        }
}

static void fill_consts(const y2h_kcf_desc *d, double sigma, float *base)
{
    const int R = d->cells_h, C = d->cells_w;
    float *lab = base + d->lab, *win = base + d->win;
    const double sigma_s = sigma * sigma;
    int i, j;
    /* gaussian_shaped_labels (:132-154) with the circshift that puts its 1 at (0, 0) folded into the index */
    for (j = 0; j < R; ++j)
        for (i = 0; i < C; ++i) {
            const int y = j - R / 2, x = i - C / 2;
            const double y_s = (double)(y * y);
            lab[(size_t)((j + R - R / 2) % R) * C + (i + C - C / 2) % C] = (float)exp(-0.5 * (y_s + (double)(x * x)) / sigma_s);
        }
    /* cosine_window_function (:261-272): the two factors of its outer product */
    for (j = 0; j < R; ++j) win[j] = (float)(0.5 * (1. - cos(2. * KCF_PI * (double)j * (1. / ((double)R - 1.)))));
    for (i = 0; i < C; ++i) win[R + i] = (float)(0.5 * (1. - cos(2. * KCF_PI * (double)i * (1. / ((double)C - 1.)))));
    twiddles(C, base + d->cc, NULL, base + d->nsc);
    twiddles(R, base + d->cr, base + d->sr, base + d->nsr);
}

/* ------------------------------------------------------------------ */
/* the frame band                                                      */
/* ------------------------------------------------------------------ */
static int half_size(int n) { return n / 2 + ((n & 1) ? ((n / 2) & 1) : 0); }

/* rows [lo, hi) of the frame that the windows of this call can read; `moving`: the second window of an updating track
 * lies up to cells_h/2 + 1 cells from the first */
static void frame_band(const y2_kcf_state *s, int moving, int *lo, int *hi)
{
    int i, a = s->fh, b = 0;
    for (i = 0; i < s->n; ++i) {
        const y2_kcf_geometry *g = &s->geo[i];
        const int rows = g->resized ? half_size(s->fh) : s->fh;
        const double margin = (double)g->win_h / 2 + 2 + (moving ? KCF_CELL * (g->cells_h / 2 + 1) : 0);
        double y1 = s->pose[i][1] - margin, y2 = s->pose[i][1] + margin;
        int r1, r2;
        if (!(y1 > 0)) y1 = 0;                                /* also a pose that is not a number */
        if (!(y2 < rows - 1)) y2 = rows - 1;
        if (y1 > rows - 1) y1 = rows - 1;
        if (y2 < 0) y2 = 0;
        r1 = (int)y1; r2 = (int)y2;
        if (g->resized) { r1 = 2 * r1 - 1; r2 = 2 * r2 + 2; }
        if (r1 < 0) r1 = 0;
        if (r2 > s->fh - 1) r2 = s->fh - 1;
        if (r1 < a) a = r1;
        if (r2 + 1 > b) b = r2 + 1;
    }
    if (a >= b) { a = 0; b = 1; }
    *lo = a; *hi = b;
}

static int upload_band(const char *who, y2_engine *e, y2_kcf_state *s, const unsigned char *frame, int step, int moving, y2h_kcf_frame *f)
{
    int lo, hi, r;
    const size_t row = (size_t)s->fw * s->fc;
    frame_band(s, moving, &lo, &hi);
    if (grow_pinned(&s->h_frame, &s->h_frame_cap, row * (hi - lo)) || grow_dev(&s->d_frame, &s->d_frame_cap, row * (hi - lo))) {
        y2_fail("%s: %s", who, y2h_last_error()); return -1;
    }
    for (r = lo; r < hi; ++r) memcpy(s->h_frame + (size_t)(r - lo) * row, frame + (size_t)r * step, row);
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_frame, s->h_frame, row * (hi - lo), e->stream));
    f->bytes = s->d_frame; f->h = s->fh; f->w = s->fw; f->c = s->fc; f->row_lo = lo; f->row_hi = hi;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the chains                                                          */
/* ------------------------------------------------------------------ */
#define D_DESC(s) ((const y2h_kcf_desc *)(s)->d_arena)
#define D_POSE(s) ((double *)((s)->d_arena + (s)->off_pose))
#define D_REC(s) ((y2h_kcf_rec *)((s)->d_arena + (s)->off_rec))

/* sub-window -> fHOG -> the windowed channels' DFT, about the stored pose or about the tracked one */
static int features(y2_engine *e, y2_kcf_state *s, const y2h_kcf_frame *f, int at_rec)
{
    const double *centres = at_rec ? (const double *)D_REC(s) : D_POSE(s);
    const int stride = at_rec ? (int)(sizeof(y2h_kcf_rec) / sizeof(double)) : 2;
    HIP_OR_ERR(y2h_kcf_patch(D_DESC(s), s->n, (float *)s->d_arena, f, centres, stride, s->max_pixels, e->stream));
    HIP_OR_ERR(y2h_kcf_fhog(D_DESC(s), s->n, (float *)s->d_arena, s->max_pixels, s->max_cells, e->stream));
    HIP_OR_ERR(y2h_kcf_dft(D_DESC(s), s->n, (float *)s->d_arena, Y2H_KCF_DFT_X, s->max_side, e->stream));
    return 0;
}

/* gaussian_correlation (:327-351) of xf with itself or with the model -> kf */
static int correlate(y2_engine *e, y2_kcf_state *s, int autoc)
{
    HIP_OR_ERR(y2h_kcf_cross(D_DESC(s), s->n, (float *)s->d_arena, autoc, e->stream));
    HIP_OR_ERR(y2h_kcf_dft(D_DESC(s), s->n, (float *)s->d_arena, Y2H_KCF_IDFT_Z, s->max_side, e->stream));
    HIP_OR_ERR(y2h_kcf_gauss(D_DESC(s), s->n, (float *)s->d_arena, s->max_cells, e->stream));
    HIP_OR_ERR(y2h_kcf_dft(D_DESC(s), s->n, (float *)s->d_arena, Y2H_KCF_DFT_G, s->max_side, e->stream));
    return 0;
}

/* init (:29-40) behind the uploads: the labels' DFT, the first model */
static int init_chain(y2_engine *e, y2_kcf_state *s, const y2h_kcf_frame *f)
{
    if (features(e, s, f, 0) != 0) return -1;
    HIP_OR_ERR(y2h_kcf_dft(D_DESC(s), s->n, (float *)s->d_arena, Y2H_KCF_DFT_LAB, s->max_side, e->stream));
    if (correlate(e, s, 1) != 0) return -1;
    HIP_OR_ERR(y2h_kcf_train(D_DESC(s), s->n, (float *)s->d_arena, 0, D_POSE(s), D_REC(s), s->max_cells, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));                  /* the pinned buffers are the next call's */
    return 0;
}

int y2_kcf_init(network net, const unsigned char *frame, int h, int w, int c, int step, const y2_kcf_box *boxes, int n)
{
    static const char *who = "y2_kcf_init";
    y2_kcf_geometry geo[Y2_KCF_MAX_TRACKERS];
    y2_engine *e;
    y2_kcf_state *s;
    y2h_kcf_frame f;
    size_t head, off, consts_end;
    int i;
    if (n > Y2_KCF_MAX_TRACKERS) { y2_fail("%s: %d trackers, at most Y2_KCF_MAX_TRACKERS = %d", who, n, Y2_KCF_MAX_TRACKERS); return -1; }
    if (n < 1 || !boxes) { y2_fail("%s: needs boxes and n >= 1", who); return -1; }
    if (frame_check(who, frame, h, w, c, step) != 0) return -1;
    for (i = 0; i < n; ++i) if (plan_box(who, i, &boxes[i], &geo[i]) != 0) return -1;
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!e->kcf) e->kcf = calloc(1, sizeof(y2_kcf_state));
    s = e->kcf;
    if (!s) { y2_fail("%s: out of memory", who); return -1; }
    HIP_OR_ERR(y2h_stream_sync(e->stream));                  /* nothing in flight reads the old trackers */
    s->n = 0; s->have_objs = 0;
    s->fh = h; s->fw = w; s->fc = c;
    s->max_pixels = s->max_cells = 0; s->max_side = 0;
    s->off_pose = align_up((size_t)n * sizeof(y2h_kcf_desc), 256);
    s->off_rec = s->off_pose + align_up((size_t)n * 2 * sizeof(double), 256);
    head = s->off_rec + align_up((size_t)n * sizeof(y2h_kcf_rec), 256);
    off = head / sizeof(float);
    for (i = 0; i < n; ++i) {
        y2h_kcf_desc *d = &s->desc[i];
        const y2_kcf_geometry *g = &geo[i];
        memset(d, 0, sizeof *d);
        d->resized = g->resized; d->win_w = g->win_w; d->win_h = g->win_h; d->cells_w = g->cells_w; d->cells_h = g->cells_h;
        off = lay_out(d, off, 1);
        s->geo[i] = *g;
        s->pose[i][0] = g->cx; s->pose[i][1] = g->cy;
        if ((long)g->win_w * g->win_h > s->max_pixels) s->max_pixels = (long)g->win_w * g->win_h;
        if ((long)g->cells_w * g->cells_h > s->max_cells) s->max_cells = (long)g->cells_w * g->cells_h;
        if (g->cells_w > s->max_side) s->max_side = g->cells_w;
        if (g->cells_h > s->max_side) s->max_side = g->cells_h;
    }
    consts_end = off * sizeof(float);
    for (i = 0; i < n; ++i) off = lay_out(&s->desc[i], off, 0);
    if (grow_pinned(&s->h_stage, &s->h_stage_cap, consts_end) || grow_dev(&s->d_arena, &s->arena_cap, off * sizeof(float)) ||
        (!s->h_rec && y2h_host_alloc((void **)&s->h_rec, Y2_KCF_MAX_TRACKERS * sizeof(y2h_kcf_rec)) != 0)) {
        y2_fail("%s: %s", who, y2h_last_error()); return -1;
    }
    memset(s->h_stage, 0, head);
    memcpy(s->h_stage, s->desc, (size_t)n * sizeof(y2h_kcf_desc));
    memcpy(s->h_stage + s->off_pose, s->pose, (size_t)n * 2 * sizeof(double));
    for (i = 0; i < n; ++i) fill_consts(&s->desc[i], geo[i].output_sigma, (float *)s->h_stage);
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_arena, s->h_stage, consts_end, e->stream));
    s->n = n;
    if (upload_band(who, e, s, frame, step, 0, &f) != 0) { s->n = 0; return -1; }
    if (init_chain(e, s, &f) != 0) { s->n = 0; return -1; }
    return 0;
}

static y2_kcf_state *tracking(const char *who, network net, y2_engine **pe)
{
    y2_engine *e = y2_engine_of(&net);
    y2_kcf_state *s = e ? e->kcf : NULL;
    if (!s || s->n < 1) { y2_fail("%s: no trackers: call y2_kcf_init first", who); return NULL; }
    *pe = e;
    return s;
}

int y2_kcf_track(network net, const unsigned char *frame, int h, int w, int c, int step, int update, y2_kcf_box *out, float *peak)
{
    static const char *who = "y2_kcf_track";
    y2_engine *e;
    y2_kcf_state *s;
    y2h_kcf_frame f;
    int i;
    if (frame_check(who, frame, h, w, c, step) != 0) return -1;
    s = tracking(who, net, &e);
    if (!s) return -1;
    if (h != s->fh || w != s->fw || c != s->fc) {
        y2_fail("%s: the frame is %d x %d x %d, the trackers were initialised on %d x %d x %d", who, w, h, c, s->fw, s->fh, s->fc);
        return -1;
    }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (upload_band(who, e, s, frame, step, update != 0, &f) != 0) return -1;
    if (features(e, s, &f, 0) != 0 || correlate(e, s, 0) != 0) return -1;
    HIP_OR_ERR(y2h_kcf_apply(D_DESC(s), s->n, (float *)s->d_arena, s->max_cells, e->stream));
    HIP_OR_ERR(y2h_kcf_dft(D_DESC(s), s->n, (float *)s->d_arena, Y2H_KCF_IDFT_P, s->max_side, e->stream));
    HIP_OR_ERR(y2h_kcf_argmax(D_DESC(s), s->n, (const float *)s->d_arena, D_POSE(s), D_REC(s), e->stream));
    if (update) {                                            /* the retraining half, about the tracked position */
        if (features(e, s, &f, 1) != 0 || correlate(e, s, 1) != 0) return -1;
        HIP_OR_ERR(y2h_kcf_train(D_DESC(s), s->n, (float *)s->d_arena, 1, D_POSE(s), D_REC(s), s->max_cells, e->stream));
    }
    HIP_OR_ERR(y2h_memcpy_d2h(s->h_rec, D_REC(s), (size_t)s->n * sizeof(y2h_kcf_rec), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    for (i = 0; i < s->n; ++i) {
        const y2_kcf_geometry *g = &s->geo[i];
        const double k = g->resized ? 2. : 1.;               /* getBBox (:65-73) */
        if (out) { out[i].cx = s->h_rec[i].cx * k; out[i].cy = s->h_rec[i].cy * k; out[i].w = g->w * k; out[i].h = g->h * k; }
        if (peak) peak[i] = s->h_rec[i].peak;
        if (update) { s->pose[i][0] = s->h_rec[i].cx; s->pose[i][1] = s->h_rec[i].cy; }
    }
    return 0;
}

int y2_kcf_fetch(network net, int i, int what, float *dst, size_t floats)
{
    static const char *who = "y2_kcf_fetch";
    y2_engine *e;
    y2_kcf_state *s = tracking(who, net, &e);
    const y2h_kcf_desc *d;
    size_t P, n;
    long long at;
    if (!s) return -1;
    if (i < 0 || i >= s->n || !dst) { y2_fail("%s: tracker %d of %d, dst %s", who, i, s->n, dst ? "given" : "NULL"); return -1; }
    d = &s->desc[i];
    P = (size_t)d->cells_h * d->cells_w;
    switch (what) {
    case Y2_KCF_PATCH: at = d->patch; n = (size_t)d->win_w * d->win_h; break;
    case Y2_KCF_FEATURES: at = d->feat; n = Y2H_KCF_CHANNELS * P; break;
    case Y2_KCF_XF: at = d->model_xf; n = 2 * Y2H_KCF_CHANNELS * P; break;
    case Y2_KCF_ALPHAF: at = d->model_alphaf; n = 2 * P; break;
    case Y2_KCF_RESPONSE: at = d->resp; n = P; break;
    default: y2_fail("%s: unknown tensor %d", who, what); return -1;
    }
    if (floats != n) { y2_fail("%s: tensor %d of tracker %d has %zu floats, not %zu", who, what, i, n, floats); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    HIP_OR_ERR(y2h_memcpy_d2h(dst, (const float *)s->d_arena + at, n * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_kcf_dft(network net, const float *src, int rows, int cols, int inverse, float *dst)
{
    static const char *who = "y2_kcf_dft";
    y2_engine *e;
    y2h_kcf_desc d;
    unsigned char *dev = NULL, *host;
    size_t head = align_up(sizeof d, 256), off, P, nin, nout;
    int rc = -1;
    if (!src || !dst || rows < 2 || cols < 2 || rows > Y2_KCF_MAX_CELLS || cols > Y2_KCF_MAX_CELLS) {
        y2_fail("%s: needs src, dst and 2 <= rows, cols <= %d", who, Y2_KCF_MAX_CELLS); return -1;
    }
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    HIP_OR_ERR(y2h_set_device(e->device));
    memset(&d, 0, sizeof d);
    d.cells_h = rows; d.cells_w = cols; d.win_w = cols * KCF_CELL; d.win_h = rows * KCF_CELL;
    P = (size_t)rows * cols;
    off = lay_out(&d, head / sizeof(float), 1);
    {                                                        /* only the buffers of the two single-channel transforms */
        const size_t two = align_up(2 * P, 64), one = align_up(P, 64);
        d.p = (long long)off; off += two; d.t = (long long)off; off += two; d.resp = (long long)off; off += one;
        d.gy = (long long)off; off += two; d.yf = (long long)off; off += two;
    }
    host = calloc(off, sizeof(float));
    if (!host) { y2_fail("%s: out of memory", who); return -1; }
    memcpy(host, &d, sizeof d);
    fill_consts(&d, 1., (float *)host);
    nin = inverse ? 2 * P : P; nout = inverse ? P : 2 * P;
    memcpy((float *)host + (inverse ? d.p : d.lab), src, nin * sizeof(float));
    HIP_OR_CLEANUP(y2h_malloc((void **)&dev, off * sizeof(float)));
    HIP_OR_CLEANUP(y2h_memcpy_h2d(dev, host, off * sizeof(float), e->stream));
    HIP_OR_CLEANUP(y2h_stream_sync(e->stream));              /* `host` is pageable */
    HIP_OR_CLEANUP(y2h_kcf_dft((const y2h_kcf_desc *)dev, 1, (float *)dev, inverse ? Y2H_KCF_IDFT_P : Y2H_KCF_DFT_LAB,
                               rows > cols ? rows : cols, e->stream));
    HIP_OR_CLEANUP(y2h_memcpy_d2h(dst, (const float *)dev + (inverse ? d.resp : d.yf), nout * sizeof(float), e->stream));
    HIP_OR_CLEANUP(y2h_stream_sync(e->stream));
    rc = 0;
cleanup:
    y2h_free(dev);
    free(host);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the application's two calls                                         */
/* ------------------------------------------------------------------ */
void y2_kcf_init_objects(network net, const unsigned char *frame, int h, int w, int c, int step, const object *objs, int n)
{
    y2_kcf_box boxes[Y2_KCF_MAX_TRACKERS];
    y2_kcf_state *s;
    int i;
    if (n > Y2_KCF_MAX_TRACKERS) { y2_fail("y2_kcf_init_objects: %d trackers, at most Y2_KCF_MAX_TRACKERS = %d", n, Y2_KCF_MAX_TRACKERS); return; }
    if (n < 1 || !objs) { y2_fail("y2_kcf_init_objects: needs objects and n >= 1"); return; }
    for (i = 0; i < n; ++i) {                                /* :774-777: float * int, then widened */
        boxes[i].cx = (double)(objs[i].x * (float)w); boxes[i].cy = (double)(objs[i].y * (float)h);
        boxes[i].w = (double)(objs[i].w * (float)w); boxes[i].h = (double)(objs[i].h * (float)h);
    }
    if (y2_kcf_init(net, frame, h, w, c, step, boxes, n) != 0) return;
    s = y2_engine_of(&net)->kcf;
    memcpy(s->objs, objs, (size_t)n * sizeof(object));
    s->have_objs = 1;
}

void y2_kcf_track_objects(network net, const unsigned char *frame, int h, int w, int c, int step, object *objs, int *n)
{
    static const char *who = "y2_kcf_track_objects";
    y2_kcf_box out[Y2_KCF_MAX_TRACKERS];
    y2_engine *e;
    y2_kcf_state *s;
    int i;
    if (!objs || !n) { y2_fail("%s: objs / n is NULL", who); return; }
    s = tracking(who, net, &e);
    if (!s) return;
    if (!s->have_objs) { y2_fail("%s: the trackers were not initialised from objects (y2_kcf_init_objects)", who); return; }
    if (y2_kcf_track(net, frame, h, w, c, step, 0, out, NULL) != 0) return;
    *n = s->n;
    for (i = 0; i < s->n; ++i) {                             /* :796-801 */
        s->objs[i].w = (float)(out[i].w / w); s->objs[i].h = (float)(out[i].h / h);
        s->objs[i].x = (float)(out[i].cx / w); s->objs[i].y = (float)(out[i].cy / h);
        objs[i] = s->objs[i];
    }
}
