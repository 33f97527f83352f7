/*
 * The depth stage of the Kinect RGB-D loop on the host side: what KinectUtil_with_cam.cpp does per frame around its
 * detector calls -- drawDepth (:394-442), colorImgFilterbyDistance (:1866-1888), caculateXYZinCameraSpace (:1482-1562)
 * and objectBelong2Person (:1632-1706) -- backed by the kernels of y2_depth.hip and the filtered region ingest of
 * y2_image.hip.  This file stages, checks and launches; there is no CPU implementation of the stage besides the scalar
 * rules of include/y2_depth_rule.h, which the kernels compile too.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"
#include "y2_depth_rule.h"
#include "y2_plane_rule.h"

_Static_assert(sizeof(y2_det3d) == sizeof(y2h_det3d), "y2_det3d and y2h_det3d are one layout");
_Static_assert(sizeof(y2_plane) == sizeof(y2h_plane), "y2_plane and y2h_plane are one layout");

#define Y2_DEPTH_EAGER 256               /* records of y2_detect_regions_depth fetched before the counts are known (25 KB) */

typedef struct y2_depth_state {
    /* upload: depth | map | body packed into pinned memory, one copy, then the alignment kernel */
    unsigned char *h_stage, *d_stage;
    size_t h_stage_cap, d_stage_cap;
    y2h_event ev_up;                     /* behind the copy: the pinned buffer may be refilled after it */
    int up_pending;
    /* the aligned planes, carved from one grow-only allocation */
    unsigned char *d_planes;
    size_t planes_cap;
    unsigned short *d16;
    short *dxy;                          /* (dx, dy) per colour pixel, (-1, -1) unmapped; unused for an identity frame */
    unsigned char *d8, *person;
    int have, has_map, H, W, dh, dw;
    float *d_tab;                        /* camera table */
    int tab_dh, tab_dw;
    /* per-box work: boxes / maps in, accumulators, results out */
    unsigned char *h_box, *d_box;
    size_t h_box_cap, d_box_cap;
    y2h_event ev_box;
    /* table-plane removal (the Grasp branch): off unless plane.iters > 0 */
    y2_plane_opts plane;
    int *plane_samples;                  /* the caller's triples (plane.samples points here), or NULL: the sampler */
    unsigned short *grasp_depth, *grasp16;   /* dh x dw and H x W; one plane for an identity frame */
    y2h_plane *plane_rec;
    int have_grasp;                      /* the uploaded frame went through the removal */
    int event, grasp_filter;
} y2_depth_state;

static int grow_dev(void **p, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    y2h_free(*p); *p = NULL; *cap = 0;
    if (y2h_malloc(p, need) != 0) return -1;
    *cap = need;
    return 0;
}

static int grow_pinned(void **p, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    y2h_host_free(*p); *p = NULL; *cap = 0;
    if (y2h_host_alloc(p, need) != 0) return -1;
    *cap = need;
    return 0;
}

static y2_depth_state *state_of(y2_engine *e, int create)
{
    if (!e->depth && create) e->depth = calloc(1, sizeof(y2_depth_state));
    return e->depth;
}

void y2_depth_free(y2_engine *e)
{
    y2_depth_state *s = e->depth;
    if (!s) return;
    if (s->up_pending) y2h_event_sync(s->ev_up);
    y2h_host_free(s->h_stage); y2h_free(s->d_stage);
    y2h_free(s->d_planes); y2h_free(s->d_tab);
    y2h_host_free(s->h_box); y2h_free(s->d_box);
    if (s->ev_up) y2h_event_destroy(s->ev_up);
    if (s->ev_box) y2h_event_destroy(s->ev_box);
    free(s->plane_samples);
    free(s);
    e->depth = NULL;
}

const unsigned char *y2_depth_plane8(const y2_engine *e, int *W)
{
    const y2_depth_state *s = e->depth;
    if (!s || !s->have) { *W = 0; return NULL; }
    *W = s->W;
    return s->d8;
}

/* the grasp16 plane the filtered ingest also reads, or NULL while the grasp filter is off */
const unsigned short *y2_depth_plane_grasp(const y2_engine *e)
{
    const y2_depth_state *s = e->depth;
    return s && s->have && s->have_grasp && s->grasp_filter ? s->grasp16 : NULL;
}

/* ------------------------------------------------------------------ */
/* the rule of the plane removal, host-callable: include/y2_plane_rule.h */
/* ------------------------------------------------------------------ */
int y2_plane_samples(const uint16_t *depth, int dh, int dw, float far_m, int iters, unsigned seed, int *triples)
{
    const float far_mm = y2_plane_far_mm(far_m);
    unsigned state = seed, n;
    int k, filled = 0;
    if (!depth || !triples || dh <= 0 || dw <= 0 || dh > 32767 || dw > 32767 || iters < 0) return -1;
    n = (unsigned)dh * (unsigned)dw;
    for (k = 0; k < iters; ++k) {
        int *t = triples + 3 * k, have = 0, draw;
        for (draw = 0; draw < Y2_PLANE_MAX_DRAWS && have < 3; ++draw) {
            int idx;
            state = y2_plane_lcg(state);
            idx = (int)((state >> 8) % n);
            if (!(y2_plane_clip(depth[idx], far_mm) > 0)) continue;
            if ((have > 0 && t[0] == idx) || (have > 1 && t[1] == idx)) continue;
            t[have++] = idx;
        }
        if (have < 3) t[0] = t[1] = t[2] = -1;
        else ++filled;
    }
    return filled;
}

int y2_plane_from_points(const float *p0, const float *p1, const float *p2, float *plane)
{
    y2_plane_hyp h;
    if (!p0 || !p1 || !p2 || !plane) return 0;
    y2_plane_of_points(p0, p1, p2, &h);
    plane[0] = h.nx; plane[1] = h.ny; plane[2] = h.nz; plane[3] = h.d;
    return h.ok;
}

int y2_plane_fit(const double *sums, double *plane)
{
    if (!sums || !plane) return 0;
    return y2_plane_fit_sums(sums, plane);
}

int y2_otsu_threshold(const int hist[256])
{
    float pro[256], delta[256];
    long n = 0;
    int i;
    for (i = 0; i < 256; ++i) n += hist[i];
    if (y2_otsu_mostly_empty(hist[0], (int)n)) return 0;
    for (i = 0; i < 256; ++i) pro[i] = y2_otsu_prob(hist[i], i, (int)n - hist[0]);
    delta[0] = 0;
    for (i = 1; i < 256; ++i) delta[i] = y2_otsu_delta(pro, i);
    return y2_otsu_pick(delta);
}

int y2_depth_roi(box b, int W, int H, int *left, int *top, int *right, int *bot)
{
    y2_roi_axis(b.x, b.w, W, left, right);
    y2_roi_axis(b.y, b.h, H, top, bot);
    return *right > *left && *bot > *top;
}

/* the refusals of the filtered ingest that come on top of y2_ingest_regions', before any device work */
int y2_depth_filter_check(const char *who, network net, const y2_region *items, int n, const float *far_m)
{
    const y2_engine *e = y2_engine_of(&net);
    const y2_depth_state *s = e ? e->depth : NULL;
    int i, any = 0;
    for (i = 0; i < n; ++i) {
        if (!(far_m[i] > 0)) continue;
        any = 1;
        if (items[i].c < 3) { y2_fail("%s: item %d: the distance filter needs a colour frame, this one has %d channel(s)", who, i, items[i].c); return -1; }
    }
    if (!any) return 0;
    if (!s || !s->have) { y2_fail("%s: the distance filter needs a depth frame: call y2_depth_upload first", who); return -1; }
    if (s->grasp_filter && !s->have_grasp) {
        y2_fail("%s: the grasp filter needs a depth frame uploaded with plane removal on (y2_depth_set_plane_removal)", who);
        return -1;
    }
    for (i = 0; i < n; ++i)
        if (far_m[i] > 0 && (items[i].h != s->H || items[i].w != s->W)) {
            y2_fail("%s: item %d: the filtered frame is %d x %d, the uploaded depth frame is aligned to %d x %d", who, i,
                    items[i].w, items[i].h, s->W, s->H);
            return -1;
        }
    return 0;
}

static int depth_frame_check(const y2_depth_frame *f)
{
    if (!f || !f->depth) { y2_fail("y2_depth_upload: no depth frame"); return -1; }
    if (f->dh <= 0 || f->dw <= 0 || f->H <= 0 || f->W <= 0) { y2_fail("y2_depth_upload: bad geometry: depth %d x %d, colour %d x %d", f->dw, f->dh, f->W, f->H); return -1; }
    if (f->dh > 32767 || f->dw > 32767) { y2_fail("y2_depth_upload: a depth frame of %d x %d is more than 32767 pixels wide or high", f->dw, f->dh); return -1; }
    if (!f->map && (f->H != f->dh || f->W != f->dw)) {
        y2_fail("y2_depth_upload: without a map the depth frame (%d x %d) must have the colour frame's size (%d x %d)", f->dw, f->dh, f->W, f->H);
        return -1;
    }
    return 0;
}

int y2_depth_upload(network net, const y2_depth_frame *f)
{
    y2_engine *e;
    y2_depth_state *s;
    size_t npix, ndep, off_map, off_body, off_tri = 0, need, o16, oxy, o8, op, pneed, ogd = 0, og16 = 0, ocnt = 0, oslab = 0, orec = 0;
    int removal;
    if (depth_frame_check(f) != 0) return -1;
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    HIP_OR_ERR(y2h_set_device(e->device));
    s = state_of(e, 1);
    if (!s) { y2_fail("y2_depth_upload: out of memory"); return -1; }
    removal = s->plane.iters > 0;
    if (removal && (!s->d_tab || s->tab_dh != f->dh || s->tab_dw != f->dw)) {     /* before any copy */
        if (!s->d_tab) y2_fail("y2_depth_upload: plane removal needs the camera table (y2_depth_set_camera_table)");
        else y2_fail("y2_depth_upload: plane removal: the camera table is %d x %d, the depth frame %d x %d", s->tab_dw, s->tab_dh, f->dw, f->dh);
        return -1;
    }
    npix = (size_t)f->H * f->W; ndep = (size_t)f->dh * f->dw;
    off_map = align_up(ndep * 2, 256);
    off_body = off_map + (f->map ? align_up(npix * 8, 256) : 0);
    need = off_body + (f->body ? ndep : 0);
    o16 = 0; oxy = align_up(npix * 2, 256); o8 = oxy + align_up(npix * 4, 256); op = o8 + align_up(npix, 256);
    pneed = op + align_up(npix, 256);
    if (removal) {                       /* the triples ride behind the frame; the grasp planes and the work area behind the planes */
        off_tri = align_up(need, 256);
        need = off_tri + (size_t)s->plane.iters * 3 * sizeof(int);
        ogd = pneed; og16 = ogd + (f->map ? align_up(ndep * 2, 256) : 0);
        ocnt = og16 + align_up(npix * 2, 256);
        oslab = ocnt + align_up(Y2H_PLANE_COUNTS * sizeof(int), 256);
        orec = oslab + align_up(y2h_plane_chunks((long)ndep) * 10 * sizeof(double), 256);
        pneed = orec + align_up(sizeof(y2h_plane), 256);
    }
    if (s->up_pending) { HIP_OR_ERR(y2h_event_sync(s->ev_up)); s->up_pending = 0; }
    if (grow_pinned((void **)&s->h_stage, &s->h_stage_cap, need) || grow_dev((void **)&s->d_stage, &s->d_stage_cap, need) ||
        grow_dev((void **)&s->d_planes, &s->planes_cap, pneed)) {
        y2_fail("y2_depth_upload: %s", y2h_last_error()); return -1;
    }
    if (!s->ev_up) HIP_OR_ERR(y2h_event_create(&s->ev_up));
    s->have = 0; s->have_grasp = 0;
    memcpy(s->h_stage, f->depth, ndep * 2);
    if (f->map) memcpy(s->h_stage + off_map, f->map, npix * 8);
    if (f->body) memcpy(s->h_stage + off_body, f->body, ndep);
    if (removal) {                       /* the sampler runs here, on the caller's frame: only the triples go up */
        int *tri = (int *)(s->h_stage + off_tri);
        if (s->plane.samples) memcpy(tri, s->plane.samples, (size_t)s->plane.iters * 3 * sizeof(int));
        else y2_plane_samples(f->depth, f->dh, f->dw, s->plane.far_m, s->plane.iters, s->plane.seed, tri);
    }
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_stage, s->h_stage, need, e->stream));
    HIP_OR_ERR(y2h_event_record(s->ev_up, e->stream));
    s->up_pending = 1;
    s->d16 = (unsigned short *)(s->d_planes + o16); s->dxy = (short *)(s->d_planes + oxy);
    s->d8 = s->d_planes + o8; s->person = s->d_planes + op;
    HIP_OR_ERR(y2h_depth_align((const unsigned short *)s->d_stage, f->body ? s->d_stage + off_body : NULL,
                              f->map ? (const float *)(s->d_stage + off_map) : NULL, f->dh, f->dw, f->H, f->W, s->d16, s->d8,
                              s->person, s->dxy, e->stream));
    s->H = f->H; s->W = f->W; s->dh = f->dh; s->dw = f->dw; s->has_map = f->map != NULL;
    if (removal) {                       /* behind the align kernel on the same stream; nothing is left for the host */
        y2h_plane_job j;
        s->grasp_depth = (unsigned short *)(s->d_planes + ogd); s->grasp16 = (unsigned short *)(s->d_planes + og16);
        s->plane_rec = (y2h_plane *)(s->d_planes + orec);
        j.depth = (const unsigned short *)s->d_stage; j.tab = s->d_tab; j.triples = (const int *)(s->d_stage + off_tri);
        j.n = (long)ndep; j.iters = s->plane.iters;
        j.far_mm = y2_plane_far_mm(s->plane.far_m); j.dist_m = s->plane.dist_m;
        j.counts = (int *)(s->d_planes + ocnt); j.slab = (double *)(s->d_planes + oslab);
        j.rec = s->plane_rec; j.grasp_depth = s->grasp_depth;
        HIP_OR_ERR(y2h_plane_remove(&j, Y2H_PLANE_ALL, e->stream));
        if (f->map) HIP_OR_ERR(y2h_plane_register(s->grasp_depth, s->dxy, f->H, f->W, f->dw, s->grasp16, e->stream));
        s->have_grasp = 1;
    }
    s->have = 1;
    return 0;
}

int y2_depth_set_plane_removal(network net, const y2_plane_opts *o)
{
    static const char *who = "y2_depth_set_plane_removal";
    y2_engine *e;
    y2_depth_state *s;
    int *samples = NULL;
    const int on = o && o->iters > 0;
    if (on) {
        if (o->iters > Y2_PLANE_MAX_ITERS) { y2_fail("%s: %d hypotheses, at most %d", who, o->iters, Y2_PLANE_MAX_ITERS); return -1; }
        if (!(o->far_m > 0) || !(o->far_m <= 3.402823466e+38f)) { y2_fail("%s: far_m must be finite and > 0", who); return -1; }
        if (!(o->dist_m > 0) || !(o->dist_m <= 3.402823466e+38f)) { y2_fail("%s: dist_m must be finite and > 0", who); return -1; }
    }
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    s = state_of(e, 1);
    if (!s) { y2_fail("%s: out of memory", who); return -1; }
    if (on && o->samples) {
        samples = malloc((size_t)o->iters * 3 * sizeof(int));
        if (!samples) { y2_fail("%s: out of memory", who); return -1; }
        memcpy(samples, o->samples, (size_t)o->iters * 3 * sizeof(int));
    }
    free(s->plane_samples);
    s->plane_samples = samples;
    memset(&s->plane, 0, sizeof s->plane);
    if (on) { s->plane = *o; s->plane.samples = samples; }
    return 0;
}

int y2_depth_set_event(network net, int event)
{
    y2_engine *e;
    y2_depth_state *s;
    if (event != Y2_EVENT_DEMO_WHAT && event != Y2_EVENT_GRASP) { y2_fail("y2_depth_set_event: unknown event %d", event); return -1; }
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    s = state_of(e, 1);
    if (!s) { y2_fail("y2_depth_set_event: out of memory"); return -1; }
    s->event = event;
    return 0;
}

int y2_depth_set_grasp_filter(network net, int on)
{
    y2_engine *e;
    y2_depth_state *s;
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    s = state_of(e, 1);
    if (!s) { y2_fail("y2_depth_set_grasp_filter: out of memory"); return -1; }
    s->grasp_filter = on != 0;
    return 0;
}

int y2_depth_set_camera_table(network net, const float *tab, int dh, int dw)
{
    y2_engine *e;
    y2_depth_state *s;
    if (tab && (dh <= 0 || dw <= 0 || dh > 32767 || dw > 32767)) { y2_fail("y2_depth_set_camera_table: bad table size %d x %d", dw, dh); return -1; }
    if (y2_prepare(&net) != 0) return -1;
    e = y2_engine_of(&net);
    HIP_OR_ERR(y2h_set_device(e->device));
    s = state_of(e, 1);
    if (!s) { y2_fail("y2_depth_set_camera_table: out of memory"); return -1; }
    HIP_OR_ERR(y2h_stream_sync(e->stream));                 /* nothing in flight reads the old table */
    y2h_free(s->d_tab); s->d_tab = NULL; s->tab_dh = s->tab_dw = 0;
    if (!tab) return 0;
    HIP_OR_ERR(y2h_malloc((void **)&s->d_tab, (size_t)dh * dw * 2 * sizeof(float)));
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_tab, tab, (size_t)dh * dw * 2 * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));                 /* `tab` is the caller's pageable memory */
    s->tab_dh = dh; s->tab_dw = dw;
    return 0;
}

static y2_depth_state *uploaded(const char *who, network net, y2_engine **pe)
{
    y2_engine *e = y2_engine_of(&net);
    y2_depth_state *s = e ? e->depth : NULL;
    if (!s || !s->have) { y2_fail("%s: no depth frame has been uploaded (y2_depth_upload)", who); return NULL; }
    *pe = e;
    return s;
}

int y2_depth_aligned(network net, uint16_t *depth16, uint8_t *depth8, uint8_t *person)
{
    y2_engine *e;
    y2_depth_state *s = uploaded("y2_depth_aligned", net, &e);
    size_t npix;
    if (!s) return -1;
    HIP_OR_ERR(y2h_set_device(e->device));
    npix = (size_t)s->H * s->W;
    if (depth16) HIP_OR_ERR(y2h_memcpy_d2h(depth16, s->d16, npix * 2, e->stream));
    if (depth8) HIP_OR_ERR(y2h_memcpy_d2h(depth8, s->d8, npix, e->stream));
    if (person) HIP_OR_ERR(y2h_memcpy_d2h(person, s->person, npix, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* the Grasp statistics read the grasp16 plane of the uploaded frame: refused when that frame has none */
static int event_check(const char *who, const y2_depth_state *s)
{
    if (s->event == Y2_EVENT_GRASP && !s->have_grasp) {
        y2_fail("%s: the Grasp event needs a depth frame uploaded with plane removal on (y2_depth_set_plane_removal)", who);
        return -1;
    }
    return 0;
}

int y2_depth_plane(network net, y2_plane *out)
{
    y2_engine *e;
    y2_depth_state *s = uploaded("y2_depth_plane", net, &e);
    if (!s) return -1;
    if (!out) { y2_fail("y2_depth_plane: out is NULL"); return -1; }
    if (!s->have_grasp) { y2_fail("y2_depth_plane: the uploaded frame did not go through plane removal (y2_depth_set_plane_removal)"); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    HIP_OR_ERR(y2h_memcpy_d2h(out, s->plane_rec, sizeof *out, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_depth_grasp_aligned(network net, uint16_t *grasp_depth, uint16_t *grasp16)
{
    y2_engine *e;
    y2_depth_state *s = uploaded("y2_depth_grasp_aligned", net, &e);
    if (!s) return -1;
    if (!s->have_grasp) { y2_fail("y2_depth_grasp_aligned: the uploaded frame did not go through plane removal (y2_depth_set_plane_removal)"); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (grasp_depth) HIP_OR_ERR(y2h_memcpy_d2h(grasp_depth, s->grasp_depth, (size_t)s->dh * s->dw * 2, e->stream));
    if (grasp16) HIP_OR_ERR(y2h_memcpy_d2h(grasp16, s->grasp16, (size_t)s->H * s->W * 2, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

static void planes_of(const y2_depth_state *s, y2h_depth_planes *p)
{
    p->grasp16 = s->event == Y2_EVENT_GRASP ? s->grasp16 : NULL;
    p->depth16 = s->d16; p->depth8 = s->d8; p->person = s->person;
    p->dxy = s->has_map ? s->dxy : NULL;
    p->cam_table = s->d_tab;
    p->H = s->H; p->W = s->W;
    p->dh = s->d_tab ? s->tab_dh : s->dh; p->dw = s->d_tab ? s->tab_dw : s->dw;
}

/* scratch of one per-box call: [head: what the host sends | accumulators | results], head and results also pinned */
typedef struct { size_t head, acc, out, total; } box_layout;

static int box_scratch(const char *who, y2_depth_state *s, size_t head_bytes, long slots, box_layout *L)
{
    L->head = 0;
    L->acc = align_up(head_bytes, 256);
    L->out = L->acc + align_up((size_t)slots * y2h_depth_acc_bytes(), 256);
    L->total = L->out + align_up((size_t)slots * sizeof(y2h_det3d), 256);
    if (grow_dev((void **)&s->d_box, &s->d_box_cap, L->total) ||
        grow_pinned((void **)&s->h_box, &s->h_box_cap, L->acc + (size_t)slots * sizeof(y2h_det3d))) {
        y2_fail("%s: %s", who, y2h_last_error()); return -1;
    }
    if (!s->ev_box) HIP_OR_ERR(y2h_event_create(&s->ev_box));
    return 0;
}

int y2_depth_boxes(network net, const box *boxes, int n, y2_det3d *out)
{
    y2_engine *e;
    y2_depth_state *s;
    y2h_depth_planes p;
    box_layout L;
    if (!boxes || !out || n < 1 || n > 65535) { y2_fail("y2_depth_boxes: needs boxes, out and 1 <= n <= 65535"); return -1; }
    s = uploaded("y2_depth_boxes", net, &e);
    if (!s || event_check("y2_depth_boxes", s) != 0) return -1;
    HIP_OR_ERR(y2h_set_device(e->device));
    if (box_scratch("y2_depth_boxes", s, (size_t)n * sizeof(box), n, &L) != 0) return -1;
    planes_of(s, &p);
    memcpy(s->h_box, boxes, (size_t)n * sizeof(box));
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_box, s->h_box, (size_t)n * sizeof(box), e->stream));
    HIP_OR_ERR(y2h_depth_boxes(&p, (const float *)s->d_box, 4, n, NULL, NULL, 1, n, s->d_box + L.acc, (y2h_det3d *)(s->d_box + L.out),
                              Y2H_DEPTH_ALL, e->stream));
    HIP_OR_ERR(y2h_memcpy_d2h(s->h_box + L.acc, s->d_box + L.out, (size_t)n * sizeof(y2h_det3d), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    memcpy(out, s->h_box + L.acc, (size_t)n * sizeof(y2_det3d));
    return 0;
}

int y2_ingest_regions_depth(network net, const y2_region *items, int n, const float *far_m, int swap_rb, int letterbox)
{
    if (!far_m) { y2_fail("y2_ingest_regions_depth: far_m is NULL"); return -1; }
    return y2_ingest_regions_far("y2_ingest_regions_depth", net, items, n, far_m, swap_rb, letterbox);
}

int y2_detect_regions_depth(network net, const y2_region *items, int n, const float *far_m, int swap_rb, int letterbox,
                            float thresh, float nms, y2_det *dets, y2_det3d *d3, int *counts, int max_per_item)
{
    static const char *who = "y2_detect_regions_depth";
    y2_engine *e;
    y2_depth_state *s;
    y2h_depth_planes p;
    y2h_box_map *maps;
    y2h_stream ds;
    box_layout L;
    const unsigned char *rec;
    long eager, total = 0;
    int i, j, per_item;
    if (!dets || !d3 || !counts || max_per_item < 1) { y2_fail("%s: needs dets, d3, counts and max_per_item >= 1", who); return -1; }
    if (y2_regions_check(who, net, items, n, letterbox) != 0) return -1;
    if (far_m && y2_depth_filter_check(who, net, items, n, far_m) != 0) return -1;
    s = uploaded(who, net, &e);
    if (!s || event_check(who, s) != 0) return -1;
    if (y2_prepare(&net) != 0) return -1;                   /* det_cap belongs to the plan */
    e = y2_engine_of(&net);
    s = e->depth;
    HIP_OR_ERR(y2h_set_device(e->device));
    per_item = max_per_item < e->det_cap ? max_per_item : e->det_cap;
    if (box_scratch(who, s, (size_t)n * sizeof(y2h_box_map), (long)n * per_item, &L) != 0) return -1;
    planes_of(s, &p);
    maps = (y2h_box_map *)s->h_box;
    for (i = 0; i < n; ++i) {
        y2h_box_map *m = &maps[i];
        y2_region_rect(&items[i], &m->rx, &m->ry, &m->rw, &m->rh);
        m->letterbox = letterbox != 0;
        m->net_w = net.w; m->net_h = net.h; m->nw = net.w; m->nh = net.h;
        if (letterbox) y2h_letterbox_dims(m->rw, m->rh, net.w, net.h, &m->nw, &m->nh);
        m->fw = items[i].w; m->fh = items[i].h;
        m->whole = m->rx == 0 && m->ry == 0 && m->rw == m->fw && m->rh == m->fh;
    }
    HIP_OR_ERR(y2h_memcpy_h2d(s->d_box, s->h_box, (size_t)n * sizeof(y2h_box_map), e->stream));
    if (far_m) { if (y2_ingest_regions_far(who, net, items, n, far_m, swap_rb, letterbox) != 0) return -1; }
    else if (y2_ingest_regions(net, items, n, swap_rb, letterbox) != 0) return -1;
    if (y2_forward_device(net, NULL) != 0) return -1;
    if (y2_detect_chain_enqueue(net, thresh, nms) != 0) return -1;
    /* behind the chain on the stream it ran on: the records and counts it left in HBM are the box list */
    ds = (e->det_overlap && e->det_stream && net.layers[e->out_layer].type == REGION) ? e->det_stream : e->stream;
    HIP_OR_ERR(y2h_depth_boxes(&p, e->d_records, 6, e->det_cap, e->d_counts, (const y2h_box_map *)s->d_box, n, per_item,
                              s->d_box + L.acc, (y2h_det3d *)(s->d_box + L.out), Y2H_DEPTH_ALL, ds));
    /* the kernels write the records densely, so a fixed, small prefix is fetched with no count on the host; only a frame
     * with more detections than that pays a second copy, once the counts are here */
    eager = (long)n * per_item < Y2_DEPTH_EAGER ? (long)n * per_item : Y2_DEPTH_EAGER;
    HIP_OR_ERR(y2h_memcpy_d2h(s->h_box + L.acc, s->d_box + L.out, (size_t)eager * sizeof(y2h_det3d), ds));
    HIP_OR_ERR(y2h_event_record(s->ev_box, ds));
    if (y2_detect_chain_fetch(net, dets, counts, max_per_item, n) != 0) {
        y2h_event_sync(s->ev_box);                          /* that copy lands in h_box: let it, before anyone refills it */
        return -1;
    }
    HIP_OR_ERR(y2h_event_sync(s->ev_box));
    for (i = 0; i < n; ++i) total += counts[i] < per_item ? counts[i] : per_item;
    if (total > eager) {
        HIP_OR_ERR(y2h_memcpy_d2h(s->h_box + L.acc + (size_t)eager * sizeof(y2h_det3d), s->d_box + L.out + (size_t)eager * sizeof(y2h_det3d),
                                 (size_t)(total - eager) * sizeof(y2h_det3d), ds));
        HIP_OR_ERR(y2h_stream_sync(ds));
    }
    rec = s->h_box + L.acc;
    for (i = 0; i < n; ++i) {
        const int kept = counts[i] < per_item ? counts[i] : per_item;
        for (j = 0; j < kept; ++j) {
            y2_det *d = &dets[(size_t)i * max_per_item + j];
            y2_region_box_to_frame(&items[i], net.w, net.h, letterbox, &d->x, &d->y, &d->w, &d->h);
            memcpy(&d3[(size_t)i * max_per_item + j], rec, sizeof(y2_det3d));
            rec += sizeof(y2h_det3d);
        }
    }
    return 0;
}

void test_detector_regions_depth(char **names, network net, const y2_region *items, int n, const float *far_m, float thresh,
                                 object **RecObjects, int *objectNumPerRegion)
{
    const float nms = 0.1f;
    layer l = net.layers[net.n - 1];
    int total = l.w * l.h * l.n, i, j;
    y2_det *dets;
    y2_det3d *d3;
    int *counts;
    if (!RecObjects || !objectNumPerRegion) { y2_fail("test_detector_regions_depth: RecObjects / objectNumPerRegion is NULL"); return; }
    if (y2_regions_check("test_detector_regions_depth", net, items, n, 0) != 0) return;
    if (total < 1) total = 1;
    dets = calloc((size_t)n * total, sizeof(y2_det));
    d3 = calloc((size_t)n * total, sizeof(y2_det3d));
    counts = calloc((size_t)n, sizeof(int));
    if (!dets || !d3 || !counts) { free(dets); free(d3); free(counts); y2_fail("test_detector_regions_depth: out of memory"); return; }
    if (y2_detect_regions_depth(net, items, n, far_m, 1, 0, thresh, nms, dets, d3, counts, total) != 0) { free(dets); free(d3); free(counts); return; }
    for (i = 0; i < n; ++i) {
        const int kept = counts[i] < total ? counts[i] : total;
        for (j = 0; j < kept; ++j) {
            const y2_det3d *t = &d3[(size_t)i * total + j];
            object *o = &RecObjects[i][objectNumPerRegion[i]];
            y2_fill_object(o, &dets[(size_t)i * total + j], names, l.classes);
            o->CameraX = t->cam_x; o->CameraY = t->cam_y; o->CameraZ = t->cam_z;
            o->CameraWidth = t->cam_w; o->CameraHeight = t->cam_h;
            o->flagBelong2Person = (unsigned char)t->belongs;
            o->bodyId = t->body_id;
            objectNumPerRegion[i]++;
        }
    }
    free(dets); free(d3); free(counts);
}
