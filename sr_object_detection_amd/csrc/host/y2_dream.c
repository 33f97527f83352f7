/*
 * Dreaming on the device: host-side replacement for src_yolo2/nightmare.c -- optimize_picture (:34-115) and the loop of
 * run_nightmare (:258-306).  The gradient of a layer's activations with respect to the input picture: the forward pass of
 * the network truncated behind max_layer, calculate_loss on its last layer, the backward pass WITH a delta for layer 0
 * (the trainer hands layer 0 none: network.c:204-206), and the picture's update.
 *
 * The convolution products, the maxpool pair and gradient_array are the trainer's kernels (y2h_train_*), fp32 only; the
 * picture side -- crop, resize, flip in both directions, calculate_loss, normalize / axpy / constrain, rotate and zoom --
 * is y2_dream.hip.  The picture lives in HBM from y2_dream_open to y2_dream_close; a step copies nothing to or from the
 * host and does not wait for the device.
 *
 * Nothing of the caller's network is changed: the reference sets net->n and calls resize_network, here the geometry of
 * the truncated network at the step's size is worked out by resize_network's rules into the context's own tables.  Per
 * input size the context keeps one set of buffers (input, image gradient, per layer output / delta / maxpool winners,
 * batch 1, dense NHWC), at most DREAM_SETS of them, the least recently used dropped; a set grows when a step asks for a
 * deeper layer than it holds.  The weights of the layers used are packed once in the trainer's [size][size][c][n] layout
 * and again when the engine's weights_gen has moved (load_weights, y2_denormalize_network, a trainer's sync).
 *
 * Not reproduced: weight_updates and bias_updates.  backward_convolutional_layer accumulates them, optimize_picture never
 * applies or reads them, so a third of the products is left out.  reconstruct_picture / smooth (-reconstruct) are out of
 * scope: that branch hard-codes 14*14*512 features of a cfg the reference does not ship.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

#define DREAM_SETS 8

typedef struct {
    int h, w, c, out_h, out_w, out_c;
    float *out, *delta;
    int *idx;
} dream_layer;

typedef struct {
    int w, h, layers;               /* the input size; buffers exist for layers 0 .. layers-1 */
    unsigned long used;
    float *in, *grad;               /* [h][w][c] */
    dream_layer *L;                 /* net->n entries */
} dream_set;

struct y2_dream {
    network *net;
    y2_engine *e;
    int c, h, w;
    float *pic, *alt, *upd;         /* the picture, rotate_image's result, the picture-sized update: [c][h][w] */
    float *tmp;                     /* the resamples' column pass; NCHW staging of y2_dream_pull (grow-only) */
    size_t tmp_floats;
    float *partials, *stat;         /* 2 * chunks of the larger reduction; mean, variance */
    size_t partial_floats;
    int *selected;
    float **weights, **biases;      /* per layer, NULL until packed */
    unsigned long gen;              /* the engine's weights_gen they were packed at */
    float *pin;                     /* pinned landing buffer of every copy (grow-only) */
    size_t pin_floats;
    dream_set sets[DREAM_SETS];
    unsigned long clock;
    dream_set *last;                /* the last step's buffers and its depth, for y2_dream_pull */
    int last_layer;
    y2_dream_counters st;
};

/* ------------------------------------------------------------------ */
/* host functions: the draws and the sizes                             */
/* ------------------------------------------------------------------ */
void y2_dream_draw(int range, int octaves, y2_dream_draws *out)
{
    if (!out) return;
    if (range < 1) range = 1;
    if (octaves < 1) octaves = 1;
    out->layer_offset = rand() % range - range / 2;     /* nightmare.c:274-275 */
    out->octave = rand() % octaves;
    out->dx = rand() % 16 - 8;                          /* nightmare.c:40-42 */
    out->dy = rand() % 16 - 8;
    out->flip = rand() % 2;
}

float y2_dream_scale(int octave) { return 1 / pow(1.33333333, octave); }

void y2_dream_size(int w, int h, float scale, int *ow, int *oh)
{
    if (ow) *ow = (int)(w * scale);
    if (oh) *oh = (int)(h * scale);
}

/* ------------------------------------------------------------------ */
/* refusals and geometry: no device call                               */
/* ------------------------------------------------------------------ */
/* resize_network's rules (y2_engine.c) for the layers a dream takes; L may be NULL */
static int geometry(const network *net, int max_layer, int w, int h, dream_layer *L)
{
    int i, c = net->c;
    for (i = 0; i <= max_layer; ++i) {
        const layer *l = &net->layers[i];
        dream_layer g = { h, w, c, 0, 0, 0, NULL, NULL, NULL };
        if (l->type == CONVOLUTIONAL) {
            g.out_w = (w + 2 * l->pad - l->size) / l->stride + 1;
            g.out_h = (h + 2 * l->pad - l->size) / l->stride + 1;
            g.out_c = l->n;
            if (w + 2 * l->pad < l->size || h + 2 * l->pad < l->size) g.out_w = g.out_h = 0;
        } else {
            g.out_w = (w + 2 * l->pad) / l->stride;
            g.out_h = (h + 2 * l->pad) / l->stride;
            g.out_c = c;
        }
        if (g.out_w <= 0 || g.out_h <= 0) return i;
        if (L) { g.out = L[i].out; g.delta = L[i].delta; g.idx = L[i].idx; L[i] = g; }
        w = g.out_w; h = g.out_h; c = g.out_c;
    }
    return -1;
}

int y2_dream_check(network *net, int max_layer, int c, int h, int w, float scale)
{
    const y2_engine *e = net ? y2_engine_of(net) : NULL;
    int i, sw, sh, chan;
    if (!e || !net->layers || net->n <= 0) { y2_fail("dream: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (max_layer < 0 || max_layer >= net->n) { y2_fail("dream: max_layer %d is outside the network's %d layers", max_layer, net->n); return -1; }
    if (net->batch != 1) { y2_fail("dream: the network is at batch %d: set_batch_network(&net, 1) first, as run_nightmare does", net->batch); return -1; }
    if (e->half) { y2_fail("dream: fp32 only: the network is in fp16 mode (y2_set_half / Y2_FP16)"); return -1; }
    if (c <= 0 || h <= 0 || w <= 0) { y2_fail("dream: a picture of %d x %d x %d", w, h, c); return -1; }
    if (c != net->c) { y2_fail("dream: the picture has %d channels, the network takes %d", c, net->c); return -1; }
    chan = net->c;
    for (i = 0; i <= max_layer; ++i) {
        const layer *l = &net->layers[i];
        const char *t = get_layer_string(l->type);
        switch (l->type) {
        case CONVOLUTIONAL:
            if (l->batch_normalize) {
                y2_fail("dream: layer %d (%s): batch_normalize=1 is refused: the reference's backward pass with train = 0 swaps in the "
                        "rolling statistics and then runs the training-mode batch-norm backward on them (fold it first: y2_denormalize_network)", i, t);
                return -1;
            }
            if (l->stride != 1) { y2_fail("dream: layer %d (%s): stride %d is refused (stride 1 only)", i, t, l->stride); return -1; }
            if (l->xnor || l->binary) { y2_fail("dream: layer %d (%s): xnor / binary weights are refused", i, t); return -1; }
            if (l->activation != LINEAR && l->activation != LEAKY && l->activation != LOGISTIC && l->activation != RELU) {
                y2_fail("dream: layer %d (%s): activation %d is refused (linear, leaky, logistic, relu)", i, t, (int)l->activation);
                return -1;
            }
            if (l->c != chan || l->size <= 0 || l->n <= 0) { y2_fail("dream: layer %d (%s): it reads %d channels, the layer in front gives %d", i, t, l->c, chan); return -1; }
            chan = l->n;
            break;
        case MAXPOOL:
            if (l->size <= 0 || l->stride <= 0 || l->pad < 0) { y2_fail("dream: layer %d (%s): size %d stride %d padding %d", i, t, l->size, l->stride, l->pad); return -1; }
            break;
        default:
            y2_fail("dream: layer %d (%s): this section type is refused (convolutional without batch_normalize, maxpool)", i, t);
            return -1;
        }
    }
    y2_dream_size(w, h, scale, &sw, &sh);
    if (!(scale > 0) || sw <= 0 || sh <= 0) { y2_fail("dream: layer 0 (%s): scale %g leaves a %d x %d picture no pixel", get_layer_string(net->layers[0].type), scale, w, h); return -1; }
    i = geometry(net, max_layer, sw, sh, NULL);
    if (i >= 0) { y2_fail("dream: layer %d (%s): no pixel is left at scale %g (input %d x %d)", i, get_layer_string(net->layers[i].type), scale, sw, sh); return -1; }
    return 0;
}

/* ------------------------------------------------------------------ */
/* buffers                                                             */
/* ------------------------------------------------------------------ */
static int dev_alloc(y2_dream *d, void **p, size_t bytes)
{
    HIP_OR_ERR(y2h_malloc(p, bytes ? bytes : 4));
    d->st.allocations++;
    return 0;
}

static int grow(y2_dream *d, float **p, size_t *have, size_t need)
{
    if (need <= *have) return 0;
    y2h_stream_sync(d->e->stream);          /* work in flight may still read the old one */
    y2h_free(*p); *p = NULL; *have = 0;
    if (dev_alloc(d, (void **)p, need * sizeof(float)) != 0) return -1;
    *have = need;
    return 0;
}

static int grow_pin(y2_dream *d, size_t need)
{
    if (need <= d->pin_floats) return 0;
    y2h_host_free(d->pin); d->pin = NULL; d->pin_floats = 0;
    HIP_OR_ERR(y2h_host_alloc((void **)&d->pin, need * sizeof(float)));
    d->pin_floats = need;
    return 0;
}

static int push(y2_dream *d, float *dst, const float *src, size_t n)
{
    if (grow_pin(d, n) != 0) return -1;
    memcpy(d->pin, src, n * sizeof(float));
    HIP_OR_ERR(y2h_memcpy_h2d(dst, d->pin, n * sizeof(float), d->e->stream));
    HIP_OR_ERR(y2h_stream_sync(d->e->stream));
    d->st.h2d_bytes += n * sizeof(float);
    return 0;
}

static int pull(y2_dream *d, const void *src, void *dst, size_t bytes)
{
    if (grow_pin(d, (bytes + 3) / 4) != 0) return -1;
    HIP_OR_ERR(y2h_memcpy_d2h(d->pin, src, bytes, d->e->stream));
    HIP_OR_ERR(y2h_stream_sync(d->e->stream));
    memcpy(dst, d->pin, bytes);
    d->st.d2h_bytes += bytes;
    return 0;
}

static void free_set(dream_set *s, int n)
{
    int i;
    if (s->L) for (i = 0; i < n; ++i) { y2h_free(s->L[i].out); y2h_free(s->L[i].delta); y2h_free(s->L[i].idx); }
    free(s->L);
    y2h_free(s->in); y2h_free(s->grad);
    memset(s, 0, sizeof *s);
}

/* the buffers of input size (w, h), deep enough for max_layer */
static dream_set *set_for(y2_dream *d, int w, int h, int max_layer)
{
    dream_set *s = NULL, *lru = NULL;
    int k, i;
    for (k = 0; k < DREAM_SETS && !s; ++k)
        if (d->sets[k].L && d->sets[k].w == w && d->sets[k].h == h) s = &d->sets[k];
    if (!s) {
        for (k = 0; k < DREAM_SETS; ++k) {          /* a free slot, or the least recently used */
            if (!d->sets[k].L) { lru = &d->sets[k]; break; }
            if (!lru || d->sets[k].used < lru->used) lru = &d->sets[k];
        }
        s = lru;
        if (s->L) {
            y2h_stream_sync(d->e->stream);
            if (d->last == s) d->last = NULL;
            free_set(s, d->net->n);
        }
        s->w = w; s->h = h; s->layers = 0;
        s->L = calloc(d->net->n, sizeof *s->L);
        if (dev_alloc(d, (void **)&s->in, (size_t)w * h * d->c * sizeof(float)) != 0 ||
            dev_alloc(d, (void **)&s->grad, (size_t)w * h * d->c * sizeof(float)) != 0) { free_set(s, d->net->n); return NULL; }
    }
    if (s->layers <= max_layer) {
        geometry(d->net, max_layer, w, h, s->L);
        for (i = s->layers; i <= max_layer; ++i) {
            dream_layer *L = &s->L[i];
            const size_t outs = (size_t)L->out_h * L->out_w * L->out_c;
            if (dev_alloc(d, (void **)&L->out, outs * sizeof(float)) != 0 || dev_alloc(d, (void **)&L->delta, outs * sizeof(float)) != 0 ||
                (d->net->layers[i].type == MAXPOOL && dev_alloc(d, (void **)&L->idx, outs * sizeof(int)) != 0)) {
                if (d->last == s) d->last = NULL;
                free_set(s, d->net->n);
                return NULL;
            }
            s->layers = i + 1;
        }
    }
    s->used = ++d->clock;
    return s;
}

/* the masters of layers 0 .. max_layer, packed once per weights_gen */
static int pack_weights(y2_dream *d, int max_layer)
{
    network *net = d->net;
    int i;
    if (y2_train_sync_if_dirty(net) != 0) return -1;        /* a trainer's steps reach the host arrays first, as in network_predict */
    if (d->gen != d->e->weights_gen) {
        y2h_stream_sync(d->e->stream);
        for (i = 0; i < net->n; ++i) { y2h_free(d->weights[i]); y2h_free(d->biases[i]); d->weights[i] = d->biases[i] = NULL; }
        d->gen = d->e->weights_gen;
    }
    for (i = 0; i <= max_layer; ++i) {
        const layer *l = &net->layers[i];
        const size_t nw = (size_t)l->n * l->c * l->size * l->size;
        float *tmp;
        int rc;
        if (l->type != CONVOLUTIONAL || d->weights[i]) continue;
        if (dev_alloc(d, (void **)&d->weights[i], nw * sizeof(float)) != 0 || dev_alloc(d, (void **)&d->biases[i], (size_t)l->n * sizeof(float)) != 0) return -1;
        tmp = malloc(nw * sizeof(float));
        y2_train_pack_weights(l->weights, tmp, l->n, l->c, l->size);
        rc = push(d, d->weights[i], tmp, nw) || push(d, d->biases[i], l->biases, l->n);
        free(tmp);
        if (rc) { y2h_free(d->weights[i]); y2h_free(d->biases[i]); d->weights[i] = d->biases[i] = NULL; return -1; }
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* lifecycle                                                           */
/* ------------------------------------------------------------------ */
void y2_dream_close(y2_dream *d)
{
    int i;
    if (!d) return;
    y2h_set_device(d->e->device);
    if (d->e->stream) y2h_stream_sync(d->e->stream);
    for (i = 0; i < DREAM_SETS; ++i) free_set(&d->sets[i], d->net->n);
    if (d->weights) for (i = 0; i < d->net->n; ++i) { y2h_free(d->weights[i]); y2h_free(d->biases[i]); }
    free(d->weights); free(d->biases);
    y2h_free(d->pic); y2h_free(d->alt); y2h_free(d->upd); y2h_free(d->tmp); y2h_free(d->partials); y2h_free(d->stat); y2h_free(d->selected);
    y2h_host_free(d->pin);
    if (d->e->dream == d) d->e->dream = NULL;
    free(d);
}

void y2_dream_free_cached(y2_engine *e)
{
    if (e && e->dream) y2_dream_close(e->dream);
}

static int open_buffers(y2_dream *d, const float *picture, size_t n)
{
    if (dev_alloc(d, (void **)&d->pic, n * sizeof(float)) != 0 || dev_alloc(d, (void **)&d->alt, n * sizeof(float)) != 0 ||
        dev_alloc(d, (void **)&d->upd, n * sizeof(float)) != 0 || dev_alloc(d, (void **)&d->stat, 2 * sizeof(float)) != 0 ||
        dev_alloc(d, (void **)&d->selected, sizeof(int)) != 0 ||
        grow(d, &d->partials, &d->partial_floats, 2 * (size_t)y2h_dream_chunks((long)n)) != 0 || grow(d, &d->tmp, &d->tmp_floats, n) != 0) return -1;
    HIP_OR_ERR(y2h_memset(d->selected, 0, sizeof(int), d->e->stream));
    HIP_OR_ERR(y2h_memset(d->stat, 0, 2 * sizeof(float), d->e->stream));
    HIP_OR_ERR(y2h_memset(d->upd, 0, n * sizeof(float), d->e->stream));
    return push(d, d->pic, picture, n);
}

y2_dream *y2_dream_open(network *net, const float *picture, int c, int h, int w)
{
    y2_engine *e;
    y2_dream *d;
    size_t n;
    if (!picture) { y2_fail("y2_dream_open: NULL picture"); return NULL; }
    if (y2_dream_check(net, 0, c, h, w, 1.f) != 0) return NULL;
    e = y2_engine_of(net);
    if (y2h_set_device(e->device) != 0) { y2_fail("y2_dream_open: %s", y2h_last_error()); return NULL; }
    if (!e->stream && y2h_stream_create(&e->stream) != 0) { y2_fail("y2_dream_open: %s", y2h_last_error()); return NULL; }
    d = calloc(1, sizeof *d);
    d->net = net; d->e = e; d->c = c; d->h = h; d->w = w;
    d->gen = e->weights_gen;
    d->weights = calloc(net->n, sizeof *d->weights);
    d->biases = calloc(net->n, sizeof *d->biases);
    n = (size_t)c * h * w;
    if (open_buffers(d, picture, n) != 0) { y2_dream_close(d); return NULL; }
    return d;
}

/* ------------------------------------------------------------------ */
/* the step                                                            */
/* ------------------------------------------------------------------ */
int y2_dream_step(y2_dream *d, int max_layer, float scale, float rate, float thresh, int norm, int dx, int dy, int flip)
{
    network *net;
    y2_engine *e;
    dream_set *s;
    int sw, sh, i;
    long n;
    if (!d) { y2_fail("y2_dream_step: NULL context"); return -1; }
    net = d->net; e = d->e;
    if (y2_dream_check(net, max_layer, d->c, d->h, d->w, scale) != 0) return -1;
    HIP_OR_ERR(y2h_set_device(e->device));
    if (pack_weights(d, max_layer) != 0) return -1;
    y2_dream_size(d->w, d->h, scale, &sw, &sh);
    if (!(s = set_for(d, sw, sh, max_layer))) return -1;
    {   /* the last layer's reduction may be longer than the picture's */
        const dream_layer *last = &s->L[max_layer];
        size_t need = 2 * (size_t)y2h_dream_chunks((long)last->out_h * last->out_w * last->out_c);
        if (grow(d, &d->partials, &d->partial_floats, need) != 0) return -1;
    }
    {   /* nightmare.c:44-46: crop_image(orig, dx, dy), resize_image, flip_image -> the NHWC input */
        y2h_dream_resample r = { d->c, d->h, d->w, 0, 0, dx, dy, d->h, d->w, sh, sw, 0, 0, 1, flip != 0 };
        if (grow(d, &d->tmp, &d->tmp_floats, y2h_dream_resample_tmp_floats(&r)) != 0) return -1;
        HIP_OR_ERR(y2h_dream_resample_run(&r, d->pic, d->tmp, s->in, e->stream));
    }
    for (i = 0; i <= max_layer; ++i) {              /* forward_network, train = 0 */
        const layer *l = &net->layers[i];
        dream_layer *L = &s->L[i];
        const float *in = i ? s->L[i - 1].out : s->in;
        if (l->type == CONVOLUTIONAL) {
            const y2h_train_conv g = { 1, L->h, L->w, L->c, l->n, l->size, l->pad, L->out_h, L->out_w };
            HIP_OR_ERR(y2h_train_conv_forward(&g, in, d->weights[i], L->out, e->stream));
            HIP_OR_ERR(y2h_train_bn_apply(L->out, NULL, NULL, NULL, NULL, NULL, d->biases[i], y2_act_code(l->activation),
                                          (long)L->out_h * L->out_w, l->n, e->stream));
        } else {
            HIP_OR_ERR(y2h_train_maxpool_forward(in, L->out, L->idx, 1, L->h, L->w, L->c, l->size, l->stride, l->pad, L->out_h, L->out_w, e->stream));
        }
    }
    n = (long)s->L[max_layer].out_h * s->L[max_layer].out_w * s->L[max_layer].out_c;
    HIP_OR_ERR(y2h_dream_loss(s->L[max_layer].out, s->L[max_layer].delta, n, thresh, d->partials, d->stat, d->selected, e->stream));
    for (i = max_layer; i >= 0; --i) {              /* backward_network with a state.delta for layer 0 */
        const layer *l = &net->layers[i];
        dream_layer *L = &s->L[i];
        float *din = i ? s->L[i - 1].delta : s->grad;
        if (l->type == CONVOLUTIONAL) {
            const y2h_train_conv g = { 1, L->h, L->w, L->c, l->n, l->size, l->pad, L->out_h, L->out_w };
            HIP_OR_ERR(y2h_train_act_gradient(L->out, L->delta, y2_act_code(l->activation), (long)L->out_h * L->out_w * l->n, e->stream));
            HIP_OR_ERR(y2h_train_conv_dinput(&g, L->delta, d->weights[i], din, e->stream));
        } else {
            HIP_OR_ERR(y2h_train_maxpool_backward(L->delta, L->idx, din, 1, L->h, L->w, L->c, l->size, l->stride, l->pad, L->out_h, L->out_w, e->stream));
        }
    }
    {   /* nightmare.c:81-84: flip_image(delta), resize_image to the picture's size, crop_image(., -dx, -dy) */
        y2h_dream_resample r = { d->c, sh, sw, 1, flip != 0, 0, 0, sh, sw, d->h, d->w, -dx, -dy, 0, 0 };
        if (grow(d, &d->tmp, &d->tmp_floats, y2h_dream_resample_tmp_floats(&r)) != 0) return -1;
        HIP_OR_ERR(y2h_dream_resample_run(&r, s->grad, d->tmp, d->upd, e->stream));
    }
    /* nightmare.c:94-107: normalize_array, axpy_cpu, constrain_image */
    HIP_OR_ERR(y2h_dream_apply(d->pic, d->upd, (long)d->c * d->h * d->w, rate, norm, d->partials, d->stat, e->stream));
    d->last = s; d->last_layer = max_layer;
    d->st.steps++;
    return 0;
}

int y2_dream_round_end(y2_dream *d, float rotate, float zoom)
{
    y2_engine *e;
    const float *src;
    int cx, cy, cw, ch;
    if (!d) { y2_fail("y2_dream_round_end: NULL context"); return -1; }
    e = d->e;
    /* nightmare.c:301: crop_image(im, im.w * (1. - zoom)/2., im.h * (1.-zoom)/2., im.w*zoom, im.h*zoom) */
    cx = d->w * (1. - zoom) / 2.;
    cy = d->h * (1. - zoom) / 2.;
    cw = d->w * zoom;
    ch = d->h * zoom;
    if (cw <= 0 || ch <= 0) { y2_fail("y2_dream_round_end: zoom %g leaves a %d x %d picture no pixel", zoom, d->w, d->h); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    src = d->pic;
    if (rotate) {
        HIP_OR_ERR(y2h_dream_rotate(d->pic, d->alt, d->c, d->h, d->w, cos(rotate), sin(rotate), e->stream));
        src = d->alt;
    }
    {
        y2h_dream_resample r = { d->c, d->h, d->w, 0, 0, cx, cy, ch, cw, d->h, d->w, 0, 0, 0, 0 };
        if (grow(d, &d->tmp, &d->tmp_floats, y2h_dream_resample_tmp_floats(&r)) != 0) return -1;
        HIP_OR_ERR(y2h_dream_resample_run(&r, src, d->tmp, d->pic, e->stream));
    }
    return 0;
}

static int upload(y2_dream *d, const float *picture)
{
    HIP_OR_ERR(y2h_set_device(d->e->device));
    return push(d, d->pic, picture, (size_t)d->c * d->h * d->w);
}

int y2_dream_fetch(y2_dream *d, float *picture)
{
    if (!d || !picture) { y2_fail("y2_dream_fetch: NULL argument"); return -1; }
    HIP_OR_ERR(y2h_set_device(d->e->device));
    return pull(d, d->pic, picture, (size_t)d->c * d->h * d->w * sizeof(float));
}

int y2_dream_stats(y2_dream *d, y2_dream_counters *out)
{
    if (!d || !out) { y2_fail("y2_dream_stats: NULL argument"); return -1; }
    HIP_OR_ERR(y2h_set_device(d->e->device));
    if (pull(d, d->selected, &d->st.selected, sizeof(int)) != 0) return -1;
    *out = d->st;
    return 0;
}

int y2_dream_pull(y2_dream *d, int layer, int what, float *dst, size_t n)
{
    const float *src = NULL;
    int c = 0, h = 0, w = 0, nhwc = 1;
    if (!d || !dst) { y2_fail("y2_dream_pull: NULL argument"); return -1; }
    if (what == Y2_DREAM_UPDATE) { src = d->upd; c = d->c; h = d->h; w = d->w; nhwc = 0; }
    else if (!d->last) { y2_fail("y2_dream_pull: no step has run"); return -1; }
    else if (what == Y2_DREAM_INPUT || what == Y2_DREAM_GRADIENT) {
        src = what == Y2_DREAM_INPUT ? d->last->in : d->last->grad; c = d->c; h = d->last->h; w = d->last->w;
    } else if (what == Y2_DREAM_OUTPUT || what == Y2_DREAM_DELTA) {
        const dream_layer *L;
        if (layer < 0 || layer > d->last_layer) { y2_fail("y2_dream_pull: layer %d: the last step ran layers 0 .. %d", layer, d->last_layer); return -1; }
        L = &d->last->L[layer];
        src = what == Y2_DREAM_OUTPUT ? L->out : L->delta; c = L->out_c; h = L->out_h; w = L->out_w;
    }
    if (!src) { y2_fail("y2_dream_pull: no array %d", what); return -1; }
    if (n != (size_t)c * h * w) { y2_fail("y2_dream_pull: array %d holds %zu floats, not %zu", what, (size_t)c * h * w, n); return -1; }
    HIP_OR_ERR(y2h_set_device(d->e->device));
    if (nhwc && h * w > 1 && c > 1) {
        if (grow(d, &d->tmp, &d->tmp_floats, n) != 0) return -1;
        HIP_OR_ERR(y2h_nhwc_to_nchw(src, c, d->tmp, 1, c, h, w, d->e->stream));
        src = d->tmp;
    }
    return pull(d, src, dst, n * sizeof(float));
}

/* ------------------------------------------------------------------ */
/* the reference's entry points                                        */
/* ------------------------------------------------------------------ */
void optimize_picture(network *net, image orig, int max_layer, float scale, float rate, float thresh, int norm)
{
    y2_engine *e = net ? y2_engine_of(net) : NULL;
    y2_dream *d;
    int dx, dy, flip;
    if (!orig.data) { y2_fail("optimize_picture: NULL picture"); return; }
    if (y2_dream_check(net, max_layer, orig.c, orig.h, orig.w, scale) != 0) return;
    dx = rand() % 16 - 8;
    dy = rand() % 16 - 8;
    flip = rand() % 2;
    d = e->dream;
    if (d && (d->c != orig.c || d->h != orig.h || d->w != orig.w)) { y2_dream_close(d); d = NULL; }
    if (d) { if (upload(d, orig.data) != 0) return; }
    else if (!(d = e->dream = y2_dream_open(net, orig.data, orig.c, orig.h, orig.w))) return;
    if (y2_dream_step(d, max_layer, scale, rate, thresh, norm, dx, dy, flip) != 0) return;
    y2_dream_fetch(d, orig.data);
}

int y2_nightmare(network *net, image im, int max_layer, int range, int norm, int rounds, int iters, int octaves, float zoom,
                 float rate, float thresh, float rotate, void (*per_round)(int round, image im, void *user), void *user)
{
    y2_dream *d;
    int e, n, rc = -1;
    if (!im.data) { y2_fail("y2_nightmare: NULL picture"); return -1; }
    if (range < 1 || octaves < 1 || rounds < 0 || iters < 0) { y2_fail("y2_nightmare: range %d octaves %d rounds %d iters %d", range, octaves, rounds, iters); return -1; }
    /* every layer and size the draws can ask for, before anything is allocated */
    if (y2_dream_check(net, max_layer - range / 2, im.c, im.h, im.w, 1.f) != 0 ||
        y2_dream_check(net, max_layer + range - 1 - range / 2, im.c, im.h, im.w, y2_dream_scale(octaves - 1)) != 0) return -1;
    if (!(d = y2_dream_open(net, im.data, im.c, im.h, im.w))) return -1;
    for (e = 0; e < rounds; ++e) {
        for (n = 0; n < iters; ++n) {
            y2_dream_draws w;
            y2_dream_draw(range, octaves, &w);
            if (y2_dream_step(d, max_layer + w.layer_offset, y2_dream_scale(w.octave), rate, thresh, norm, w.dx, w.dy, w.flip) != 0) goto done;
        }
        if (y2_dream_fetch(d, im.data) != 0) goto done;
        if (per_round) per_round(e, im, user);
        if (y2_dream_round_end(d, rotate, zoom) != 0) goto done;
    }
    rc = 0;
done:
    y2_dream_close(d);
    return rc;
}
