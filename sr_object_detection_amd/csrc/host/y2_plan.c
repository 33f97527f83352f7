/*
 * The plan of a network: where every layer's activations live, what is fused or aliased away, how the input reaches
 * layer 0, which kernel runs each convolution.  y2_engine_build (at the end) is the list of passes; each pass decides one
 * thing, and the helpers in front of them (conv descriptor, input view, input form) are what the forward pass reads the
 * decisions through.  Built lazily at the first predict after parse / resize / set_batch.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <pthread.h>
#include <string.h>
#include "y2_internal.h"

void y2_free_plan(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    if (!e) return;
    for (i = 0; i < net->n; ++i) {
        y2_ldev *d = ld_of(&net->layers[i]);
        if (!d) continue;
        y2h_free(d->out_alloc); d->out_alloc = NULL; d->out = NULL;
        y2h_free(d->d_region); d->d_region = NULL;
        y2h_free(d->d_flat); d->d_flat = NULL;
        y2h_free(d->d_halo); d->d_halo = NULL; d->halo_px = 0;
        y2h_free(d->d_bin); d->d_bin = NULL;
        y2h_free(d->d_state); d->d_state = NULL;
        y2h_free(d->d_proj); d->d_proj = NULL;
        y2h_free(d->d_hist); d->d_hist = NULL;
        y2h_free(d->d_zf); d->d_zf = NULL;
        y2h_free(d->d_tmp); d->d_tmp = NULL;
        d->placed_in = -1; d->alias_of = -1; d->copy_mask = 0;
        d->fused_pool = 0; d->fused_into = -1;
        d->out_half = 0;
        d->form = Y2_FORM_DIRECT;
        d->tile_bm = d->tile_bn = d->ksplit = 0;
        d->conn_ranges = 0;
    }
    y2_drop_graphs(e);
    y2h_free(e->d_in_nchw); e->d_in_nchw = NULL;
    y2h_free(e->d_in_nhwc); e->d_in_nhwc = NULL;
    y2h_free(e->d_out_nchw); e->d_out_nchw = NULL;
    y2h_free(e->d_ws); e->d_ws = NULL; e->ws_bytes = 0;
    y2h_free(e->d_u8); e->d_u8 = NULL; e->u8_cap = 0;
    y2h_free(e->d_planes); e->d_planes = NULL; e->planes_cap = 0;
    y2h_free(e->d_rtmp); e->d_rtmp = NULL; e->rtmp_cap = 0;
    if (e->reg_pending) { y2h_event_sync(e->ev_reg); e->reg_pending = 0; }
    y2h_free(e->d_reg); e->d_reg = NULL; e->reg_cap = 0;
    y2h_free(e->d_boxes); e->d_boxes = NULL;
    y2h_free(e->d_probs); e->d_probs = NULL;
    y2h_free(e->d_probs_nms); e->d_probs_nms = NULL;
    y2h_free(e->d_records); e->d_records = NULL;
    y2h_free(e->d_counts); e->d_counts = NULL;
    y2h_free(e->d_class_counts); e->d_class_counts = NULL;
    y2h_free(e->d_best); e->d_best = NULL;
    y2h_free(e->d_mean_ring); e->d_mean_ring = NULL; e->mean_els = 0; e->mean_index = 0;
    y2h_host_free(e->h_records); e->h_records = NULL;
    y2h_host_free(e->h_counts); e->h_counts = NULL;
    e->built = 0;
}

/* ------------------------------------------------------------------ */
/* what the forward pass reads the plan through                        */
/* ------------------------------------------------------------------ */
static int producer_can_place(const layer *l)
{
    return l->type == CONVOLUTIONAL || l->type == MAXPOOL || l->type == REORG;
}

/* device code of a reference ACTIVATION (activations.h:7) */
int y2_act_code(ACTIVATION a)
{
    switch (a) {
    case LINEAR: return Y2H_ACT_LINEAR;
    case LEAKY: return Y2H_ACT_LEAKY;
    case LOGISTIC: return Y2H_ACT_LOGISTIC;
    case RELU: return Y2H_ACT_RELU;
    case RELIE: return Y2H_ACT_RELIE;
    case RAMP: return Y2H_ACT_RAMP;
    case TANH: return Y2H_ACT_TANH;
    case PLSE: return Y2H_ACT_PLSE;
    case ELU: return Y2H_ACT_ELU;
    case LOGGY: return Y2H_ACT_LOGGY;
    case STAIR: return Y2H_ACT_STAIR;
    case HARDTAN: return Y2H_ACT_HARDTAN;
    case LHTAN: return Y2H_ACT_LHTAN;
    }
    return -1;
}
/* the four activations of the target cfgs are applied in the producing kernel's epilogue; the others run as the
 * reference runs every activation -- a pass of their own over the stored output (activations.c:95) */
int y2_act_in_kernel(ACTIVATION a) { const int c = y2_act_code(a); return c >= 0 && c <= Y2H_ACT_RELU; }
int y2_act_for_kernel(ACTIVATION a) { return y2_act_in_kernel(a) ? y2_act_code(a) : Y2H_ACT_LINEAR; }
/* the cfg name of an ACTIVATION (activations.c:8-38 get_activation_string) */
static const char *act_name(ACTIVATION a)
{
    static const char *const names[] = { "logistic", "relu", "relie", "linear", "ramp", "tanh", "plse", "leaky", "elu", "loggy",
                                         "stair", "hardtan", "lhtan" };
    return ((int)a >= 0 && (int)a < (int)(sizeof names / sizeof names[0])) ? names[a] : "relu";
}

/* what the input form means: the size of the engine's NHWC input buffer and layer 0's descriptor fields */
void y2_input_form(const network *net, y2_in_form *f)
{
    const y2_engine *e = y2_engine_of(net);
    const int px = e->in_halo_px;
    memset(f, 0, sizeof *f);
    f->ldx = net->c;
    switch (e->in_form) {
    case Y2_IN_NHWC: f->floats = e->in_floats; break;
    case Y2_IN_NHWC_HALO: f->floats = (size_t)net->batch * (net->h + 2 * px) * (net->w + 2 * px) * net->c; f->x_halo = px; break;
    case Y2_IN_NHWC4_HALO_F16:                 /* 4 halves = 2 floats per pixel */
        f->floats = (size_t)net->batch * (net->h + 2) * (net->w + 2) * 2; f->x_halo = px; f->x_f16 = 1; f->ldx = 4; break;
    case Y2_IN_NCHW: f->floats = 64; f->x_nchw = 1; break;      /* the buffer is not used */
    }
}

/* the only code that fills a y2h_conv from a layer */
void y2_conv_desc(const network *net, int i, y2h_conv *c, const float *x, int ldx)
{
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    const y2_engine *e = d->eng;
    y2_in_form in;
    y2_input_form(net, &in);
    memset(c, 0, sizeof *c);
    c->batch = l->batch; c->h = l->h; c->w = l->w; c->c = l->c; c->ldx = ldx;
    c->n = l->n; c->size = l->size; c->stride = l->stride; c->pad = l->pad;
    c->out_h = l->out_h; c->out_w = l->out_w; c->ldy = d->out_ld;
    c->batch_normalize = l->batch_normalize;
    c->activation = y2_act_for_kernel(l->activation);
    c->x = x;
    c->x_halo = (i == 0) ? in.x_halo : 0;
    if (i > 0 && ld_of(&net->layers[i - 1])->d_halo) c->x_halo = ld_of(&net->layers[i - 1])->halo_px;
    if (l->xnor) c->x_halo = 0;
    c->fuse_maxpool2 = d->fused_pool;
    c->ws = e->d_ws;
    c->ws_bytes = e->ws_bytes;
    c->y = d->out;
    c->y_f16 = d->out_half;
    c->x_f16 = (i > 0) ? ld_of(&net->layers[i - 1])->out_half : in.x_f16;
    c->x_nchw = (i == 0 && in.x_nchw);
    c->tile_bm = d->tile_bm; c->tile_bn = d->tile_bn; c->ksplit = d->ksplit;
    if (e->arena) {
        c->w_packed = (const float *)(e->arena + d->off_w_packed);
        c->w_ref = d->has_w_ref ? (const float *)(e->arena + d->off_w_ref) : NULL;
        c->bias = (const float *)(e->arena + d->off_bias);
        if (y2_half_weights(net, i)) {
            c->alpha = (const float *)(e->arena + d->off_alpha);
            c->beta = (const float *)(e->arena + d->off_beta);
        }
        if (l->batch_normalize) {
            c->mean = (const float *)(e->arena + d->off_mean);
            c->scale = (const float *)(e->arena + d->off_scale);
            c->rinv = (const double *)(e->arena + d->off_rinv);
        }
    }
}

/* the descriptor for a question to the dispatch (which kernel, how much scratch) asked while the plan is being built:
 * the arena may not exist yet, or be laid out for the previous plan */
static void conv_query(const network *net, int i, y2h_conv *c, const float *x, int ldx)
{
    y2_conv_desc(net, i, c, x, ldx);
    c->w_packed = Y2_ALIGNED_STANDIN;
}

/* a recurrent first layer behind a [net] with inputs= only reads the caller's rows as they are */
int y2_flat_input(const network *net)
{
    return net->n > 0 && is_recurrent(&net->layers[0]) && !(net->h && net->w && net->c);
}

void y2_input_view(const network *net, int i, const float **x, int *ldx)
{
    const y2_engine *e = y2_engine_of(net);
    if (i == 0 && y2_flat_input(net)) { *x = e->cur_input; *ldx = net->inputs; return; }
    if (i == 0) {
        y2_in_form in;
        y2_input_form(net, &in);
        *x = in.x_nchw ? e->cur_input : e->d_in_nhwc; *ldx = in.ldx;
    } else {
        const y2_ldev *p = ld_of(&net->layers[i - 1]);
        *x = p->out; *ldx = p->out_ld;
        /* (a half [crop] keeps the [h+2][w+2][4] form of the fp16 first-layer kernel there) */
        if (p->d_halo && net->layers[i].type == CONVOLUTIONAL) { *x = p->d_halo; *ldx = p->out_half ? 4 : net->layers[i - 1].out_c; }
    }
    /* an xnor convolution reads the binarized copy of its input */
    if (net->layers[i].type == CONVOLUTIONAL && net->layers[i].xnor && ld_of(&net->layers[i])->d_bin) {
        *x = ld_of(&net->layers[i])->d_bin; *ldx = net->layers[i].c;
    }
    /* a [connected] layer is run as a 1x1 convolution over a 1x1 image whose channels are the whole input vector */
    if (net->layers[i].type == CONNECTED) *ldx = net->layers[i].inputs;
}

/* the layer whose activations a layer reads, looking through the inference no-ops ([dropout], [cost]) */
int y2_producer_of(const network *net, int i)
{
    int p = i - 1;
    while (p > 0 && (net->layers[p].type == DROPOUT || net->layers[p].type == COST)) --p;
    return p;
}

/* 1: the layer's activations are a flat [batch][outputs] fp32 vector, not an NHWC image */
int y2_is_flat(const network *net, int i)
{
    switch (net->layers[i].type) {
    case REGION: case AVGPOOL: case SOFTMAX: case CONNECTED: case DETECTION: case RNN: case GRU: return 1;
    case DROPOUT: case COST: case ACTIVE: return i > 0 ? y2_is_flat(net, i - 1) : 0;   /* as the layer in front */
    default: return 0;
    }
}

/* 1: layer i holds half weights -- its input is half.  A [connected] layer looks through [dropout]; the convolution
 * behind a half [crop] that runs the fp16 first-layer kernel keeps fp32 [n][27] weights, as that kernel does at layer 0 */
int y2_half_weights(const network *net, int i)
{
    const y2_ldev *pd;
    if (i <= 0) return 0;
    pd = ld_of(&net->layers[net->layers[i].type == CONNECTED ? y2_producer_of(net, i) : i - 1]);
    if (!pd->out_half) return 0;
    return !(net->layers[i].type == CONVOLUTIONAL && pd->d_halo);
}

/* Y2_CONN_KSPLIT=n forces the K ranges of connected_f16 (tests; clamped by y2h_connected_f16_plan) */
static int conn_forced_ranges(void)
{
    const char *ks = getenv("Y2_CONN_KSPLIT");
    return (ks && atoi(ks) > 0) ? atoi(ks) : 0;
}

static int upload_small(void **dst, const void *src, size_t bytes, y2h_stream s)
{
    if (*dst) { y2h_free(*dst); *dst = NULL; }
    if (y2h_malloc(dst, bytes) != 0) return -1;
    if (y2h_memcpy_h2d(*dst, src, bytes, s) != 0) return -1;
    return y2h_stream_sync(s);
}

/* the split-K scratch shared by all conv layers only grows */
static int grow_workspace(y2_engine *e, size_t need)
{
    if (need <= e->ws_bytes) return 0;
    y2h_free(e->d_ws); e->d_ws = NULL; e->ws_bytes = 0;
    HIP_OR_ERR(y2h_malloc((void **)&e->d_ws, need));
    e->ws_bytes = need;
    return 0;
}

/* split-K scratch: the largest request of any conv layer under the current tile choices, and of the matrix-core forms
 * of the recurrent products */
static int plan_workspace(network *net)
{
    y2_engine *e = y2_engine_of(net);
    size_t need = y2_rec_workspace_bytes(net);
    int i;
    for (i = 0; i < net->n; ++i) {
        y2h_conv c;
        const y2_conv_form *f;
        const float *x; int ldx;
        size_t b;
        if ((net->layers[i].type != CONVOLUTIONAL && net->layers[i].type != CONNECTED) || e->strict) continue;
        if (ld_of(&net->layers[i])->conn_ranges) {         /* connected_f16: the raw sums of its K ranges */
            const layer *l = &net->layers[i];
            if (y2h_connected_f16_plan(l->batch, l->inputs, l->outputs, ld_of(l)->conn_ranges, NULL, &b, NULL, 0) == 0 && b > need) need = b;
            continue;
        }
        y2_input_view(net, i, &x, &ldx);
        conv_query(net, i, &c, x, ldx);
        f = &y2_conv_forms[ld_of(&net->layers[i])->form];
        b = f->workspace_bytes ? f->workspace_bytes(&c) : 0;
        if (b > need) need = b;
    }
    return grow_workspace(e, need);
}

/* ------------------------------------------------------------------ */
/* tile autotuning (y2_set_autotune)                                   */
/* ------------------------------------------------------------------ */
/* Measured choices are remembered per layer shape for the life of the process, so that re-plans (set_batch_network,
 * resize_network back and forth, several networks of one family) do not measure again. */
typedef struct { int batch, h, w, c, n, size, stride, pool, bm, bn, ks; } tune_entry;
static tune_entry g_tuned[256];
static int g_ntuned = 0;
static pthread_mutex_t g_tuned_mu = PTHREAD_MUTEX_INITIALIZER;    /* networks / Detectors may be built from several threads */

/* the layers autotuning looks at: the direct matrix-core convolutions (a Winograd layer has no direct tile to measure) */
static int has_tile_to_measure(const layer *l)
{
    return l->type == CONVOLUTIONAL && ld_of(l)->uses_mfma && !l->xnor && ld_of(l)->form == Y2_FORM_DIRECT;
}

/* Candidates are timed INSIDE whole forward passes (per-layer HIP events, as y2_layer_times_ms reads them): timed in
 * isolation, back to back, a layer finds its own weights in the Infinity Cache and small tiles look better than they are
 * in the real sequence, where the 204 MB of yolo.cfg weights stream from HBM once per forward. */
static int autotune_layers(network *net)
{
    y2_engine *e = y2_engine_of(net);
    const int keep_timing = e->timing;
    int i, k, a;
    size_t need = 0;
    for (i = 0; i < net->n; ++i) {          /* scratch for the largest K-split any candidate may ask for */
        const layer *l = &net->layers[i];
        y2h_conv c;
        const float *x; int ldx, n, bm[64], bn[64], ks[64];
        if (!has_tile_to_measure(l)) continue;
        y2_input_view(net, i, &x, &ldx);
        y2_conv_desc(net, i, &c, x, ldx);
        n = y2h_conv_candidates(&c, bm, bn, ks, 64);
        for (a = 0; a < n; ++a) {
            size_t b = (size_t)ks[a] * l->batch * l->out_h * l->out_w * l->out_c * sizeof(float);
            if (ks[a] > 1 && b > need) need = b;
        }
    }
    if (grow_workspace(e, need) != 0) return -1;
    if (y2h_memset(e->d_in_nchw, 0, e->in_floats * sizeof(float), e->stream) != 0) { y2_fail("autotune: %s", y2h_last_error()); return -1; }
    e->timing = 1;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        y2h_conv c;
        const float *x; int ldx, n, hit = 0, bm[64], bn[64], ks[64], best = 0;
        float best_ms = 0.f;
        if (!has_tile_to_measure(l)) continue;
        y2_input_view(net, i, &x, &ldx);
        y2_conv_desc(net, i, &c, x, ldx);
        pthread_mutex_lock(&g_tuned_mu);
        for (k = 0; k < g_ntuned && !hit; ++k) {
            const tune_entry *t = &g_tuned[k];
            if (t->batch == c.batch && t->h == c.h && t->w == c.w && t->c == c.c && t->n == c.n && t->size == c.size &&
                t->stride == c.stride && t->pool == c.fuse_maxpool2) { d->tile_bm = t->bm; d->tile_bn = t->bn; d->ksplit = t->ks; hit = 1; }
        }
        pthread_mutex_unlock(&g_tuned_mu);
        /* big grids (hundreds of tiles per CU round) are where the cost model is reliable and a measurement costly */
        if (!hit && 2.0 * l->batch * l->out_h * l->out_w * (double)l->n * l->size * l->size * l->c > 40e9) continue;
        if (!hit) {
            c.tile_bm = c.tile_bn = c.ksplit = 0;
            n = y2h_conv_candidates(&c, bm, bn, ks, 64);
            if (n < 0) { e->timing = keep_timing; y2_fail("autotune of layer %d failed (%d): %s", i, n, y2h_last_error()); return -1; }
            if (n == 0) continue;
            for (a = 0; a < n; ++a) {
                float ms = 0.f, m2 = 0.f;
                int rep;
                d->tile_bm = bm[a]; d->tile_bn = bn[a]; d->ksplit = ks[a];
                for (rep = 0; rep < 2; ++rep) {            /* the first pass also sets the kernel's LDS attribute */
                    if (y2_enqueue_forward(net, e->d_in_nchw) != 0) { e->timing = keep_timing; return -1; }
                    if (y2h_event_elapsed_ms(e->ev[i], e->ev[i + 1], &m2) != 0) { e->timing = keep_timing; y2_fail("autotune: %s", y2h_last_error()); return -1; }
                    ms = (rep == 0 || m2 < ms) ? m2 : ms;
                }
                if (getenv("Y2_AUTOTUNE_LOG"))
                    fprintf(stderr, "autotune layer %2d %3dx%-3d c%-4d n%-5d k%d%s: %3dx%-3d ks%-2d %.4f ms%s\n", i, l->h, l->w, l->c, l->n, l->size,
                            c.fuse_maxpool2 ? "+pool" : "", bm[a], bn[a], ks[a], ms, a == 0 ? "  (model)" : "");
                if (a == 0) ms *= 0.98f;                     /* the model's choice stays unless another wins by 2 % */
                if (a == 0 || ms < best_ms) { best_ms = ms; best = a; }
            }
            d->tile_bm = bm[best]; d->tile_bn = bn[best]; d->ksplit = ks[best];
            pthread_mutex_lock(&g_tuned_mu);
            if (g_ntuned < (int)(sizeof g_tuned / sizeof g_tuned[0])) {
                tune_entry *t = &g_tuned[g_ntuned++];
                t->batch = c.batch; t->h = c.h; t->w = c.w; t->c = c.c; t->n = c.n; t->size = c.size; t->stride = c.stride;
                t->pool = c.fuse_maxpool2; t->bm = d->tile_bm; t->bn = d->tile_bn; t->ks = d->ksplit;
            }
            pthread_mutex_unlock(&g_tuned_mu);
        }
        y2_conv_desc(net, i, &c, x, ldx);
        d->kernel = y2h_conv_variant(&c, 0);
        if (d->fused_pool) { snprintf(d->kname, sizeof d->kname, "%s+maxpool2", d->kernel); d->kernel = d->kname; }
    }
    e->timing = keep_timing;
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* A replica (y2_weights_arena on a rank that never loads weights) is planned while its arena is still uninitialised HBM:
 * timing candidates on garbage / NaN data would let every rank keep a different K-split, and ranks that are supposed to be
 * bit-identical replicas would differ in the last bits.  Such a build keeps the cost model's choices; the measurement runs
 * at the first build AFTER the arena became resident (y2_weights_resident drops the plan when autotuning is on). */
static int autotune_allowed(const y2_engine *e) { return e->autotune && !e->strict && !e->arena_pending; }

/* ------------------------------------------------------------------ */
/* the passes, in the order y2_engine_build runs them                  */
/* ------------------------------------------------------------------ */
/* [softmax] tree=: the tree must cover the layer's rows exactly.  softmax_tree (softmax_layer.c:35-47) walks the tree's
 * groups whatever inputs/groups is: a larger tree writes past the row, a smaller one leaves outputs unwritten.  Needs no
 * device, and is the first thing a plan asks. */
int y2_softmax_tree_check(const network *net)
{
    int i, g, j, count;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const tree *t = l->softmax_tree;
        if (l->type != SOFTMAX || !t) continue;
        if (l->groups <= 0 || t->n != l->inputs / l->groups) {
            y2_fail("softmax layer %d: tree has %d nodes but the layer's rows have inputs/groups = %d (the reference would read or "
                    "write out of bounds, softmax_layer.c:41-45)", i, t->n, l->groups > 0 ? l->inputs / l->groups : 0);
            return -1;
        }
        for (g = 0, count = 0; g < t->groups; ++g) {
            if (t->group_size[g] < 0 || t->group_offset[g] != count) { y2_fail("softmax layer %d: tree group %d is not contiguous", i, g); return -1; }
            count += t->group_size[g];
        }
        if (count != t->n) { y2_fail("softmax layer %d: the tree's groups hold %d of its %d nodes", i, count, t->n); return -1; }
        for (j = 0; j < t->n; ++j)
            if (t->parent[j] >= t->n || t->group[j] < 0 || t->group[j] >= t->groups) {
                y2_fail("softmax layer %d: tree node %d has parent %d, group %d (of %d nodes, %d groups)", i, j, t->parent[j], t->group[j], t->n, t->groups);
                return -1;
            }
    }
    return 0;
}

static int plan_checks(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) { y2_fail("network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (y2_softmax_tree_check(net) != 0) return -1;
    if (net->gpu_index < 0) {
        y2_fail("gpu_index %d: this library has no CPU compute path; select a GPU (>= 0)", net->gpu_index);
        return -1;
    }
    if (y2h_device_count() <= 0) { y2_fail("no HIP device visible: the MI355X engine cannot run"); return -1; }
    e->device = net->gpu_index;
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!e->stream) HIP_OR_ERR(y2h_stream_create(&e->stream));
    return 0;
}

/* every layer follows the network batch (set_batch_network only rewrites the field); a recurrent layer runs
 * net.batch / steps sequences (rnn_layer.c:32) */
static int plan_batches(network *net)
{
    int i;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        l->batch = net->batch;
        if (!is_recurrent(l)) continue;
        if (l->steps <= 0 || net->batch % l->steps) {
            y2_fail("layer %d (%s): batch %d is not a multiple of time_steps %d", i, get_layer_string(l->type), net->batch, l->steps);
            return -1;
        }
        l->batch = net->batch / l->steps;
    }
    return 0;
}

/* let the sources of concatenating routes write into the route buffer */
static int plan_routes(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i, k;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        if (l->type == ROUTE && l->n == 1) d->alias_of = l->input_layers[0];
        if (l->type == COST) d->alias_of = i - 1;
        if (l->type != ROUTE || l->n < 2) continue;
        if (l->n > 32) { y2_fail("route layer %d has %d inputs (max 32)", i, l->n); return -1; }
        if (!l->out_c) { y2_fail("route layer %d concatenates layers of different spatial size", i); return -1; }
        for (k = 0; k < l->n; ++k) {
            layer *src = &net->layers[l->input_layers[k]];
            y2_ldev *sd = ld_of(src);
            int dup = 0, m;
            for (m = 0; m < k; ++m) if (l->input_layers[m] == l->input_layers[k]) dup = 1;
            if (!dup && producer_can_place(src) && sd->placed_in < 0 && l->input_layers[k] != e->out_layer)
                sd->placed_in = i;
            else
                d->copy_mask |= 1u << k;
        }
    }
    return 0;
}

/* conv -> 2x2/2 maxpool pairs whose full-resolution activation nobody else reads are fused:
 * the conv kernel pools in its epilogue and writes straight into the maxpool layer's buffer */
static int plan_pool_fusion(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i, k;
    if (!e->fusion || e->strict) return 0;
    for (i = 0; i + 1 < net->n; ++i) {
        layer *l = &net->layers[i], *m = &net->layers[i + 1];
        int used = 0, j;
        if (l->type != CONVOLUTIONAL || m->type != MAXPOOL) continue;
        if (m->size != 2 || m->stride != 2 || m->pad != 0 || (l->out_h & 1) || (l->out_w & 1)) continue;
        if (l->stride != 1 || l->pad != l->size / 2 || !(l->size == 1 || l->size == 3)) continue;
        if (!y2_act_in_kernel(l->activation)) continue;       /* the separate activation pass must see every pixel */
        if (!((l->c % 16 == 0) || (i == 0 && l->c == 3 && l->size == 3 && l->n <= 64))) continue;
        if (i == e->out_layer || ld_of(l)->placed_in >= 0) continue;
        for (j = 0; j < net->n; ++j) {
            if (net->layers[j].type == ROUTE)
                for (k = 0; k < net->layers[j].n; ++k) if (net->layers[j].input_layers[k] == i) used = 1;
            if (net->layers[j].type == SHORTCUT && net->layers[j].index == i) used = 1;
        }
        if (used) continue;
        ld_of(l)->fused_pool = 1;
        ld_of(m)->fused_into = i;
    }
    return 0;
}

/* fp16 storage (y2_set_half): image-like activations are half, heads stay fp32 */
static int plan_half(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i, k;
    if (!e->half || e->strict) return 0;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l), *pd = i > 0 ? ld_of(&net->layers[i - 1]) : NULL;
        switch (l->type) {
        case CONVOLUTIONAL:
            if (l->xnor) { y2_fail("fp16 mode: layer %d: xnor convolutions have no half-precision form", i); return -1; }
            if (!y2_act_in_kernel(l->activation)) { y2_fail("fp16 mode: layer %d: activation %d has no half-precision form", i, (int)l->activation); return -1; }
            /* the conv feeding a region head writes fp32: the head's logistic/softmax/exp run in fp32 */
            d->out_half = !(i + 1 < net->n && net->layers[i + 1].type == REGION);
            break;
        case MAXPOOL: case REORG:
            if (!pd || !pd->out_half) { y2_fail("fp16 mode: layer %d (%s) needs a half-precision producer", i, get_layer_string(l->type)); return -1; }
            d->out_half = 1;
            break;
        case ROUTE:
            if (l->n == 1) d->out_half = ld_of(&net->layers[l->input_layers[0]])->out_half;
            else {
                for (k = 0; k < l->n; ++k)
                    if (!ld_of(&net->layers[l->input_layers[k]])->out_half) { y2_fail("fp16 mode: route layer %d mixes fp32 and half inputs", i); return -1; }
                d->out_half = 1;
            }
            break;
        case REGION: case SOFTMAX: case DETECTION:
            if (pd && pd->out_half) { y2_fail("fp16 mode: layer %d (%s) needs an fp32 producer (a convolutional or avgpool layer)", i, get_layer_string(l->type)); return -1; }
            break;
        case CONNECTED: {
            /* reads a half image or a half flat vector; like the conv in front of [region], the last dense layer of a
             * head writes fp32: a dense layer stores half only for another dense layer */
            const int pi = y2_producer_of(net, i);
            int nx = i + 1;
            if (i == 0) { y2_fail("layer %d (%s) cannot be the first layer", i, get_layer_string(l->type)); return -1; }
            if (!y2_act_in_kernel(l->activation)) { y2_fail("fp16 mode: layer %d (connected): activation %d has no half-precision form", i, (int)l->activation); return -1; }
            if (!ld_of(&net->layers[pi])->out_half) {
                y2_fail("fp16 mode: layer %d (connected) needs a half-precision producer, layer %d (%s) stores fp32", i, pi, get_layer_string(net->layers[pi].type));
                return -1;
            }
            while (nx < net->n && (net->layers[nx].type == DROPOUT || net->layers[nx].type == COST)) ++nx;
            d->out_half = nx < net->n && net->layers[nx].type == CONNECTED;
        } break;
        case LOCAL:
            if (!pd || !pd->out_half || y2_is_flat(net, i - 1)) { y2_fail("fp16 mode: layer %d (local) needs a half-precision image producer", i); return -1; }
            if (!y2_act_in_kernel(l->activation)) { y2_fail("fp16 mode: layer %d (local): activation %d has no half-precision form", i, (int)l->activation); return -1; }
            d->out_half = 1;
            break;
        case CROP:
            /* reads the fp32 network input and writes half */
            if (i != 0) { y2_fail("fp16 mode: layer %d (crop) has a half-precision form only as the first layer", i); return -1; }
            d->out_half = 1;
            break;
        case DROPOUT: d->out_half = pd ? pd->out_half : 0; break;
        case NORMALIZATION: case ACTIVE:
            if (!pd || !pd->out_half) { y2_fail("fp16 mode: layer %d (%s) needs a half-precision producer", i, get_layer_string(l->type)); return -1; }
            if (l->type == ACTIVE && !y2_act_in_kernel(l->activation)) { y2_fail("fp16 mode: layer %d: activation %d has no half-precision form", i, (int)l->activation); return -1; }
            if (l->type == NORMALIZATION && !y2h_lrn_fast_ok(l->c, l->size)) { y2_fail("fp16 mode: layer %d: a normalization over %d channels has no half-precision form", i, l->c); return -1; }
            d->out_half = 1;
            break;
        case COST: d->out_half = pd ? pd->out_half : 0; break;
        case SHORTCUT: case BATCHNORM: case RNN: case GRU:
            y2_fail("fp16 mode: layer %d (%s) has no half-precision kernel", i, get_layer_string(l->type)); return -1;
        default: break;
        }
    }
    if (net->n > 0 && net->layers[0].type != CONVOLUTIONAL && net->layers[0].type != CROP) { y2_fail("fp16 mode: the first layer must be convolutional or crop"); return -1; }
    return 0;
}

/* give this layer an activation buffer of its own: NHWC, fp32 or half */
static int alloc_activations(y2_ldev *d, const layer *l)
{
    d->out_floats = (size_t)l->batch * l->out_h * l->out_w * l->out_c;
    HIP_OR_ERR(y2h_malloc((void **)&d->out_alloc, d->out_floats * (d->out_half ? 2 : 4)));
    d->out = d->out_alloc;
    d->out_ld = l->out_c;
    return 0;
}

/* a flat [batch][outputs] vector: fp32, or half for a dense layer that feeds another one in fp16 mode */
static int alloc_flat(y2_ldev *d, const layer *l)
{
    HIP_OR_ERR(y2h_malloc((void **)&d->d_flat, (size_t)l->batch * l->outputs * (d->out_half ? 2 : sizeof(float))));
    d->out = d->d_flat; d->out_ld = l->outputs;
    return 0;
}

static void alias_output(y2_ldev *d, const y2_ldev *sd, const char *kernel)
{
    d->out = sd->out; d->out_ld = sd->out_ld; d->kernel = kernel;
}

/* allocate.  Routes first (their sources point into them). */
static int plan_activations(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i, k;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type == ROUTE && l->n >= 2 && alloc_activations(ld_of(l), l) != 0) return -1;
    }
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        switch (l->type) {
        case CONVOLUTIONAL: case MAXPOOL: case REORG:
            d->kernel = l->type == MAXPOOL ? "maxpool_nhwc" : (l->type == REORG ? "reorg_nhwc" : "conv");
            if (d->fused_pool) break;            /* writes into the maxpool layer's buffer (set below) */
            if (d->placed_in >= 0) {
                layer *r = &net->layers[d->placed_in];
                y2_ldev *rd = ld_of(r);
                int choff = 0;
                for (k = 0; k < r->n && r->input_layers[k] != i; ++k) choff += net->layers[r->input_layers[k]].out_c;
                d->out = d->out_half ? (float *)((unsigned short *)rd->out + choff) : rd->out + choff;
                d->out_ld = r->out_c;
            } else if (alloc_activations(d, l) != 0) return -1;
            break;
        case SHORTCUT: case CROP: case LOCAL: case BATCHNORM:
            if (alloc_activations(d, l) != 0) return -1;
            d->kernel = l->type == SHORTCUT ? "shortcut" : l->type == CROP ? (d->out_half ? "crop_f16" : "crop") :
                        l->type == LOCAL ? (d->out_half ? "local_f16" : e->strict ? "local_ref" : "local") : "batchnorm";
            break;
        case NORMALIZATION:
            if (alloc_activations(d, l) != 0) return -1;
            /* a row too wide for a workgroup's tile runs the reference-order kernel in every mode */
            d->kernel = d->out_half ? "lrn_nhwc_f16" : (e->strict || !y2h_lrn_fast_ok(l->c, l->size)) ? "lrn_ref" : "lrn_nhwc";
            break;
        case ACTIVE:
            if (y2_act_code(l->activation) < 0) { y2_fail("activation layer %d: unknown activation %d", i, (int)l->activation); return -1; }
            if ((y2_is_flat(net, i) ? alloc_flat(d, l) : alloc_activations(d, l)) != 0) return -1;
            snprintf(d->kname, sizeof d->kname, d->out_half ? "activation_f16(%s)" : "activation(%s)", act_name(l->activation));
            d->kernel = d->kname;
            break;
        case ROUTE:
            d->kernel = "route(zero-copy)";
            if (l->n == 1) alias_output(d, ld_of(&net->layers[d->alias_of]), d->kernel);
            else if (d->copy_mask) d->kernel = "route(copy_channels)";
            break;
        case COST:
            alias_output(d, ld_of(&net->layers[i - 1]), "none");
            break;
        case REGION:
            HIP_OR_ERR(y2h_malloc((void **)&d->d_region, (size_t)l->batch * l->outputs * sizeof(float)));
            d->out = d->d_region; d->out_ld = l->outputs / (l->h * l->w);
            d->kernel = l->softmax_tree ? "region+tree_softmax" : "region";
            break;
        case AVGPOOL: case SOFTMAX:
            if (alloc_flat(d, l) != 0) return -1;
            d->kernel = l->type == AVGPOOL ? "avgpool" : (l->softmax_tree ? "softmax_tree" : "softmax_rows");
            break;
        case CONNECTED: case DETECTION: {
            /* YOLOv1 family: flat fp32 vectors.  The producer of a dense layer must be contiguous (an image
             * producer is read as [y][x][c] with re-ordered weights, see y2_arena.c pack_filters) */
            const int pi = y2_producer_of(net, i);
            const y2_ldev *pd = i > 0 ? ld_of(&net->layers[pi]) : NULL;
            if (i == 0) { y2_fail("layer %d (%s) cannot be the first layer", i, get_layer_string(l->type)); return -1; }
            if (!y2_is_flat(net, pi) && (pd->out_ld != net->layers[pi].out_c || pd->fused_pool)) {
                y2_fail("layer %d (%s): its input (layer %d) is not stored contiguously", i, get_layer_string(l->type), pi);
                return -1;
            }
            if (l->type == DETECTION && !y2_is_flat(net, pi)) { y2_fail("detection layer %d must follow a flat layer ([connected])", i); return -1; }
            if (alloc_flat(d, l) != 0) return -1;
            d->kernel = l->type == DETECTION ? (l->softmax ? "detection(copy+softmax)" : "detection(copy)") : "connected";
        } break;
        case RNN: case GRU:
            if (y2_rec_plan(net, i) != 0) return -1;
            break;
        case DROPOUT:
            if (i == 0) { y2_fail("dropout layer %d has no input layer", i); return -1; }
            d->alias_of = i - 1;
            alias_output(d, ld_of(&net->layers[i - 1]), "none (inference)");
            break;
        default:
            y2_fail("layer %d: type %d has no device implementation", i, (int)l->type);
            return -1;
        }
    }
    for (i = 0; i + 1 < net->n; ++i) {
        y2_ldev *d = ld_of(&net->layers[i]), *md = ld_of(&net->layers[i + 1]);
        if (!d->fused_pool) continue;
        alias_output(d, md, d->kernel);
        md->kernel = "(fused into the conv before)";
    }
    return 0;
}

/* the second copies some convolutions read.  A [crop] in front of a few-channel convolution (vgg-16.cfg, strided.cfg,
 * yolov1/yolo-small.cfg) also writes its window with the zero border the first-layer / stem kernels want;
 * xnor=1 convolutions (convolutional_layer.c:443-447) read a +-1 copy of their input */
static int plan_input_copies(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    for (i = 0; i + 1 < net->n && !e->strict && !e->half; ++i) {
        const layer *l = &net->layers[i], *nl = &net->layers[i + 1];
        y2_ldev *d = ld_of(l);
        y2h_conv c0;
        size_t fl;
        int px;
        if (l->type != CROP || nl->type != CONVOLUTIONAL || nl->c > 4 || ld_of(nl)->fused_pool || nl->xnor) continue;
        conv_query(net, i + 1, &c0, NULL, nl->c);
        px = y2h_conv_first_layer_ok(&c0) ? 1 : y2h_conv_stem_halo(&c0);
        if (px <= 0) continue;
        fl = (size_t)l->batch * (l->out_h + 2 * px) * (l->out_w + 2 * px) * l->out_c;
        HIP_OR_ERR(y2h_malloc((void **)&d->d_halo, fl * sizeof(float)));
        HIP_OR_ERR(y2h_memset(d->d_halo, 0, fl * sizeof(float), e->stream));
        d->halo_px = px;
    }
    /* fp16 mode: the half counterpart for a first-layer [crop] -- the [b][h+2][w+2][4] form with a zero halo that the fp16
     * first-layer kernel reads (vgg-16.cfg, yolov1/yolo-small.cfg) */
    if (net->n > 1 && !e->strict && net->layers[0].type == CROP && ld_of(&net->layers[0])->out_half) {
        const layer *l = &net->layers[0], *nl = &net->layers[1];
        y2_ldev *d = ld_of(l);
        y2h_conv c0;
        if (nl->type == CONVOLUTIONAL && nl->c <= 4 && !ld_of(nl)->fused_pool) {
            conv_query(net, 1, &c0, NULL, nl->c);
            if (y2h_conv_first_layer_f16_ok(&c0)) {
                const size_t bytes = (size_t)l->batch * (l->out_h + 2) * (l->out_w + 2) * 4 * 2;
                HIP_OR_ERR(y2h_malloc((void **)&d->d_halo, bytes));
                HIP_OR_ERR(y2h_memset(d->d_halo, 0, bytes, e->stream));
                d->halo_px = 1;
            }
        }
    }
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type == CONVOLUTIONAL && l->xnor)
            HIP_OR_ERR(y2h_malloc((void **)&ld_of(l)->d_bin, (size_t)l->batch * l->h * l->w * l->c * sizeof(float)));
    }
    return 0;
}

/* how the network input reaches layer 0 (Y2_IN_*), asked of the dispatch with layer 0's own descriptor */
static int choose_input_form(const network *net, int *halo_px)
{
    const y2_engine *e = y2_engine_of(net);
    const layer *l0 = &net->layers[0];
    const int half = e->half && ld_of(l0)->out_half;
    y2h_conv c0;
    int form;
    *halo_px = 1;
    if (e->strict || l0->type != CONVOLUTIONAL || l0->xnor) return Y2_IN_NHWC;
    /* a 3-channel 3x3 first layer reads its input with a one-pixel zero halo (no tap bounds tests) */
    conv_query(net, 0, &c0, NULL, net->c);
    form = y2h_conv_first_layer_ok(&c0) ? Y2_IN_NHWC_HALO : Y2_IN_NHWC;
    if (form == Y2_IN_NHWC && !half) {
        /* other few-channel stems (7x7/2, 11x11/4, ...): the stem kernel reads a halo as wide as the padding */
        const int px = y2h_conv_stem_halo(&c0);
        if (px > 0) { form = Y2_IN_NHWC_HALO; *halo_px = px; }
    }
    /* fp16 mode: the first layer reads a half [b][h+2][w+2][4] copy of the input on the fp16 matrix cores */
    if (half && net->c <= 4 && y2h_conv_first_layer_f16_ok(&c0)) form = Y2_IN_NHWC4_HALO_F16;
    /* ... or, where the shape allows, reads the fp32 planes of the network input directly: no transform kernel */
    if ((form == Y2_IN_NHWC4_HALO_F16 || (form == Y2_IN_NHWC_HALO && *halo_px == 1 && y2h_conv_first_layer_ok(&c0))) &&
        y2h_conv_first_layer_nchw_ok(&c0)) form = Y2_IN_NCHW;
    return form;
}

/* the input form and the engine's two input buffers */
static int plan_input(network *net)
{
    y2_engine *e = y2_engine_of(net);
    y2_in_form in;
    e->in_floats = (size_t)net->batch * net->inputs;
    e->in_form = Y2_IN_NHWC;                      /* layer 0's descriptor is asked about the plain form */
    if (net->n > 0) e->in_form = choose_input_form(net, &e->in_halo_px);
    y2_input_form(net, &in);
    HIP_OR_ERR(y2h_malloc((void **)&e->d_in_nchw, e->in_floats * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_in_nhwc, in.floats * sizeof(float)));
    HIP_OR_ERR(y2h_memset(e->d_in_nhwc, 0, in.floats * sizeof(float), e->stream));     /* the halo stays zero */
    return 0;
}

/* the host and device output buffers, and for a detection head the decode / NMS buffers */
static int plan_output(network *net)
{
    y2_engine *e = y2_engine_of(net);
    layer *ol = &net->layers[e->out_layer];
    e->out_floats = (size_t)net->batch * ol->outputs;
    y2_engine_host_output(net);
    if (!e->h_out) { y2_fail("out of host memory for the network output"); return -1; }
    if (e->out_floats > e->h_out_stage_cap) {
        y2h_host_free(e->h_out_stage); e->h_out_stage = NULL; e->h_out_stage_cap = 0;
        HIP_OR_ERR(y2h_host_alloc((void **)&e->h_out_stage, e->out_floats * sizeof(float)));
        e->h_out_stage_cap = e->out_floats;
    }
    HIP_OR_ERR(y2h_malloc((void **)&e->d_out_nchw, e->out_floats * sizeof(float)));
    if (ol->type != REGION && ol->type != DETECTION) return 0;
    e->det_total = ol->w * ol->h * ol->n;         /* a [detection] layer has w = h = side */
    e->det_classes = ol->classes;
    e->det_batch = net->batch;
    e->det_cap = e->det_total;
    HIP_OR_ERR(y2h_malloc((void **)&e->d_boxes, (size_t)net->batch * e->det_total * 4 * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_probs, (size_t)net->batch * e->det_total * ol->classes * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_probs_nms, (size_t)net->batch * e->det_total * ol->classes * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_records, (size_t)net->batch * e->det_cap * 6 * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_counts, (size_t)net->batch * sizeof(int)));
    HIP_OR_ERR(y2h_malloc((void **)&e->d_class_counts, (size_t)net->batch * ol->classes * sizeof(int)));
    e->class_counts_zeroed = 0;
    HIP_OR_ERR(y2h_malloc((void **)&e->d_best, (size_t)2 * net->batch * e->det_total * sizeof(float)));
    HIP_OR_ERR(y2h_host_alloc((void **)&e->h_records, (size_t)net->batch * e->det_cap * 6 * sizeof(float)));
    HIP_OR_ERR(y2h_host_alloc((void **)&e->h_counts, (size_t)net->batch * sizeof(int)));
    return 0;
}

/* The tree tables of a [region] / [softmax] tree= head, in ONE block of ints:
 *   parent[n] | group_size[groups] | group_offset[groups] | group[n] | order[n] | level_off[levels + 1]
 * (order / level_off: the nodes by depth level for the level-parallel hierarchy walk, only when every parent precedes its
 * child; tree_levels = 0 otherwise).  Every plan derives them again from the layer's tree; they depend on the tree alone,
 * so they go up -- one copy, one wait -- only when they differ from what the device already holds: a re-plan after
 * resize_network / set_batch_network costs a tree head no copy and no wait. */
static int plan_tree_tables(y2_engine *e, y2_ldev *d, const layer *l)
{
    const tree *t = l->softmax_tree;
    const int n = t->n, g = t->groups;
    int *depth = calloc(n > 0 ? n : 1, sizeof(int)), *blk = NULL, *order, *loff, j, ok = 1, maxd = 0, lv, pos = 0, rc = -1;
    size_t ints;
    for (j = 0; j < n && ok; ++j) {
        int par = t->parent[j];
        if (par >= j) ok = 0;
        else depth[j] = par < 0 ? 0 : depth[par] + 1;
        if (ok && depth[j] > maxd) maxd = depth[j];
    }
    ints = (size_t)2 * n + 2 * g + (ok ? (size_t)n + maxd + 2 : 0);
    blk = calloc(ints ? ints : 1, sizeof(int));
    if (!depth || !blk) { y2_fail("out of memory"); goto cleanup; }
    memcpy(blk, t->parent, n * sizeof(int));
    memcpy(blk + n, t->group_size, g * sizeof(int));
    memcpy(blk + n + g, t->group_offset, g * sizeof(int));
    memcpy(blk + n + 2 * g, t->group, n * sizeof(int));
    order = blk + 2 * n + 2 * g; loff = order + n;
    if (ok) {
        for (lv = 0; lv <= maxd; ++lv) {
            loff[lv] = pos;
            for (j = 0; j < n; ++j) if (depth[j] == lv) order[pos++] = j;
        }
        loff[maxd + 1] = pos;
    }
    if (!d->d_tree_block || d->tree_block_ints != ints || memcmp(d->h_tree_block, blk, ints * sizeof(int)) != 0) {
        free(d->h_tree_block); d->h_tree_block = blk; blk = NULL; d->tree_block_ints = ints;
        if (upload_small((void **)&d->d_tree_block, d->h_tree_block, ints * sizeof(int), e->stream)) {
            y2h_free(d->d_tree_block); d->d_tree_block = NULL;
            y2_fail("tree upload: %s", y2h_last_error());
            goto cleanup;
        }
    }
    d->d_tree_parent = d->d_tree_block;
    d->d_tree_gsize = d->d_tree_block + n;
    d->d_tree_goff = d->d_tree_block + n + g;
    d->d_tree_group = d->d_tree_block + n + 2 * g;
    d->d_tree_order = ok ? d->d_tree_block + 2 * n + 2 * g : NULL;
    d->d_tree_loff = ok ? d->d_tree_order + n : NULL;
    d->tree_levels = ok ? maxd + 1 : 0;
    /* detect mode's (score, class) per box as a by-product of the region layer (y2h_region_forward_tree) */
    y2h_free(d->d_tree_best); d->d_tree_best = NULL;
    if (ok && l->type == REGION && !l->map && l->coords == 4 && y2h_region_tree_best_ok(l->classes, d->tree_levels) &&
        y2h_malloc((void **)&d->d_tree_best, (size_t)2 * l->batch * l->h * l->w * l->n * sizeof(float))) {
        y2_fail("tree scratch: %s", y2h_last_error());
        goto cleanup;
    }
    rc = 0;
cleanup:
    free(depth); free(blk);
    return rc;
}

/* the constants of the heads: a region layer's anchors and class map, and the tree tables of a [region] or [softmax] tree= */
static int plan_head_constants(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        tree *t = l->softmax_tree;
        if (l->type != REGION && !(l->type == SOFTMAX && t)) continue;
        if (l->type == REGION && upload_small((void **)&d->d_anchors, l->biases, 2 * l->n * sizeof(float), e->stream)) { y2_fail("anchor upload: %s", y2h_last_error()); return -1; }
        if (t && plan_tree_tables(e, d, l) != 0) return -1;
        if (l->map && upload_small((void **)&d->d_map, l->map, 200 * sizeof(int), e->stream)) { y2_fail("map upload: %s", y2h_last_error()); return -1; }
    }
    return 0;
}

/* decide per conv whether it runs on the matrix cores (the arena is laid out after that: a layer off them keeps a
 * reference-layout copy of its weights), and name its kernel */
static int plan_conv_kernels(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        y2h_conv c;
        const float *x; int ldx;
        if (l->type != CONVOLUTIONAL && l->type != CONNECTED) continue;
        if (y2_act_code(l->activation) < 0) { y2_fail("layer %d: unknown activation %d", i, (int)l->activation); return -1; }
        y2_input_view(net, i, &x, &ldx);
        conv_query(net, i, &c, x, ldx);
        if (l->type == CONNECTED && y2_half_weights(net, i)) {
            /* fp16 mode.  Up to 16 rows: connected_f16.  More: the fp16 matrix-core conv tile on a 1x1 image where its own
             * query takes the descriptor, else connected_f16 in passes of 16.  Y2_CONN_F16=skinny|mfma forces the form
             * where both are possible.  One half copy of the weights either way, no reference-layout copy. */
            const char *form = getenv("Y2_CONN_F16");
            const int tile_ok = y2h_conv_uses_mfma(&c) && strncmp(y2h_conv_variant(&c, 0), "conv_mfma_f16", 13) == 0;
            int tile = tile_ok && l->batch > 16;
            if (form && strcmp(form, "skinny") == 0) tile = 0;
            if (form && strcmp(form, "mfma") == 0) tile = tile_ok;
            d->uses_mfma = tile;
            d->has_w_ref = 0;
            if (tile) { d->kernel = y2h_conv_variant(&c, 0); continue; }
            if (y2h_connected_f16_plan(l->batch, l->inputs, l->outputs, conn_forced_ranges(), &d->conn_ranges, NULL, NULL, 0) != 0) {
                y2_fail("fp16 mode: layer %d (connected): %d inputs x %d outputs cannot be planned", i, l->inputs, l->outputs);
                return -1;
            }
            snprintf(d->kname, sizeof d->kname, d->conn_ranges > 1 ? "connected_f16+ksplit%d" : "connected_f16", d->conn_ranges);
            d->kernel = d->kname;
            continue;
        }
        d->uses_mfma = !e->strict && y2h_conv_uses_mfma(&c);
        if (d->fused_pool && !d->uses_mfma) {
            /* the shape test of the fusion pass was optimistic (e.g. misaligned input view): give the conv its own buffer back */
            y2_ldev *md = ld_of(&net->layers[i + 1]);
            d->fused_pool = 0; md->fused_into = -1; md->kernel = "maxpool_nhwc";
            if (alloc_activations(d, l) != 0) return -1;
            conv_query(net, i, &c, x, ldx);
        }
        d->has_w_ref = !d->uses_mfma;
        d->kernel = y2h_conv_variant(&c, e->strict);
        if (l->type == CONNECTED && !d->uses_mfma) d->kernel = "connected_ref";
        if (d->fused_pool) { snprintf(d->kname, sizeof d->kname, "%s+maxpool2", d->kernel); d->kernel = d->kname; }
    }
    return 0;
}

/* The Winograd form a convolution runs in, and the name of its kernel.  The precedence is stated here and
 * nowhere else: the split GEMM (the rule: include/y2_split_rule.h, asked through y2h_wino_split_plan) beats fp32 Winograd
 * (y2_wino_rule.h, y2h_wino_plan), which beats the fused stationary kernel (y2_winos_rule.h, y2h_winos_plan); the first
 * whose rule takes the descriptor has it, and a descriptor none takes stays direct, its name untouched.  Host arithmetic
 * only. */
int y2_conv_form_of(const y2h_conv *c, int fused_pool, char *name, size_t name_len)
{
    const char *pool = fused_pool ? "+maxpool2" : "";
    y2h_wino_split x;
    y2h_wino w;
    y2h_winos s;
    if (y2h_wino_split_plan(c, &x) == 0 && x.take) { snprintf(name, name_len, "conv_winox_f32_%dx%dx%d%s", x.bm, x.bn, x.bk, pool); return Y2_FORM_WINOX; }
    if (y2h_wino_plan(c, &w) == 0 && w.take) { snprintf(name, name_len, "conv_wino_f32_%dx%dx32%s", w.bm, w.bn, pool); return Y2_FORM_WINO; }
    if (y2h_winos_plan(c, &s) == 0 && s.take) { snprintf(name, name_len, "conv_winos_f32_c%d%s", s.form, pool); return Y2_FORM_WINOS; }
    return Y2_FORM_DIRECT;
}

/* The form of a layer: a Winograd form where y2_conv_form_of gives one -- nothing that runs in a Winograd form moves -- and
 * among the layers it leaves direct the direct split kernel where its rule takes the descriptor (y2_splitd_rule.h,
 * y2h_conv_splitd_plan).  Host arithmetic only. */
int y2_conv_layer_form(const y2h_conv *c, int fused_pool, char *name, size_t name_len)
{
    const int form = y2_conv_form_of(c, fused_pool, name, name_len);
    y2h_splitd sd;
    if (form != Y2_FORM_DIRECT) return form;
    if (y2h_conv_splitd_plan(c, &sd) == 0 && sd.take) {
        snprintf(name, name_len, "conv_splitd_f32_%dx%dx%d%s", sd.bm, sd.bn, sd.bk, fused_pool ? "+maxpool2" : "");
        return Y2_FORM_SPLITD;
    }
    return Y2_FORM_DIRECT;
}

/* which of the fp32 matrix-core convolutions run as a Winograd form or as the direct split kernel instead (y2_conv_layer_form).  Such a layer keeps its
 * form's U in the arena in place of its packed filters and is named after the form; its launches sit between the layer's
 * two timing events like any layer's.  Never in strict or half mode. */
static int plan_conv_forms(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    if (e->strict || e->half) return 0;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        y2h_conv c;
        const float *x; int ldx;
        if (l->type != CONVOLUTIONAL || !d->uses_mfma || l->xnor) continue;
        y2_input_view(net, i, &x, &ldx);
        conv_query(net, i, &c, x, ldx);
        d->form = y2_conv_layer_form(&c, d->fused_pool, d->kname, sizeof d->kname);
        if (d->form != Y2_FORM_DIRECT) d->kernel = d->kname;
    }
    return 0;
}

/* timing events */
static int plan_timing_events(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    if (e->n_ev == net->n + 1) return 0;
    if (e->ev) { for (i = 0; i < e->n_ev; ++i) y2h_event_destroy(e->ev[i]); free(e->ev); }
    e->n_ev = net->n + 1;
    e->ev = calloc(e->n_ev, sizeof(y2h_event));
    for (i = 0; i < e->n_ev; ++i) HIP_OR_ERR(y2h_event_create(&e->ev[i]));
    return 0;
}

/* Pass order is part of the plan: fusion must see placement, the buffers must see fusion and fp16 storage, the kernel
 * choice reads the buffers' alignment.  plan_conv_forms follows plan_conv_kernels because it chooses among the layers that
 * pass put on the matrix cores, with the fused pool as that pass left it, and overwrites the name it gave; it precedes
 * y2_arena_layout because the form decides what the filter slot holds.  The arena layout must see both. */
int y2_engine_build(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (plan_checks(net) != 0) return -1;
    y2_free_plan(net);
    if (plan_batches(net) != 0 || plan_routes(net) != 0 || plan_pool_fusion(net) != 0 || plan_half(net) != 0 ||
        plan_activations(net) != 0 || plan_input_copies(net) != 0 || plan_input(net) != 0 || plan_output(net) != 0 ||
        plan_head_constants(net) != 0 || plan_conv_kernels(net) != 0 || plan_conv_forms(net) != 0) return -1;
    y2_arena_layout(net);
    /* the arena commit: signature, reallocation, the refusal of a replicated rank whose layout changed */
    if (plan_workspace(net) != 0 || y2_arena_commit(net) != 0 || plan_timing_events(net) != 0) return -1;
    e->built = 1;
    e->built_batch = net->batch; e->built_w = net->w; e->built_h = net->h; e->built_strict = e->strict;
    e->built_fusion = e->fusion;
    e->built_half = e->half;
    if (!e->weights_external) e->arena_pending = 0;              /* an ordinary build uploads the host weights below */
    e->built_autotune = e->arena_pending ? 0 : e->autotune;      /* a skipped measurement is made up for at the next forward */
    if (e->weights_dirty && !e->weights_external && y2_upload_weights(net) != 0) return -1;
    if (autotune_allowed(e)) {
        /* measured tile shapes: needs the buffers and the arena, so it runs last; the scratch is sized again afterwards */
        if (autotune_layers(net) != 0 || plan_workspace(net) != 0) { e->built = 0; return -1; }
    }
    return 0;
}
