/*
 * Network runtime: the engine's lifecycle, the forward pass, graph replay and the public runtime API.
 * The plan the forward pass runs is built by y2_plan.c, the weight arena by y2_arena.c, [rnn] / [gru] are in y2_rec.c.
 *
 * Host-side replacement for src_yolo2/network.c (forward_network :145,
 * network_predict :458, set_batch_network :308, resize_network :322,
 * free_network :592) and src_yolo2/network_kernels.cu (forward_network_gpu :43,
 * network_predict_gpu :392), re-designed for one MI355X:
 *
 *  - activations are NHWC in HBM and never leave it between layers; there is
 *    no im2col workspace, no per-call cudaMalloc/H2D/cudaFree
 *    (network_kernels.cu:399,405), no per-layer fill of `delta`
 *    (network_kernels.cu:50-52);
 *  - [route] is planned away: a one-input route aliases its source, and the
 *    sources of a concatenating route write straight into the route's buffer
 *    at their channel offset (conv / maxpool / reorg kernels take an output
 *    channel stride), so the copy_ongpu launches of route_layer.c:104-117
 *    disappear; a copy kernel remains only for sources that cannot be placed;
 *  - all weights sit in ONE device allocation ("arena") in kernel layout
 *    ([n][kh][kw][c] filters + the per-filter epilogue constants), so that a
 *    multi-GPU launcher replicates the model with a single broadcast;
 *  - the plan is built lazily at the first predict after parse / resize /
 *    set_batch, which also lets set_batch_network grow the batch safely.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

void y2_drop_graphs(y2_engine *e)
{
    int k;
    for (k = 0; k < 4; ++k) {
        if (e->graphs[k]) y2h_graph_destroy(e->graphs[k]);
        e->graphs[k] = NULL; e->graph_srcs[k] = NULL;
    }
    e->graph = NULL; e->graph_src = NULL; e->graph_next = 0;
}

y2_engine *y2_engine_of(const network *net) { return net ? (y2_engine *)net->engine : NULL; }

int y2_engine_create(network *net)
{
    y2_engine *e = calloc(1, sizeof *e);
    int i;
    const char *st = getenv("Y2_STRICT");
    e->device = net->gpu_index;
    e->weights_dirty = 1;
    e->strict = (st && atoi(st) != 0) ? 1 : 0;
    e->fusion = getenv("Y2_NO_FUSE") ? 0 : 1;
    { const char *g = getenv("Y2_GRAPH"); e->graph_on = (g && atoi(g) != 0) ? 1 : 0; }
    { const char *hf = getenv("Y2_FP16"); e->half = (hf && atoi(hf) != 0) ? 1 : 0; }
    { const char *at = getenv("Y2_AUTOTUNE"); e->autotune = (at && atoi(at) != 0) ? 1 : 0; }
    e->n_layers = net->n;
    e->out_layer = y2_out_layer(net);
    for (i = 0; i < net->n; ++i) {
        y2_ldev *d = calloc(1, sizeof *d);
        d->eng = e;
        d->index = i;
        d->placed_in = -1;
        d->alias_of = -1;
        d->fused_into = -1;
        net->layers[i].dev = d;
    }
    net->engine = e;
    y2_engine_host_output(net);
    return 0;
}

/* (Re)allocate the host output buffer for the current batch/size and publish it as l.output of the output
 * layer.  Done at parse time and on set_batch / resize, not at the first predict: the reference allocates
 * l.output in make_*_layer, and callers copy `layer l = net.layers[n-1]` long before they predict. */
void y2_engine_host_output(network *net)
{
    y2_engine *e = y2_engine_of(net);
    layer *ol;
    size_t need;
    if (!e || !net->layers) return;
    e->out_layer = y2_out_layer(net);
    ol = &net->layers[e->out_layer];
    need = (size_t)net->batch * ol->outputs;
    if (need > e->h_out_cap || !e->h_out) {
        if (e->h_out_pinned) y2h_host_free(e->h_out); else free(e->h_out);
        e->h_out = NULL; e->h_out_pinned = 0;
        /* With a GPU in the machine the buffer is pinned memory of its own (hipHostMalloc, never a registered heap block:
         * profiles/r02_notes.md), so that network_predict's device-to-host copy lands in the buffer the caller reads --
         * one copy, as the reference's cuda_pull_array into l.output (network_kernels.cu:412-416).  Without one (cfg tools,
         * the CPU test suite) it is plain page-aligned memory; nothing can be predicted then anyway. */
        if (y2h_device_count() > 0 && y2h_host_alloc((void **)&e->h_out, (need ? need : 1) * sizeof(float)) == 0) e->h_out_pinned = 1;
        else if (posix_memalign((void **)&e->h_out, 4096, (need ? need : 1) * sizeof(float)) != 0) e->h_out = NULL;
        if (e->h_out) memset(e->h_out, 0, (need ? need : 1) * sizeof(float));
        e->h_out_cap = need;
    }
    ol->output = e->h_out;
}

void y2_engine_invalidate(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->built = 0;
}

void y2_engine_destroy(network *net)
{
    y2_engine *e = y2_engine_of(net);
    int i;
    if (!e) return;
    if (e->stream || e->arena || e->built) y2h_set_device(e->device);
    y2_dream_free_cached(e);
    y2_train_free(net);
    free(e->lr.steps); free(e->lr.scales);
    y2_free_plan(net);
    y2_feed_close(net);
    for (i = 0; i < net->n; ++i) {
        y2_ldev *d = ld_of(&net->layers[i]);
        if (!d) continue;
        y2h_free(d->d_anchors); y2h_free(d->d_tree_block); free(d->h_tree_block); y2h_free(d->d_map);
        y2h_free(d->d_tree_best);
        y2h_free(d->d_tree_leaf); free(d->h_tree_leaf);
        free(d);
        net->layers[i].dev = NULL;
    }
    y2h_free(e->arena);
    y2_chargen_free(e);
    y2_depth_free(e);
    y2_kcf_free_engine(e);
    y2_go_free_engine(e);
    y2h_host_free(e->h_out_stage);
    y2h_host_free(e->h_reg_stage);
    y2h_host_free(e->h_tta); y2h_free(e->d_tta);
    if (e->ev_reg) y2h_event_destroy(e->ev_reg);
    if (e->h_out_pinned) y2h_host_free(e->h_out); else free(e->h_out);
    if (e->ev) { for (i = 0; i < e->n_ev; ++i) y2h_event_destroy(e->ev[i]); free(e->ev); }
    if (e->ev_det) y2h_event_destroy(e->ev_det);
    if (e->ev_out) y2h_event_destroy(e->ev_out);
    y2_drop_graphs(e);
    if (e->det_stream) y2h_stream_destroy(e->det_stream);
    if (e->ev_fwd) y2h_event_destroy(e->ev_fwd);
    y2h_stream_destroy(e->stream);
    free(e);
    net->engine = NULL;
}

static int ensure_built(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) { y2_fail("network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (y2_train_sync_if_dirty(net) != 0) return -1;
    if (!e->built || e->built_batch != net->batch || e->built_w != net->w || e->built_h != net->h ||
        e->built_strict != e->strict || e->built_fusion != e->fusion || e->built_half != e->half ||
        e->built_autotune != e->autotune) {
        if (y2_engine_build(net) != 0) return -1;
    } else {
        HIP_OR_ERR(y2h_set_device(e->device));
        if (e->weights_dirty && !e->weights_external && y2_upload_weights(net) != 0) return -1;
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* forward                                                             */
/* ------------------------------------------------------------------ */
/* One forward pass = a fixed sequence of 20-60 kernel launches with fixed arguments as long as the plan and the input
 * pointer stay the same.  At batch 1 (the Kinect application's mode) most of them run for 5-30 us, the same order as
 * the host-side cost of a launch; with y2_set_graph the sequence is captured into a hipGraph at the first call and
 * replayed with one hipGraphLaunch afterwards.  A new input pointer re-records; a new plan drops the graph. */
int y2_engine_forward(network *net, const float *d_input_nchw)
{
    y2_engine *e;
    if (ensure_built(net) != 0) return -1;
    e = y2_engine_of(net);
    if ((net->c <= 0 || net->h <= 0 || net->w <= 0) && !y2_flat_input(net)) { y2_fail("network input must be an image (h,w,c > 0)"); return -1; }
    if (!d_input_nchw) d_input_nchw = e->d_in_nchw;     /* filled by y2_ingest_u8 */
    if (!e->graph_on || e->timing || e->strict) return y2_enqueue_forward(net, d_input_nchw);
    {   /* a recording bakes in each softmax's temperature, which callers write between calls (test_char_rnn, rnn.c:244) */
        uint64_t sig = 1469598103934665603ull;
        int i;
        for (i = 0; i < net->n; ++i) {
            uint32_t b;
            if (net->layers[i].type != SOFTMAX) continue;
            memcpy(&b, &net->layers[i].temperature, sizeof b);
            sig = (sig ^ b) * 1099511628211ull;
        }
        if (sig != e->graph_params) { y2_drop_graphs(e); e->graph_params = sig; }
    }
    /* y2_set_detect_overlap together with graph replay: the wait that keeps this forward's region layer from overwriting
     * d_region while the previous batch's decode / NMS still read it on det_stream cannot live inside the graph (it would
     * be captured once, against whatever det_pending was then, on an event recorded outside the capture).  It is issued
     * here, in front of the capture and of every replay: the whole forward waits, slightly more than the eager path's
     * wait in front of the region layer, and the captured sequence itself carries no wait (e->capturing). */
    if (e->det_overlap && e->det_pending == 1 && e->ev_det) HIP_OR_ERR(y2h_stream_wait_event(e->stream, e->ev_det));
    if (!e->graph || e->graph_src != d_input_nchw) {
        /* one recording per input pointer, up to four (y2_feed_forward alternates between its HBM slots: with a single
         * recording every step of a double-buffered feed would capture and instantiate again) */
        int k, slot = -1;
        for (k = 0; k < 4; ++k) if (e->graphs[k] && e->graph_srcs[k] == d_input_nchw) slot = k;
        if (slot < 0) {
            y2h_graph g = NULL;
            slot = e->graph_next;
            e->graph_next = (e->graph_next + 1) & 3;
            if (e->graphs[slot]) { y2h_graph_destroy(e->graphs[slot]); e->graphs[slot] = NULL; e->graph_srcs[slot] = NULL; }
            e->graph = NULL; e->graph_src = NULL;
            HIP_OR_ERR(y2h_graph_begin(e->stream));
            e->capturing = 1;
            if (y2_enqueue_forward(net, d_input_nchw) != 0) { e->capturing = 0; y2h_graph_abort(e->stream); return -1; }
            e->capturing = 0;
            if (y2h_graph_end(e->stream, &g) != 0) { y2_fail("hipGraph capture of the forward pass failed: %s", y2h_last_error()); return -1; }
            e->graphs[slot] = g; e->graph_srcs[slot] = d_input_nchw;
        }
        e->graph = e->graphs[slot];
        e->graph_src = d_input_nchw;
    }
    e->cur_input = d_input_nchw;
    HIP_OR_ERR(y2h_graph_launch(e->graph, e->stream));
    return 0;
}

/* bring the caller's NCHW input into the form layer 0 reads (Y2_IN_*) */
static int forward_input(network *net, const float *d_input_nchw)
{
    y2_engine *e = y2_engine_of(net);
    const int misaligned = ((uintptr_t)d_input_nchw % 16) != 0;
    e->cur_input = d_input_nchw;
    if (y2_flat_input(net)) {
        /* a recurrent first layer reads the caller's rows; the plan chose its forms for a 16-byte aligned buffer */
        if (misaligned && d_input_nchw != e->d_in_nchw) {
            HIP_OR_ERR(y2h_memcpy_d2d(e->d_in_nchw, d_input_nchw, e->in_floats * sizeof(float), e->stream));
            e->cur_input = e->d_in_nchw;
        }
        return 0;
    }
    switch (e->in_form) {
    case Y2_IN_NCHW:
        /* the first layer reads d_input_nchw (fp32 kernel: dword loads, any float pointer).  The fp16 first-layer kernel
         * reads the planes with 16-byte loads: a caller's pointer that is not 16-byte aligned (a frame slice of an
         * odd-sized batch) goes through the engine's own input slot */
        if (!e->half || !misaligned) break;
        if (d_input_nchw != e->d_in_nchw) HIP_OR_ERR(y2h_memcpy_d2d(e->d_in_nchw, d_input_nchw, e->in_floats * sizeof(float), e->stream));
        e->cur_input = e->d_in_nchw;
        break;
    case Y2_IN_NHWC4_HALO_F16:
        HIP_OR_ERR(y2h_nchw_to_nhwc4_halo_f16(d_input_nchw, e->d_in_nhwc, net->batch, net->c, net->h, net->w, e->stream));
        break;
    case Y2_IN_NHWC_HALO:
        HIP_OR_ERR(y2h_nchw_to_nhwc_halo(d_input_nchw, e->d_in_nhwc, net->batch, net->c, net->h, net->w, net->c, e->in_halo_px, e->stream));
        break;
    case Y2_IN_NHWC:
        HIP_OR_ERR(y2h_nchw_to_nhwc(d_input_nchw, e->d_in_nhwc, net->batch, net->c, net->h, net->w, net->c, e->stream));
        break;
    }
    return 0;
}

/* an activation the producing kernel does not apply runs as a pass of its own over the stored output */
int y2_activate_after(y2_engine *e, ACTIVATION a, float *y, int ld, long rows, int n)
{
    if (!y2_act_in_kernel(a)) HIP_OR_ERR(y2h_activate_array(y, ld, rows, n, y2_act_code(a), e->stream));
    return 0;
}

static int forward_convolutional(network *net, int i, const float *x, int ldx)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    const y2_conv_form *form = &y2_conv_forms[d->form];
    y2h_conv c;
    if (l->xnor) {
        /* the input view already points at d_bin: binarize the producer's activations into it first */
        const float *px; int pld;
        if (i == 0) { px = e->d_in_nhwc; pld = net->c; }
        else { const y2_ldev *p = ld_of(&net->layers[i - 1]); px = p->out; pld = p->out_ld; }
        HIP_OR_ERR(y2h_binarize(px, pld, d->d_bin, (long)l->batch * l->h * l->w, l->c, e->stream));
    }
    y2_conv_desc(net, i, &c, x, ldx);
    if (form->forward) HIP_OR_ERR(form->forward(&c, e->stream));       /* w_packed holds the form's U (y2_arena.c) */
    else HIP_OR_ERR(y2h_conv_forward(&c, e->strict, e->stream));
    return y2_activate_after(e, l->activation, d->out, d->out_ld, (long)l->batch * l->out_h * l->out_w, l->out_c);
}

/* the sources of a concatenating route that could not be placed in its buffer are copied into it */
static int forward_route(network *net, int i)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    int k, choff = 0;
    if (l->n < 2 || !d->copy_mask) return 0;
    for (k = 0; k < l->n; ++k) {
        const layer *src = &net->layers[l->input_layers[k]];
        const y2_ldev *sd = ld_of(src);
        if ((d->copy_mask & (1u << k)) && d->out_half)
            HIP_OR_ERR(y2h_copy_channels_f16(sd->out, sd->out_ld, (unsigned short *)d->out + choff, d->out_ld, src->out_c,
                                             (long)l->batch * l->out_h * l->out_w, e->stream));
        else if (d->copy_mask & (1u << k))
            HIP_OR_ERR(y2h_copy_channels(sd->out, sd->out_ld, d->out + choff, d->out_ld, src->out_c,
                                         (long)l->batch * l->out_h * l->out_w, e->stream));
        choff += src->out_c;
    }
    return 0;
}

static int forward_region(network *net, int i, const float *x, int ldx)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    y2_ldev *d = ld_of(l);
    const tree *t = l->softmax_tree;
    /* y2_set_detect_overlap: the previous batch's decode / NMS may still be reading d_region on det_stream */
    if (e->det_overlap && e->det_pending == 1 && i == e->out_layer && !e->capturing) HIP_OR_ERR(y2h_stream_wait_event(e->stream, e->ev_det));
    /* The (score, class) pair per box that detect mode needs, as a by-product of this layer: it saves the detect call
     * a sweep over the class rows (batch-1 latency), but it lengthens the forward; with y2_set_detect_overlap that
     * sweep runs beside the NEXT forward on the detection stream, where it is the cheaper place (yolo9000 544 b8:
     * 1999 against 1977 images/s, profiles/r03_notes.md section 10) */
    d->tree_best_valid = 0;
    if (t && d->d_tree_best && !e->det_overlap) d->tree_best_valid = 1;
    if (t)
        /* (strict mode keeps the reference's double exp in the group softmax; otherwise expf: the 9418 double exps per
         * box are what this layer costs in yolo9000) */
        HIP_OR_ERR(y2h_region_forward_tree(x, ldx, d->d_region, l->batch, l->h * l->w, l->n, l->classes, l->coords, t->groups,
                                           d->d_tree_gsize, d->d_tree_goff, d->d_tree_parent, d->d_tree_order, d->d_tree_loff,
                                           d->tree_levels, d->tree_best_valid ? d->d_tree_best : NULL,
                                           e->strict ? 0 : Y2H_REGION_FAST_EXP, e->stream));
    else
        HIP_OR_ERR(y2h_region_forward(x, ldx, d->d_region, l->batch, l->h * l->w, l->n, l->classes, l->coords, l->softmax,
                                      0, d->d_tree_gsize, d->d_tree_goff, e->stream));
    return 0;
}

/* connected_layer.c:141-176.  Fast path: a 1x1 convolution over a 1x1 image on the matrix cores (weights
 * re-ordered for an NHWC producer at upload); otherwise, and in strict mode, the reference-order kernel */
static int forward_connected(network *net, int i, const float *x, int ldx)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    y2h_conv c;
    y2_conv_desc(net, i, &c, x, ldx);
    if (d->conn_ranges && !e->strict) {
        /* fp16 mode: the weight-streaming form; its epilogue applies the activation (the plan admits no other) */
        HIP_OR_ERR(y2h_connected_f16(x, (long)l->inputs, c.w_packed, c.alpha, c.beta, d->d_flat, l->outputs, d->out_half, l->batch,
                                     l->inputs, l->outputs, c.activation, d->conn_ranges, e->d_ws, e->ws_bytes, e->stream));
        return 0;
    }
    if (d->uses_mfma && !e->strict) HIP_OR_ERR(y2h_conv_forward(&c, 0, e->stream));
    else {
        const int pi = y2_producer_of(net, i);
        const layer *pl = &net->layers[pi];
        const int flat = y2_is_flat(net, pi);
        const int hw = flat ? 1 : pl->out_h * pl->out_w, cc = l->inputs / hw;
        HIP_OR_ERR(y2h_connected_ref(x, (long)l->inputs, flat ? cc : ld_of(pl)->out_ld, hw, cc, c.w_ref, d->d_flat, l->outputs,
                                     l->batch, l->batch_normalize, c.activation, c.mean, c.rinv, c.scale, c.bias, e->stream));
    }
    return y2_activate_after(e, l->activation, d->d_flat, l->outputs, (long)l->batch, l->outputs);
}

/* detection_layer.c:49-66 at inference: copy, then a softmax over every cell's class scores */
static int forward_detection(network *net, int i, const float *x)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    int b;
    HIP_OR_ERR(y2h_memcpy_d2d(d->d_flat, x, (size_t)l->batch * l->outputs * sizeof(float), e->stream));
    for (b = 0; b < l->batch && l->softmax; ++b)
        HIP_OR_ERR(y2h_softmax_rows(d->d_flat + (size_t)b * l->outputs, d->d_flat + (size_t)b * l->outputs,
                                    (long)l->side * l->side, l->classes, 1.f, e->stream));
    return 0;
}

int y2_enqueue_forward(network *net, const float *d_input_nchw)
{
    y2_engine *e = y2_engine_of(net);
    int i, rc;
    if (forward_input(net, d_input_nchw) != 0) return -1;
    if (e->timing) HIP_OR_ERR(y2h_event_record(e->ev[0], e->stream));
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        const float *x; int ldx;
        y2_input_view(net, i, &x, &ldx);
        rc = 0;
        switch (l->type) {
        case CONVOLUTIONAL: rc = forward_convolutional(net, i, x, ldx); break;
        case MAXPOOL:
            if (d->fused_into >= 0) break;       /* already produced by the conv before it */
            if (d->out_half)
                HIP_OR_ERR(y2h_maxpool_f16(x, ldx, d->out, d->out_ld, l->batch, l->h, l->w, l->c, l->size, l->stride, l->pad,
                                           l->out_h, l->out_w, e->stream));
            else
                HIP_OR_ERR(y2h_maxpool(x, ldx, d->out, d->out_ld, l->batch, l->h, l->w, l->c, l->size, l->stride, l->pad,
                                       l->out_h, l->out_w, e->stream));
            break;
        case REORG:
            if (d->out_half)
                HIP_OR_ERR(y2h_reorg_f16(x, ldx, d->out, d->out_ld, l->batch, l->h, l->w, l->c, l->stride, l->reverse, e->stream));
            else
                HIP_OR_ERR(y2h_reorg(x, ldx, d->out, d->out_ld, l->batch, l->h, l->w, l->c, l->stride, l->reverse, e->stream));
            break;
        case ROUTE: rc = forward_route(net, i); break;
        case REGION: rc = forward_region(net, i, x, ldx); break;
        case AVGPOOL:
            if (i > 0 && ld_of(&net->layers[i - 1])->out_half)
                HIP_OR_ERR(y2h_avgpool_f16(x, ldx, d->d_flat, l->batch, l->h, l->w, l->c, e->stream));
            else
                HIP_OR_ERR(y2h_avgpool(x, ldx, d->d_flat, l->batch, l->h, l->w, l->c, e->stream));
            break;
        case SOFTMAX: {
            /* the input of a softmax layer is a flat [batch][inputs] vector; an image-like producer
             * (1x1 spatial, as after avgpool) is contiguous when its stride equals its channel count */
            layer *pl = &net->layers[i - 1];
            /* a one-channel fp32 image at pixel stride 1 reads the same as NHWC and as the reference's NCHW row (go.test.cfg:
             * a 1x1 convolution to one channel in front of the softmax over the 361 points) */
            const int one_channel = i > 0 && pl->out_c == 1 && ldx == 1 && !ld_of(pl)->out_half;
            if (i == 0 || (pl->out_h * pl->out_w > 1 && pl->type != AVGPOOL && pl->type != SOFTMAX && !one_channel)) {
                y2_fail("softmax layer %d: input must be a flat vector (e.g. after avgpool)", i);
                return -1;
            }
            if (l->softmax_tree)          /* softmax_layer.c:54-55: every row is the tree's sibling groups, each softmaxed on its own */
                HIP_OR_ERR(y2h_softmax_tree_rows(x, d->d_flat, (long)l->batch * l->groups, l->inputs / l->groups, l->temperature,
                                                 l->softmax_tree->groups, d->d_tree_gsize, d->d_tree_goff, d->d_tree_group, e->stream));
            else HIP_OR_ERR(y2h_softmax_rows(x, d->d_flat, (long)l->batch * l->groups, l->inputs / l->groups, l->temperature, e->stream));
        } break;
        case CONNECTED: rc = forward_connected(net, i, x, ldx); break;
        case RNN: case GRU: rc = y2_rec_forward(net, i, x); break;
        case DROPOUT:
            break;                    /* dropout_layer.c:34: nothing happens at inference; the output is the input */
        case DETECTION: rc = forward_detection(net, i, x); break;
        case SHORTCUT: {
            const y2_ldev *fd = ld_of(&net->layers[l->index]);
            if (y2_act_code(l->activation) < 0) { y2_fail("shortcut layer %d: unknown activation %d", i, (int)l->activation); return -1; }
            if (i == 0) { y2_fail("shortcut layer %d has no input layer", i); return -1; }
            HIP_OR_ERR(y2h_shortcut(x, ldx, fd->out, fd->out_ld, d->out, d->out_ld, l->batch, l->w, l->h, l->c,
                                    l->out_w, l->out_h, l->out_c, y2_act_for_kernel(l->activation), e->stream));
            rc = y2_activate_after(e, l->activation, d->out, d->out_ld, (long)l->batch * l->out_h * l->out_w, l->out_c);
        } break;
        case CROP:
            if (d->out_half) {            /* fp16 mode: half NHWC, and the first-layer kernel's [h+2][w+2][4] form beside it */
                HIP_OR_ERR(y2h_crop_f16(x, ldx, d->out, d->out_ld, d->d_halo, l->batch, l->h, l->w, l->c, l->out_h, l->out_w, l->noadjust, e->stream));
                break;
            }
            HIP_OR_ERR(y2h_crop(x, ldx, d->out, d->out_ld, l->batch, l->h, l->w, l->c, l->out_h, l->out_w, l->noadjust, 0, e->stream));
            if (d->d_halo)
                HIP_OR_ERR(y2h_crop(x, ldx, d->d_halo, l->out_c, l->batch, l->h, l->w, l->c, l->out_h, l->out_w, l->noadjust, d->halo_px, e->stream));
            break;
        case BATCHNORM:
            HIP_OR_ERR(y2h_batchnorm(x, ldx, d->out, d->out_ld, (long)l->batch * l->h * l->w, l->c, (const float *)(e->arena + d->off_mean),
                                     (const double *)(e->arena + d->off_rinv), (const float *)(e->arena + d->off_scale), e->stream));
            break;
        case NORMALIZATION:               /* normalization_layer.c:65-94 */
            if (d->out_half)
                HIP_OR_ERR(y2h_lrn_f16(x, ldx, d->out, d->out_ld, (long)l->batch * l->h * l->w, l->c, l->size, l->alpha, l->beta, l->kappa, e->stream));
            else
                HIP_OR_ERR(y2h_lrn(x, ldx, d->out, d->out_ld, (long)l->batch * l->h * l->w, l->c, l->size, l->alpha, l->beta, l->kappa,
                                   e->strict, e->stream));
            break;
        case ACTIVE: {                    /* activation_layer.c:39-43: copy, then activate_array */
            const int flat = y2_is_flat(net, i);
            const long rows = flat ? (long)l->batch : (long)l->batch * l->out_h * l->out_w;
            const int n = flat ? l->outputs : l->out_c;
            if (d->out_half) HIP_OR_ERR(y2h_activate_copy_f16(x, ldx, d->out, d->out_ld, rows, n, y2_act_code(l->activation), e->stream));
            else HIP_OR_ERR(y2h_activate_copy(x, ldx, d->out, d->out_ld, rows, n, y2_act_code(l->activation), e->stream));
        } break;
        case LOCAL:
            if (y2_act_code(l->activation) < 0) { y2_fail("local layer %d: unknown activation %d", i, (int)l->activation); return -1; }
            if (d->out_half) {
                HIP_OR_ERR(y2h_local_f16(x, ldx, e->arena + d->off_w_packed, (const float *)(e->arena + d->off_bias), d->out, d->out_ld,
                                         l->batch, l->h, l->w, l->c, l->n, l->size, l->stride, l->pad, l->out_h, l->out_w,
                                         y2_act_for_kernel(l->activation), e->stream));
                break;
            }
            HIP_OR_ERR(y2h_local(x, ldx, (const float *)(e->arena + d->off_w_packed), (const float *)(e->arena + d->off_bias), d->out,
                                 d->out_ld, l->batch, l->h, l->w, l->c, l->n, l->size, l->stride, l->pad, l->out_h, l->out_w,
                                 y2_act_for_kernel(l->activation), e->strict, e->stream));
            rc = y2_activate_after(e, l->activation, d->out, d->out_ld, (long)l->batch * l->out_h * l->out_w, l->out_c);
            break;
        case COST:
            break;                    /* cost_layer.c:75: nothing happens without truth */
        default:
            y2_fail("layer %d: unsupported type", i);
            return -1;
        }
        if (rc != 0) return -1;
        if (e->timing) HIP_OR_ERR(y2h_event_record(e->ev[i + 1], e->stream));
    }
    return 0;
}

/* layer i's output in the reference's layout, on the device: a flat layer as it is, an image layer through an
 * NHWC -> NCHW pass into `nchw` */
static int stage_output(const network *net, int i, float *nchw, const float **src)
{
    const y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    *src = d->out;
    if (y2_is_flat(net, i) && d->out_half) {      /* a dense layer that feeds another one in fp16 mode */
        HIP_OR_ERR(y2h_f16_to_f32(d->out, nchw, (long)l->batch * l->outputs, e->stream));
        *src = nchw;
        return 0;
    }
    if (y2_is_flat(net, i)) return 0;
    if (d->out_half)
        HIP_OR_ERR(y2h_nhwc_f16_to_nchw(d->out, d->out_ld, nchw, l->batch, l->out_c, l->out_h, l->out_w, e->stream));
    else
        HIP_OR_ERR(y2h_nhwc_to_nchw(d->out, d->out_ld, nchw, l->batch, l->out_c, l->out_h, l->out_w, e->stream));
    *src = nchw;
    return 0;
}

/* the output layer of the last forward in the reference's layout, in HBM: [batch][outputs] */
int y2_output_device(network *net, const float **rows)
{
    y2_engine *e = y2_engine_of(net);
    return stage_output(net, e->out_layer, e->d_out_nchw, rows);
}

/* copy the output layer to the pinned host buffer in the reference's layout */
int y2_engine_fetch_output(network *net)
{
    y2_engine *e = y2_engine_of(net);
    const float *src;
    if (stage_output(net, e->out_layer, e->d_out_nchw, &src) != 0) return -1;
    if (e->h_out_pinned) {          /* the synchronous call: straight into the caller's buffer */
        HIP_OR_ERR(y2h_memcpy_d2h(e->h_out, src, e->out_floats * sizeof(float), e->stream));
        HIP_OR_ERR(y2h_stream_sync(e->stream));
        return 0;
    }
    HIP_OR_ERR(y2h_memcpy_d2h(e->h_out_stage, src, e->out_floats * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    memcpy(e->h_out, e->h_out_stage, e->out_floats * sizeof(float));
    return 0;
}

/* the same copy without the wait: an event is recorded behind it for y2_output_fetch */
int y2_output_enqueue(network net)
{
    y2_engine *e = y2_engine_of(&net);
    const float *src;
    if (!e || !e->built) { y2_fail("y2_output_enqueue: run a forward first"); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!e->ev_out) HIP_OR_ERR(y2h_event_create(&e->ev_out));
    if (stage_output(&net, e->out_layer, e->d_out_nchw, &src) != 0) return -1;
    HIP_OR_ERR(y2h_memcpy_d2h(e->h_out_stage, src, e->out_floats * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_event_record(e->ev_out, e->stream));
    e->out_pending = 1;
    return 0;
}

float *y2_output_fetch(network net)
{
    y2_engine *e = y2_engine_of(&net);
    if (!e || !e->out_pending) { y2_fail("y2_output_fetch: nothing was enqueued (call y2_output_enqueue after a forward)"); return NULL; }
    if (y2h_event_sync(e->ev_out) != 0) { y2_fail("y2_output_fetch: %s", y2h_last_error()); return NULL; }
    e->out_pending = 0;
    memcpy(e->h_out, e->h_out_stage, e->out_floats * sizeof(float));
    return e->h_out;
}

/* ------------------------------------------------------------------ */
/* public runtime API                                                  */
/* ------------------------------------------------------------------ */
void cuda_set_device(int n)                  /* cuda.c:12-17 */
{
    gpu_index = n;
    if (n >= 0 && y2h_set_device(n) != 0) y2_fail("cuda_set_device(%d): %s", n, y2h_last_error());
}

float *network_predict(network net, float *input)
{
    y2_engine *e;
    if (ensure_built(&net) != 0) return NULL;
    e = y2_engine_of(&net);
    if (y2h_memcpy_h2d(e->d_in_nchw, input, e->in_floats * sizeof(float), e->stream) != 0) {
        y2_fail("input upload: %s", y2h_last_error());
        return NULL;
    }
    if (y2_engine_forward(&net, e->d_in_nchw) != 0) return NULL;
    if (y2_engine_fetch_output(&net) != 0) return NULL;
    return e->h_out;
}

float *network_predict_gpu(network net, float *input) { return network_predict(net, input); }

float *y2_network_predict_device(network net, const float *d_input)
{
    if (y2_engine_forward(&net, d_input) != 0) return NULL;
    if (y2_engine_fetch_output(&net) != 0) return NULL;
    return y2_engine_of(&net)->h_out;
}

int y2_forward_device(network net, const float *d_input) { return y2_engine_forward(&net, d_input); }

int y2_prepare(network *net) { return ensure_built(net); }

void y2_set_strict(network *net, int strict)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->strict = strict ? 1 : 0;
}

void y2_set_half(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->half = on ? 1 : 0;
}

void y2_set_autotune(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->autotune = on ? 1 : 0;
}

void y2_set_detect_overlap(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) return;
    if (e->det_pending == 1 && e->ev_det) y2h_event_sync(e->ev_det);     /* nothing of the other mode left in flight */
    e->det_overlap = on ? 1 : 0;
}

void y2_set_fusion(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->fusion = on ? 1 : 0;
}

void y2_set_graph(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) return;
    e->graph_on = on ? 1 : 0;
    if (!on) y2_drop_graphs(e);
}

void y2_set_timing(network *net, int on)
{
    y2_engine *e = y2_engine_of(net);
    if (e) e->timing = on ? 1 : 0;
}

int y2_layer_times_ms(network net, float *ms, int max_layers)
{
    y2_engine *e = y2_engine_of(&net);
    int i, n;
    if (!e || !e->built || !e->timing) return 0;
    n = net.n < max_layers ? net.n : max_layers;
    for (i = 0; i < n; ++i) if (y2h_event_elapsed_ms(e->ev[i], e->ev[i + 1], &ms[i]) != 0) return i;
    return n;
}

const char *y2_layer_kernel(network net, int i)
{
    if (i < 0 || i >= net.n || !net.layers[i].dev) return "";
    return ld_of(&net.layers[i])->kernel ? ld_of(&net.layers[i])->kernel : "";
}

void *y2_stream(network net) { y2_engine *e = y2_engine_of(&net); return e ? e->stream : NULL; }
void y2_sync(network net) { y2_engine *e = y2_engine_of(&net); if (e && e->stream) y2h_stream_sync(e->stream); }

int y2_pull_layer_output(network net, int i, float *dst)
{
    y2_engine *e = y2_engine_of(&net);
    layer *l;
    y2_ldev *d;
    float *tmp = NULL;
    const float *src;
    size_t n;
    int rc;
    if (!e || !e->built || i < 0 || i >= net.n) { y2_fail("y2_pull_layer_output: no forward has run"); return -1; }
    l = &net.layers[i];
    d = ld_of(l);
    n = (size_t)l->batch * (is_recurrent(l) ? l->steps : 1) * l->outputs;     /* a recurrent layer: all T steps */
    if (d->fused_pool) {
        y2_fail("layer %d is fused with the maxpool behind it and its full-resolution output is never stored; "
                "call y2_set_fusion(&net, 0) (or set Y2_NO_FUSE=1) to inspect it", i);
        return -1;
    }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!y2_is_flat(&net, i) || d->out_half) HIP_OR_ERR(y2h_malloc((void **)&tmp, n * sizeof(float)));
    rc = stage_output(&net, i, tmp, &src);
    if (rc == 0 && (y2h_memcpy_d2h(dst, src, n * sizeof(float), e->stream) != 0 || y2h_stream_sync(e->stream) != 0)) {
        y2_fail("y2_pull_layer_output: %s", y2h_last_error());
        rc = -1;
    }
    y2h_free(tmp);
    return rc;
}

float *get_network_output(network net)       /* network.c:173-181 */
{
    int i = y2_out_layer(&net);
    return net.layers[i].output;
}
float *get_network_output_gpu(network net) { return get_network_output(net); }
int get_network_output_size(network net) { return net.layers[y2_out_layer(&net)].outputs; }
int get_network_input_size(network net) { return net.layers[0].inputs; }

void set_batch_network(network *net, int b)  /* network.c:308-320 */
{
    int i;
    if (b <= 0) { y2_fail("set_batch_network: batch %d", b); return; }
    for (i = 0; i < net->n; ++i)
        if (is_recurrent(&net->layers[i]) && b % net->layers[i].steps) {
            y2_fail("set_batch_network: batch %d is not a multiple of time_steps %d (layer %d)", b, net->layers[i].steps, i);
            return;
        }
    for (i = 0; i < net->n; ++i)
        if (is_recurrent(&net->layers[i])) { y2_engine_invalidate(net); break; }   /* the re-plan zeroes the state */
    if (y2_train_sync_if_dirty(net) != 0) return;      /* train, set_batch_network(&net, 1), predict: the steps are kept */
    y2_train_free(net);
    net->batch = b;
    for (i = 0; i < net->n; ++i) net->layers[i].batch = is_recurrent(&net->layers[i]) ? b / net->layers[i].steps : b;
    y2_engine_host_output(net);     /* HBM buffers are re-planned at the next predict if the batch changed */
}

int resize_network(network *net, int w, int h)   /* network.c:322-388 */
{
    int i, inputs = 0, k;
    for (i = 0; i < net->n; ++i)
        if (is_recurrent(&net->layers[i])) {       /* the reference errors too: "Cannot resize this type of layer" */
            y2_fail("resize_network: layer %d (%s) cannot be resized", i, get_layer_string(net->layers[i].type));
            return -1;
        }
    /* [activation] has no resize (network.c:358-360); found before anything is changed, so the network stays usable.
     * Layers behind an [avgpool] are not visited (network.c:367) */
    for (i = 0; i < net->n && net->layers[i].type != AVGPOOL; ++i)
        if (net->layers[i].type == ACTIVE) {
            fprintf(stderr, "Resizing type %d \n", (int)ACTIVE);
            y2_fail("Cannot resize this type of layer");
            return -1;
        }
    if (y2_train_sync_if_dirty(net) != 0) return -1;
    y2_train_free(net);
    net->w = w; net->h = h;
    net->inputs = w * h * net->c;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        switch (l->type) {
        case CONVOLUTIONAL:                  /* convolutional_layer.c:360-398 */
            l->w = w; l->h = h;
            l->out_w = (l->w + 2 * l->pad - l->size) / l->stride + 1;
            l->out_h = (l->h + 2 * l->pad - l->size) / l->stride + 1;
            l->outputs = l->out_h * l->out_w * l->out_c;
            l->inputs = l->w * l->h * l->c;
            l->workspace_size = (size_t)l->out_h * l->out_w * l->size * l->size * l->c * sizeof(float);
            break;
        case MAXPOOL:                        /* maxpool_layer.c:54-77 */
            l->w = w; l->h = h;
            l->inputs = h * w * l->c;
            l->out_w = (w + 2 * l->pad) / l->stride;
            l->out_h = (h + 2 * l->pad) / l->stride;
            l->outputs = l->out_w * l->out_h * l->c;
            break;
        case CROP:                           /* crop_layer.c:48-66 */
            l->w = w; l->h = h;
            l->out_w = l->scale * w;
            l->out_h = l->scale * h;
            l->inputs = l->w * l->h * l->c;
            l->outputs = l->out_h * l->out_w * l->out_c;
            break;
        case REGION:                         /* region_layer.c:53-71 */
            l->w = w; l->h = h;
            l->outputs = h * w * l->n * (l->classes + l->coords + 1);
            l->inputs = l->outputs;
            break;
        case ROUTE: {                        /* route_layer.c:39-71 */
            layer *first = &net->layers[l->input_layers[0]];
            l->out_w = first->out_w; l->out_h = first->out_h; l->out_c = first->out_c;
            l->outputs = first->outputs;
            l->input_sizes[0] = first->outputs;
            for (k = 1; k < l->n; ++k) {
                layer *nx = &net->layers[l->input_layers[k]];
                l->outputs += nx->outputs;
                l->input_sizes[k] = nx->outputs;
                if (nx->out_w == first->out_w && nx->out_h == first->out_h) l->out_c += nx->out_c;
                else l->out_h = l->out_w = l->out_c = 0;
            }
            l->inputs = l->outputs;
            l->h = l->out_h; l->w = l->out_w; l->c = l->out_c;
        } break;
        case REORG:                          /* reorg_layer.c:45-76 */
            l->w = w; l->h = h;
            if (l->reverse) { l->out_w = w * l->stride; l->out_h = h * l->stride; l->out_c = l->c / (l->stride * l->stride); }
            else { l->out_w = w / l->stride; l->out_h = h / l->stride; l->out_c = l->c * (l->stride * l->stride); }
            l->outputs = l->out_h * l->out_w * l->out_c;
            l->inputs = l->outputs;
            break;
        case AVGPOOL:                        /* avgpool_layer.c:33-38 */
            l->w = w; l->h = h;
            l->inputs = h * w * l->c;
            break;
        case NORMALIZATION:                  /* normalization_layer.c:37-63 */
            l->w = l->out_w = w; l->h = l->out_h = h;
            l->inputs = l->outputs = w * h * l->c;
            break;
        case COST: case SOFTMAX:
            l->inputs = inputs; l->outputs = inputs;
            break;
        default:
            fprintf(stderr, "Resizing type %d \n", (int)l->type);
            y2_fail("Cannot resize this type of layer");
            return -1;
        }
        inputs = l->outputs;
        w = l->out_w; h = l->out_h;
        if (l->type == AVGPOOL) break;       /* network.c:366: layers after avgpool keep their size */
    }
    net->outputs = net->layers[y2_out_layer(net)].outputs;
    y2_engine_invalidate(net);
    y2_engine_host_output(net);
    return 0;
}

static void free_tree(tree *t)
{
    int i;
    if (!t) return;
    if (t->name) for (i = 0; i < t->n; ++i) free(t->name[i]);
    free(t->name); free(t->leaf); free(t->parent); free(t->group); free(t->group_size); free(t->group_offset);
    free(t);
}

void free_network(network net)               /* network.c:592-609 */
{
    int i;
    if (!net.layers) return;
    y2_engine_destroy(&net);
    for (i = 0; i < net.n; ++i) {
        layer *l = &net.layers[i];
        free(l->weights); free(l->biases); free(l->scales); free(l->rolling_mean); free(l->rolling_variance);
        free(l->input_layers); free(l->input_sizes); free(l->map); free(l->cost);
        free_tree(l->softmax_tree);
        if (is_recurrent(l)) {
            layer *subs[9] = { l->input_layer, l->self_layer, l->output_layer, l->input_z_layer, l->state_z_layer, l->input_r_layer,
                               l->state_r_layer, l->input_h_layer, l->state_h_layer };
            int k;
            for (k = 0; k < 9; ++k) {
                if (!subs[k]) continue;
                free(subs[k]->weights); free(subs[k]->biases); free(subs[k]->scales); free(subs[k]->rolling_mean);
                free(subs[k]->rolling_variance); free(subs[k]);
            }
        }
    }
    free(net.layers);
    free(net.seen);
}

void reset_rnn_state(network net, int b)      /* rnn.c:116-127 */
{
    y2_engine *e = y2_engine_of(&net);
    int i;
    if (!e) { y2_fail("reset_rnn_state: network has no engine (was it built by parse_network_cfg?)"); return; }
    for (i = 0; i < net.n; ++i) {
        const layer *l = &net.layers[i];
        const int B = is_recurrent(l) ? net.batch / l->steps : 0;
        if (is_recurrent(l) && (b < -1 || b >= B)) { y2_fail("reset_rnn_state: item %d outside the %d sequences of layer %d", b, B, i); return; }
    }
    /* before the first forward (or a re-plan) there is nothing to clear: the plan starts every state at zero */
    if (!e->built || e->built_batch != net.batch) return;
    if (y2h_set_device(e->device) != 0) { y2_fail("reset_rnn_state: %s", y2h_last_error()); return; }
    for (i = 0; i < net.n; ++i) {
        const layer *l = &net.layers[i];
        const y2_ldev *d = ld_of(l);
        size_t H;
        if (!is_recurrent(l) || !d->d_state) continue;
        H = (size_t)y2_rec_hidden(l);
        if (y2h_memset(d->d_state + (b < 0 ? 0 : (size_t)b * H), 0, (b < 0 ? (size_t)l->batch : 1) * H * sizeof(float), e->stream) != 0) {
            y2_fail("reset_rnn_state: %s", y2h_last_error());
            return;
        }
    }
}

void top_predictions(network net, int k, int *index)   /* network.c:449-454 */
{
    top_k(get_network_output(net), get_network_output_size(net), k, index);
}

char *get_layer_string(LAYER_TYPE a)         /* network.c:73-130 */
{
    switch (a) {
    case CONVOLUTIONAL: return "convolutional";
    case MAXPOOL: return "maxpool";
    case ROUTE: return "route";
    case REORG: return "reorg";
    case REGION: return "region";
    case AVGPOOL: return "avgpool";
    case SOFTMAX: return "softmax";
    case COST: return "cost";
    case SHORTCUT: return "shortcut";
    case CROP: return "crop";
    case LOCAL: return "local";
    case BATCHNORM: return "batchnorm";
    case CONNECTED: return "connected";
    case DROPOUT: return "dropout";
    case DETECTION: return "detection";
    case RNN: return "rnn";
    case GRU: return "gru";
    case NORMALIZATION: return "normalization";
    case ACTIVE: return "activation";
    default: return "none";
    }
}
