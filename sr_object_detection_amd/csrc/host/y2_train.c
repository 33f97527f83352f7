/*
 * Training on the device: host-side replacement for the other half of src_yolo2/network.c -- train_network_datum
 * (:225-243), backward_network (:197-215), update_network (:160-171), get_current_rate (:48-79) -- and for the
 * forward(train) / backward / update functions of the convolutional, batch-norm, maxpool, avgpool, softmax, cost, route,
 * reorg, region, connected, dropout and detection layers, whose loop nests run as the y2h_train_* kernels (y2_train.hip,
 * y2_train_det.hip, y2_train_dense.hip).
 *
 * A [connected] layer's master is [outputs][inputs] with the K index in the order of the dense NHWC activation it reads
 * (y2_train_pack_dense_weights); its three products are fp32 in every precision mode.  A [dropout] owns no activation:
 * its output and delta ARE those of the layer in front (dropout_layer.c scales both in place), so that layer's
 * gradient_array reads the post-dropout values, as the reference's does; its draws are libc rand() on the host, in the
 * reference's index order, layer by layer in forward order.
 *
 * The inference plan folds batch norm, fuses pooling and keeps weights in per-kernel layouts, so nothing of it is
 * reused: the trainer owns master parameters, their update buffers and per layer output / delta / x / x_norm / mean /
 * variance, all dense NHWC.  struct network and struct layer are untouched (layer.delta stays NULL); the schedule of
 * the [net] section lives in the engine.
 *
 * The reference zeroes every delta in the forward pass (network.c:152-154); in the backward pass the consumers of a layer
 * then add to its delta in descending layer order (col2im_cpu, backward_maxpool_layer, backward_route_layer ...), and
 * [reorg] assigns.  plan_deltas walks that order once at prepare time: the first writer of a delta stores (0 + v == v),
 * every later one adds -- its kernel writes into the staging buffer, which a step does not use otherwise, and one add
 * follows -- and a reorg always stores.  A delta nobody writes keeps the zeros it was allocated with.  A network
 * without [route] has one writer per delta and launches what it launched before routes were known here.
 *
 * The detection loader's trainer entries live here too (y2_train_load_detection, y2_train_step_loaded, y2_train_pull_input):
 * data.c:664-714 load_data_detection with its pixel work as one kernel (y2_augment.hip) that writes the trainer's NHWC input
 * in place; the draws, the truth and the packer are the device-free y2_aug.c.  The classifier loader (data.c:870-879
 * load_data_augment) is y2_train_load_classification, staged the same way: rotate_crop_image, flip and distortion are the
 * second kernel of y2_augment.hip, the draws and the label row come from y2_aug.c.
 *
 * An [rnn] trains by back-propagation through time (rnn_layer.c:83-172, CPU branch) in the composed form: the
 * products that do not depend on the step before run once over all T*B rows, the self sub-layer's forward and its delta chain
 * run step by step, the per-step batch-norm work runs as the grouped kernels of y2_train_rnn.hip.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "y2_internal.h"

typedef struct y2_tlayer {
    float *out, *delta;                 /* [batch][out_h][out_w][out_c] */
    float *x, *x_norm;                  /* batch-normalised convolutions */
    float *mean, *variance, *mean_delta, *variance_delta;
    float *weights, *weight_updates, *biases, *bias_updates, *scales, *scale_updates, *rolling_mean, *rolling_variance;
    int *idx;                           /* [maxpool] winners */
    float *cost;                        /* [cost], [region]: one float */
    y2h_train_conv g;
    int din_add;                        /* this layer is not the first writer of the delta in front of it (plan_deltas) */
    int *src_add;                       /* [route]: the same per source */
    y2h_train_region rg;                /* [region]; its anchors are `biases`, 2*n floats */
    y2h_train_region_stats *stats;
    y2h_train_dense dg;                 /* [connected] */
    int fwd_ranges, dx_ranges;          /* its reduction ranges, fixed when the workspace was sized (Y2_TRAIN_DENSE_KSPLIT is read then) */
    int src_c, src_h, src_w;            /* [connected], [dropout]: the activation in front as an image (h = w = 1: flat) */
    float *rnd, *h_rnd;                 /* [dropout]: the step's draws, [batch][inputs] in the reference's order; pinned staging */
    int alias;                          /* [dropout]: out and delta are the layer's in front, not owned */
    y2h_train_detection dt;             /* [detection] */
    y2h_train_detection_stats *dstats;
    /* [rnn]: its three [connected] sub-layers input / self / output, each with out, delta, x, x_norm over all T*B rows
     * (step-major), mean and variance [T][outputs] and dg the product over all rows; the T+1 state slots of [B][hidden];
     * the per-step bias and scale sums.  out and delta of the [rnn] ARE the output sub-layer's (rnn_layer.c:58-59). */
    struct y2_tlayer *sub;
    float *state, *bias_steps, *scale_steps;
    y2h_train_dense dg_step;            /* the self sub-layer: one step's B rows */
    y2h_train_conv cg;                  /* a sub-layer whose hoisted weight gradient runs as the convolution template at size 1 */
    int dw_conv;
    int step_fwd_ranges, step_dx_ranges;
    int fused;                          /* the self sub-layer's steps run as the fused kernels (rnn_step_form) */
} y2_tlayer;

typedef struct y2_trainer {
    int n, batch;
    y2_tlayer *L;
    float *d_x_nchw, *d_x, *d_truth;    /* the step's input as given, as NHWC, and its truth */
    float *dense_ws;                    /* partial sums of the dense forward / input-gradient ranges */
    float *step_ws;                     /* the fused backward step's partials (y2h_train_rnn_fused_ws_bytes) */
    size_t step_ws_bytes;
    float *dw_tmp;                      /* [inputs][outputs] landing buffer of an [rnn] sub-layer's weight gradient (rnn_dweight) */
    size_t dw_tmp_floats;
    float *ws, *scratch, *stage;        /* weight-gradient partial tiles, reduction partials (and the region head's), NCHW staging
                                           of y2_train_pull and landing buffer of a delta's later writers */
    size_t truth_floats;                /* per step: batch * l.truths of a [region] head, batch * inputs of a [cost] */
    size_t stage_floats;
    float *h_cost, *h_in, *h_pull;      /* pinned: one float per layer; the host batch and truth of y2_train_step; the landing
                                           buffer of every copy down (stage_floats, at least the largest weight array) */
    int dirty;                          /* steps ran since the masters last reached the host arrays */
    /* y2_train_load_detection: descriptor table | truth | packed source pixels, staged in pinned memory and sent up in one
     * copy (both grow-only); d_x and d_truth hold a loaded batch while `loaded` */
    unsigned char *h_load, *d_load;
    size_t h_load_cap, d_load_cap;
    y2h_event ev_load;                  /* recorded behind that copy: the call waits for it before it returns */
    int loaded;
    float load_ms[3];                   /* the last load's host wall time: pack, enqueue (copy + launch), wait for the copy */
} y2_trainer;

/* ------------------------------------------------------------------ */
/* the schedule (parser.c:538-576, network.c:31-79)                    */
/* ------------------------------------------------------------------ */
void y2_lr_parse(list *o, y2_lr_schedule *lr)
{
    char *p = option_find(o, "policy");
    memset(lr, 0, sizeof *lr);
    if (!p) p = "constant";
    lr->policy = !strcmp(p, "random") ? Y2_LR_RANDOM : !strcmp(p, "poly") ? Y2_LR_POLY : !strcmp(p, "step") ? Y2_LR_STEP :
                 !strcmp(p, "exp") ? Y2_LR_EXP : !strcmp(p, "sigmoid") ? Y2_LR_SIG : !strcmp(p, "steps") ? Y2_LR_STEPS : Y2_LR_CONSTANT;
    lr->adam = option_find_int_quiet(o, "adam", 0);
    lr->burn_in = option_find_int_quiet(o, "burn_in", 0);
    lr->step = option_find_int_quiet(o, "step", 1);
    lr->scale = option_find_float_quiet(o, "scale", 1);
    lr->gamma = option_find_float_quiet(o, "gamma", 1);
    lr->power = option_find_float_quiet(o, "power", 1);
    if (lr->policy == Y2_LR_STEPS) {
        char *l = option_find(o, "steps"), *s = option_find(o, "scales");
        int n = 1, i;
        if (!l || !s) return;                       /* the reference exits; the forward path never needed them */
        for (i = 0; l[i]; ++i) if (l[i] == ',') ++n;
        lr->steps = calloc(n, sizeof(int));
        lr->scales = calloc(n, sizeof(float));
        for (i = 0; i < n && l && s; ++i) {
            lr->steps[i] = atoi(l);
            lr->scales[i] = atof(s);
            l = strchr(l, ','); if (l) ++l;
            s = strchr(s, ','); if (s) ++s;
        }
        lr->num_steps = i;
    }
}

/* ------------------------------------------------------------------ */
/* the precision of the convolution products                           */
/* ------------------------------------------------------------------ */
static const char *const precision_names[] = { "fp32", "bf16x3", "bf16" };

int y2_train_precision_env(int *mode)
{
    const char *w = getenv("Y2_TRAIN_PRECISION");
    int k;
    if (!w || !*w) return 0;
    for (k = 0; k < 3; ++k)
        if (!strcmp(w, precision_names[k])) { *mode = k; return 0; }
    y2_fail("Y2_TRAIN_PRECISION=%s: unknown training precision (fp32, bf16x3, bf16)", w);
    return -1;
}

int y2_train_set_precision(network *net, int mode)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) { y2_fail("y2_train_set_precision: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (mode != Y2_TRAIN_FP32 && mode != Y2_TRAIN_BF16X3 && mode != Y2_TRAIN_BF16) {
        y2_fail("y2_train_set_precision: unknown mode %d (Y2_TRAIN_FP32 = 0 fp32, Y2_TRAIN_BF16X3 = 1 bf16x3, Y2_TRAIN_BF16 = 2 bf16)", mode);
        return -1;
    }
    e->train_precision = mode;
    return 0;
}

int y2_train_precision(network *net)
{
    const y2_engine *e = y2_engine_of(net);
    if (!e) { y2_fail("y2_train_precision: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    return e->train_precision;
}

/* the three products of a convolution in the engine's precision; fp32 mode launches what it always launched */
static int planes_of(const y2_engine *e) { return e->train_precision == Y2_TRAIN_BF16X3 ? 3 : 1; }

static int conv_forward(const y2_engine *e, const y2h_train_conv *g, const float *x, const float *w, float *y)
{
    if (e->train_precision == Y2_TRAIN_FP32) return y2h_train_conv_forward(g, x, w, y, e->stream);
    return y2h_train_conv_forward_bf16(g, x, w, y, planes_of(e), e->stream);
}

static int conv_dinput(const y2_engine *e, const y2h_train_conv *g, const float *dy, const float *w, float *dx)
{
    if (e->train_precision == Y2_TRAIN_FP32) return y2h_train_conv_dinput(g, dy, w, dx, e->stream);
    return y2h_train_conv_dinput_bf16(g, dy, w, dx, planes_of(e), e->stream);
}

static int conv_dweight(const y2_engine *e, const y2h_train_conv *g, const float *x, const float *dy, float *dw, float *ws)
{
    if (e->train_precision == Y2_TRAIN_FP32) return y2h_train_conv_dweight(g, x, dy, dw, ws, e->stream);
    return y2h_train_conv_dweight_bf16(g, x, dy, dw, ws, planes_of(e), e->stream);
}

int get_current_batch(network net)
{
    return (*net.seen) / (net.batch * net.subdivisions);
}

float get_current_rate(network net)
{
    const y2_engine *e = y2_engine_of(&net);
    const y2_lr_schedule *s = e ? &e->lr : NULL;
    int batch_num = get_current_batch(net);
    int i;
    float rate;
    if (!s) return net.learning_rate;
    switch (s->policy) {
    case Y2_LR_CONSTANT:
        return net.learning_rate;
    case Y2_LR_STEP:
        return net.learning_rate * pow(s->scale, batch_num / s->step);
    case Y2_LR_STEPS:
        rate = net.learning_rate;
        for (i = 0; i < s->num_steps; ++i) {
            if (s->steps[i] > batch_num) return rate;
            rate *= s->scales[i];
        }
        return rate;
    case Y2_LR_EXP:
        return net.learning_rate * pow(s->gamma, batch_num);
    case Y2_LR_POLY:
        if (batch_num < s->burn_in) return net.learning_rate * pow((float)batch_num / s->burn_in, s->power);
        return net.learning_rate * pow(1 - (float)batch_num / net.max_batches, s->power);
    case Y2_LR_SIG:
        return net.learning_rate * (1. / (1. + exp(s->gamma * (batch_num - s->step))));
    default:
        return net.learning_rate;
    }
}

float get_network_cost(network net)
{
    int i, count = 0;
    float sum = 0;
    for (i = 0; i < net.n; ++i)
        if (net.layers[i].cost) { sum += net.layers[i].cost[0]; ++count; }
    return sum / count;
}

/* ------------------------------------------------------------------ */
/* the weight layout                                                   */
/* ------------------------------------------------------------------ */
void y2_train_pack_weights(const float *ref, float *packed, int n, int c, int size)
{
    int f, ci, ky, kx;
    for (f = 0; f < n; ++f)
        for (ci = 0; ci < c; ++ci)
            for (ky = 0; ky < size; ++ky)
                for (kx = 0; kx < size; ++kx)
                    packed[((size_t)(ky * size + kx) * c + ci) * n + f] = ref[(((size_t)f * c + ci) * size + ky) * size + kx];
}

void y2_train_unpack_weights(const float *packed, float *ref, int n, int c, int size)
{
    int f, ci, ky, kx;
    for (f = 0; f < n; ++f)
        for (ci = 0; ci < c; ++ci)
            for (ky = 0; ky < size; ++ky)
                for (kx = 0; kx < size; ++kx)
                    ref[(((size_t)f * c + ci) * size + ky) * size + kx] = packed[((size_t)(ky * size + kx) * c + ci) * n + f];
}

/* A dense layer's master is [outputs][inputs] like the host's; behind an image (h * w > 1) the reference's input index is
 * ci*h*w + y*w + x and the trainer's activation is dense NHWC, so the K index of the master runs (y, x, ci). */
void y2_train_pack_dense_weights(const float *ref, float *packed, int outputs, int c, int h, int w)
{
    const size_t k = (size_t)c * h * w;
    int o, ci, p;
    for (o = 0; o < outputs; ++o)
        for (ci = 0; ci < c; ++ci)
            for (p = 0; p < h * w; ++p)
                packed[o * k + (size_t)p * c + ci] = ref[o * k + (size_t)ci * h * w + p];
}

void y2_train_unpack_dense_weights(const float *packed, float *ref, int outputs, int c, int h, int w)
{
    const size_t k = (size_t)c * h * w;
    int o, ci, p;
    for (o = 0; o < outputs; ++o)
        for (ci = 0; ci < c; ++ci)
            for (p = 0; p < h * w; ++p)
                ref[o * k + (size_t)ci * h * w + p] = packed[o * k + (size_t)p * c + ci];
}

/* ------------------------------------------------------------------ */
/* refusals                                                            */
/* ------------------------------------------------------------------ */
/* an [rnn]: what backward_rnn_layer's CPU branch can be followed through */
static int refuse_rnn(const network *net, int i)
{
    const layer *l = &net->layers[i];
    const layer *subs[3] = { l->input_layer, l->self_layer, l->output_layer };
    int k;
    if (i + 1 >= net->n || (net->layers[i + 1].type != RNN && net->layers[i + 1].type != CONNECTED)) {
        y2_fail("training: layer %d (rnn): a recurrent layer must feed an [rnn] or a [connected] layer", i);
        return -1;
    }
    /* the parser already refuses an [rnn] behind an image (y2_cfg.c flat_before): this guards a network whose layer fields were
     * set by hand.  The input sub-layer's weights are in the reference's column order, an image is ordered by pixel here. */
    if (i == 0 ? (net->h > 0 && net->w > 0 && net->c > 1 && net->h * net->w > 1)
               : (net->layers[i - 1].out_h * net->layers[i - 1].out_w > 1 && net->layers[i - 1].out_c > 1)) {
        y2_fail("training: layer %d (rnn): a recurrent layer needs a flat input (inputs= in the [net], or a dense layer in front), not an image", i);
        return -1;
    }
    if (l->shortcut) {
        y2_fail("training: layer %d (rnn): shortcut=1 is not trainable (the reference's backward reads a state its forward did not produce)", i);
        return -1;
    }
    if (l->self_layer->activation == LOGGY) { y2_fail("training: layer %d (rnn): logistic=2 (loggy) is not trainable", i); return -1; }
    for (k = 0; k < 3; ++k) {
        const ACTIVATION a = subs[k]->activation;
        if (a != LINEAR && a != LEAKY && a != LOGISTIC && a != RELU) {
            y2_fail("training: layer %d (rnn): activation %d is not trainable (linear, leaky, logistic, relu)", i, (int)a);
            return -1;
        }
    }
    if (l->batch_normalize && l->batch < 2) {
        y2_fail("training: layer %d (rnn): batch normalisation over batch / time_steps = %d value divides by zero in the reference", i, l->batch);
        return -1;
    }
    return 0;
}

static int refuse(const network *net)
{
    const y2_engine *e = y2_engine_of(net);
    int i, flat = 0;           /* the running activation reads the same as [batch][c][h][w] and as [batch][h][w][c] */
    int det;                   /* the network ends in [detection]: [connected] and [dropout] train */
    int rnn = 0;               /* the network holds an [rnn]: [connected] trains */
    if (!e || !net->layers || net->n <= 0) { y2_fail("y2_train_prepare: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (e->half) { y2_fail("training is fp32 only: the network is in fp16 mode (y2_set_half / Y2_FP16)"); return -1; }
    if (e->lr.adam) { y2_fail("training: adam=1 is not implemented (SGD with momentum only)"); return -1; }
    if (e->lr.policy == Y2_LR_RANDOM) { y2_fail("training: policy=random is refused (its rate is a draw of rand(), not a function of the step)"); return -1; }
    if (e->lr.policy == Y2_LR_STEPS && !e->lr.num_steps) { y2_fail("training: STEPS policy must have steps and scales in cfg file"); return -1; }
    det = net->layers[net->n - 1].type == DETECTION;
    for (i = 0; i < net->n; ++i) rnn |= net->layers[i].type == RNN;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const char *t = get_layer_string(l->type);
        if (l->type == GRU) {
            y2_fail("training: layer %d (%s): a [gru] layer cannot be trained (the reference's backward_gru_layer is empty: there is no gradient to follow)", i, t);
            return -1;
        }
        if (l->type == RNN && refuse_rnn(net, i) != 0) return -1;
        if ((l->type == SOFTMAX || l->type == COST) && !flat) {
            y2_fail("training: layer %d (%s): its input must be one value per channel (put an [avgpool] in front): rows of an "
                    "image are ordered by channel in the truth and by pixel on the device", i, t);
            return -1;
        }
        if (l->type == DETECTION && !flat) {
            y2_fail("training: layer %d (%s): its input must be one value per channel (put a [connected] in front): the head reads "
                    "rows ordered by channel, an image is ordered by pixel on the device", i, t);
            return -1;
        }
        if (l->type == CONVOLUTIONAL || l->type == MAXPOOL) flat = l->out_h * l->out_w == 1 || l->out_c == 1;
        if (l->type == AVGPOOL || l->type == CONNECTED || l->type == RNN) flat = 1;
        if (l->type == ROUTE || l->type == REORG || l->type == REGION) flat = 0;
        if ((l->type == ROUTE || l->type == REORG) && net->layers[net->n - 1].type != REGION) {
            y2_fail("training: layer %d (%s) trains only in a network that ends in [region]", i, t);
            return -1;
        }
        if ((l->type == CONNECTED || l->type == DROPOUT) && !det && !(rnn && l->type == CONNECTED)) {
            y2_fail("training: layer %d (%s) trains only in a network that ends in [detection]", i, t);
            return -1;
        }
        switch (l->type) {
        case CONVOLUTIONAL:
            if (l->stride != 1) { y2_fail("training: layer %d (%s): stride %d is not trainable (stride 1 only)", i, t, l->stride); return -1; }
            if (l->xnor || l->binary) { y2_fail("training: layer %d (%s): xnor / binary weights are not trainable", i, t); return -1; }
            if (l->activation != LINEAR && l->activation != LEAKY && l->activation != LOGISTIC && l->activation != RELU) {
                y2_fail("training: layer %d (%s): activation %d is not trainable (linear, leaky, logistic, relu)", i, t, (int)l->activation);
                return -1;
            }
            if (l->batch_normalize && (long)net->batch * l->out_h * l->out_w < 2) {
                y2_fail("training: layer %d (%s): batch normalisation over batch*out_h*out_w = %ld value divides by zero in the reference",
                        i, t, (long)net->batch * l->out_h * l->out_w);
                return -1;
            }
            break;
        case MAXPOOL: case AVGPOOL:
            break;
        case SOFTMAX:
            if (l->softmax_tree || l->groups > 1) { y2_fail("training: layer %d (%s): a tree or groups > 1 softmax is not trainable", i, t); return -1; }
            break;
        case COST:
            if (l->cost_type != SSE) { y2_fail("training: layer %d (%s): only type=sse is trainable", i, t); return -1; }
            if (i == 0) { y2_fail("training: layer %d (%s): a cost layer needs a layer in front of it", i, t); return -1; }
            if (i != net->n - 1) { y2_fail("training: layer %d (%s): only the last layer may be a cost layer (one truth per step)", i, t); return -1; }
            break;
        case ROUTE:
            if (l->n <= 0 || l->out_h <= 0 || l->out_w <= 0) { y2_fail("training: layer %d (%s): its sources must have one spatial size", i, t); return -1; }
            break;
        case REORG:
            if (l->reverse) { y2_fail("training: layer %d (%s): reverse=1 is not trainable", i, t); return -1; }
            if (i == 0 || l->stride <= 0 || l->h % l->stride || l->w % l->stride || l->c % (l->stride * l->stride)) {
                y2_fail("training: layer %d (%s): %d x %d x %d does not divide by stride %d", i, t, l->w, l->h, l->c, l->stride);
                return -1;
            }
            break;
        case REGION:
            if (l->softmax_tree || l->map) { y2_fail("training: layer %d (%s): tree= / map= is not trainable", i, t); return -1; }
            if (l->classfix != 0) { y2_fail("training: layer %d (%s): classfix=%d is not trainable (0 only)", i, t, l->classfix); return -1; }
            if (l->softmax != 1) { y2_fail("training: layer %d (%s): only softmax=1 is trainable", i, t); return -1; }
            if (i != net->n - 1) { y2_fail("training: layer %d (%s): only the last layer may be a region layer (one truth per step)", i, t); return -1; }
            if (i == 0 || l->classes <= 0 || net->layers[i - 1].out_h != l->h || net->layers[i - 1].out_w != l->w ||
                net->layers[i - 1].out_c != l->n * (5 + l->classes)) {
                y2_fail("training: layer %d (%s): the layer in front must give %d channels on the %d x %d grid", i, t, l->n * (5 + l->classes), l->w, l->h);
                return -1;
            }
            break;
        case CONNECTED:
            if (l->activation != LINEAR && l->activation != LEAKY && l->activation != LOGISTIC && l->activation != RELU) {
                y2_fail("training: layer %d (%s): activation %d is not trainable (linear, leaky, logistic, relu)", i, t, (int)l->activation);
                return -1;
            }
            if (l->batch_normalize && net->batch < 2) {
                y2_fail("training: layer %d (%s): batch normalisation over batch = %d value divides by zero in the reference", i, t, net->batch);
                return -1;
            }
            break;
        case DROPOUT:
            if (i == 0) { y2_fail("training: layer %d (%s): a dropout layer needs a layer in front of it", i, t); return -1; }
            break;
        case RNN:           /* refuse_rnn above */
            break;
        case DETECTION:
            if (l->random) {
                y2_fail("training: layer %d (%s): random=1 is refused (it picks the box by a draw of rand() inside the loss while seen < 64000)", i, t);
                return -1;
            }
            if (i != net->n - 1) { y2_fail("training: layer %d (%s): only the last layer may be a detection layer (one truth per step)", i, t); return -1; }
            if (l->coords != 4) { y2_fail("training: layer %d (%s): coords=%d is not trainable (4 only)", i, t, l->coords); return -1; }
            /* the parser already refuses a cfg whose count differs (y2_cfg.c make_detection): this guards a network whose
             * layer fields were set by hand */
            if (i == 0 || l->side <= 0 || l->n <= 0 || l->classes <= 0 ||
                net->layers[i - 1].outputs != l->side * l->side * ((1 + l->coords) * l->n + l->classes)) {
                y2_fail("training: layer %d (%s): the layer in front must give side*side*((1+coords)*num+classes) = %d values", i, t,
                        l->side * l->side * ((1 + l->coords) * l->n + l->classes));
                return -1;
            }
            break;
        default:
            y2_fail("training: layer %d (%s) is not trainable (convolutional, maxpool, avgpool, softmax, cost, route, reorg, region; "
                    "connected, dropout, detection in a network that ends in [detection]; rnn, and connected behind it)", i, t);
            return -1;
        }
    }
    if ((net->h <= 0 || net->w <= 0 || net->c <= 0) && !(net->layers[0].type == RNN && net->inputs > 0)) { y2_fail("training: the network input must be an image (h, w, c > 0)"); return -1; }
    if (net->layers[net->n - 1].type != COST && net->layers[net->n - 1].type != REGION && !det) {
        y2_fail("training: layer %d (%s): the last layer must be [cost], [region] or [detection]", net->n - 1, get_layer_string(net->layers[net->n - 1].type));
        return -1;
    }
    return 0;
}

static int truths_per_image(const network *net)
{
    const layer *last = &net->layers[net->n - 1];
    return last->type == REGION || last->type == DETECTION ? last->truths : last->inputs;
}

int y2_train_truth_floats(network *net)
{
    if (!net || refuse(net) != 0) return -1;
    return truths_per_image(net);
}

/* ------------------------------------------------------------------ */
/* lifecycle                                                           */
/* ------------------------------------------------------------------ */
void y2_train_free(network *net)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e ? e->trainer : NULL;
    int i;
    if (!t) return;
    y2h_set_device(e->device);
    if (e->stream) y2h_stream_sync(e->stream);
    for (i = 0; i < t->n; ++i) {
        y2_tlayer *L = &t->L[i];
        float *all[] = { L->out, L->delta, L->x, L->x_norm, L->mean, L->variance, L->mean_delta, L->variance_delta, L->weights,
                         L->weight_updates, L->biases, L->bias_updates, L->scales, L->scale_updates, L->rolling_mean,
                         L->rolling_variance, L->cost };
        size_t k;
        int m;
        for (m = 0; L->sub && m < 3; ++m) {
            y2_tlayer *S = &L->sub[m];
            float *mine[] = { S->out, S->delta, S->x, S->x_norm, S->mean, S->variance, S->mean_delta, S->variance_delta, S->weights,
                              S->weight_updates, S->biases, S->bias_updates, S->scales, S->scale_updates, S->rolling_mean,
                              S->rolling_variance };
            for (k = 0; k < sizeof mine / sizeof mine[0]; ++k) y2h_free(mine[k]);
        }
        y2h_free(L->state); y2h_free(L->bias_steps); y2h_free(L->scale_steps);
        for (k = L->alias || L->sub ? 2 : 0; k < sizeof all / sizeof all[0]; ++k) y2h_free(all[k]);
        free(L->sub);
        y2h_free(L->idx);
        y2h_free(L->stats);
        y2h_free(L->dstats);
        y2h_free(L->rnd);
        y2h_host_free(L->h_rnd);
        free(L->src_add);
    }
    y2h_free(t->d_x_nchw); y2h_free(t->d_x); y2h_free(t->d_truth);
    y2h_free(t->dw_tmp); y2h_free(t->step_ws);
    y2h_free(t->ws); y2h_free(t->scratch); y2h_free(t->stage); y2h_free(t->dense_ws);
    y2h_host_free(t->h_cost); y2h_host_free(t->h_in); y2h_host_free(t->h_pull);
    y2h_host_free(t->h_load); y2h_free(t->d_load);
    if (t->ev_load) y2h_event_destroy(t->ev_load);
    free(t->L);
    free(t);
    e->trainer = NULL;
}

static int dev_floats(float **p, size_t n, y2_engine *e)
{
    HIP_OR_ERR(y2h_malloc((void **)p, (n ? n : 1) * sizeof(float)));
    HIP_OR_ERR(y2h_memset(*p, 0, (n ? n : 1) * sizeof(float), e->stream));
    return 0;
}

static int push(float *dst, const float *src, size_t n, float *pinned, y2_engine *e)
{
    memcpy(pinned, src, n * sizeof(float));
    HIP_OR_ERR(y2h_memcpy_h2d(dst, pinned, n * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* a [cost] over this many values or more sums in chunks (y2h_train_cost_sse_chunked); every network below it -- a classifier's
 * batch x classes -- launches what it launched */
#define COST_CHUNKED_FROM (1L << 20)

static size_t max_z(size_t a, size_t b) { return a > b ? a : b; }

/* the reference's backward order (network.c:204-223), walked once: who finds a delta already written */
static void plan_deltas(const network *net, y2_trainer *t)
{
    int *written = calloc(net->n, sizeof(int));
    int i, k;
    for (i = net->n - 1; i >= 0; --i) {
        const layer *l = &net->layers[i];
        y2_tlayer *L = &t->L[i];
        if (l->type == ROUTE) {
            L->src_add = calloc(l->n, sizeof(int));
            for (k = 0; k < l->n; ++k) { L->src_add[k] = written[l->input_layers[k]]; written[l->input_layers[k]] = 1; }
        } else if (l->type == DROPOUT) {
            if (i > 0) written[i - 1] = written[i];                    /* neither stores nor adds: its delta IS the one in front */
        } else if (i > 0) {
            L->din_add = l->type == REORG ? 0 : written[i - 1];        /* reorg_layer.c:92 assigns */
            written[i - 1] = 1;
        }
    }
    free(written);
}

/* ------------------------------------------------------------------ */
/* [rnn]: back-propagation through time (rnn_layer.c:83-172) */
/* ------------------------------------------------------------------ */
static const layer *rnn_sub(const layer *l, int k) { return k == 0 ? l->input_layer : k == 1 ? l->self_layer : l->output_layer; }

/* the bytes prepare_rnn is about to ask for, summed before the first of them is.  The sum decides nothing: the runtime layer
 * has no query for free memory, so an allocation that fails is what stops y2_train_prepare, and the figure (a double: no
 * overflow at any shape) is there for its message, which names the layer and the figure and so tells the caller what to
 * shrink. */
static double rnn_device_bytes(const network *net)
{
    double floats = 0;
    int i, k;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const double rows = (double)l->steps * l->batch;
        if (l->type != RNN) continue;
        floats += (rows + l->batch) * l->hidden + 2. * l->steps * (l->hidden > l->outputs ? l->hidden : l->outputs);
        for (k = 0; k < 3; ++k) {
            const layer *s = rnn_sub(l, k);
            floats += rows * s->outputs * (s->batch_normalize ? 4 : 2) + 2. * s->outputs * s->inputs + 2. * s->outputs;
            if (s->batch_normalize) floats += (2. * l->steps + 6) * s->outputs;
        }
    }
    return floats * sizeof(float);
}

/* Which kernels make a hoisted weight gradient over `rows` = T*B rows.  y2h_train_dense_dweight is laid out around few rows
 * and walks all of them in one wave per 32 x 32 tile of the gradient; the convolution template at size 1 splits the rows.
 * Measured: at 73 728 rows the template takes 3.01 ms against 4.87 (1024 inputs) and 0.81 against 4.71 (256), at
 * 128 rows 0.021 against 0.015.  The crossing was not looked for: the template from 8192 rows on.  The template writes
 * [inputs][outputs], so its result lands in a buffer of its own and is added transposed.
 * Y2_RNN_TRAIN_DWEIGHT=dense|conv forces one at prepare time (tests). */
#define RNN_DWEIGHT_CONV_FROM 8192
/* Measured in alternating processes: the fused form LOSES, 251.3 ms a step against 164.0 at 128 x 576 and 11.0
 * against 8.2 at 16 x 64 -- its hidden / 32 workgroups leave 224 of 256 CUs idle while the dense product spreads a step over
 * K ranges -- so the rule chooses the composed form everywhere and the fused one runs only when forced. */
#define RNN_STEP_DEFAULT_FUSED 0

static int rnn_dweight_by_conv(long rows, int *by_conv)
{
    const char *f = getenv("Y2_RNN_TRAIN_DWEIGHT");
    *by_conv = rows >= RNN_DWEIGHT_CONV_FROM;
    if (!f || !*f) return 0;
    if (!strcmp(f, "dense")) *by_conv = 0;
    else if (!strcmp(f, "conv")) *by_conv = 1;
    else { y2_fail("Y2_RNN_TRAIN_DWEIGHT=%s: unknown form (dense, conv)", f); return -1; }
    return 0;
}

/* The form of the self sub-layer's steps.  The rule is y2h_train_rnn_fused_fits (B <= 128 rows, LDS, the partials' bytes);
 * what fits takes RNN_STEP_DEFAULT_FUSED's form, everything else the composed one.  Y2_RNN_TRAIN_STEP=composed|fused forces a
 * form at prepare time (tests); a forced fused form that does not fit is refused. */
static int rnn_step_form(int i, int B, int hidden, int *fused)
{
    const char *f = getenv("Y2_RNN_TRAIN_STEP");
    const int fits = y2h_train_rnn_fused_fits(B, hidden);
    *fused = fits && RNN_STEP_DEFAULT_FUSED;
    if (!f || !*f) return 0;
    if (!strcmp(f, "composed")) *fused = 0;
    else if (!strcmp(f, "fused")) {
        if (!fits) {
            y2_fail("training: layer %d (rnn): Y2_RNN_TRAIN_STEP=fused, but %d sequences of %d values do not fit the fused step kernels "
                    "(at most 128 rows; partial sums within 256 MiB)", i, B, hidden);
            return -1;
        }
        *fused = 1;
    } else { y2_fail("Y2_RNN_TRAIN_STEP=%s: unknown form (composed, fused)", f); return -1; }
    return 0;
}

static int rnn_dweight(y2_tlayer *S, const float *x, y2_trainer *t, y2_engine *e)
{
    const size_t nw = (size_t)S->dg.inputs * S->dg.outputs;
    if (!S->dw_conv) { HIP_OR_ERR(y2h_train_dense_dweight(&S->dg, x, S->delta, S->weight_updates, e->stream)); return 0; }
    HIP_OR_ERR(y2h_memset(t->dw_tmp, 0, nw * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_train_conv_dweight(&S->cg, x, S->delta, t->dw_tmp, t->ws, e->stream));
    HIP_OR_ERR(y2h_train_rnn_add_transposed(S->weight_updates, t->dw_tmp, S->dg.outputs, S->dg.inputs, e->stream));
    return 0;
}

static int prepare_rnn(network *net, int i, y2_trainer *t, y2_engine *e, float *pin, size_t *dense_ws, size_t *ws)
{
    const layer *l = &net->layers[i];
    y2_tlayer *L = &t->L[i];
    const int T = l->steps, B = l->batch, wide = l->hidden > l->outputs ? l->hidden : l->outputs;
    int k;
    if (!(L->sub = calloc(3, sizeof *L->sub))) { y2_fail("out of memory"); return -1; }
    if (rnn_step_form(i, B, l->hidden, &L->fused) != 0) return -1;
    if (L->fused) t->step_ws_bytes = max_z(t->step_ws_bytes, y2h_train_rnn_fused_ws_bytes(B, l->hidden));
    if (dev_floats(&L->state, (size_t)(T + 1) * B * l->hidden, e) || dev_floats(&L->bias_steps, (size_t)T * wide, e) ||
        dev_floats(&L->scale_steps, (size_t)T * wide, e)) return -1;
    for (k = 0; k < 3; ++k) {
        const layer *s = rnn_sub(l, k);
        y2_tlayer *S = &L->sub[k];
        const size_t outs = (size_t)T * B * s->outputs, nw = (size_t)s->outputs * s->inputs, n = s->outputs;
        y2h_train_dense dg = { T * B, s->inputs, s->outputs }, step = { B, s->inputs, s->outputs };
        size_t fw = 0, bw = 0, sfw = 0, sbw = 0;
        S->dg = dg;
        if (y2h_train_dense_plan(&dg, Y2H_DENSE_FORWARD, 0, &S->fwd_ranges, &fw, NULL, 0) != 0 ||
            y2h_train_dense_plan(&dg, Y2H_DENSE_DINPUT, 0, &S->dx_ranges, &bw, NULL, 0) != 0 ||
            (k == 1 && (y2h_train_dense_plan(&step, Y2H_DENSE_FORWARD, 0, &L->step_fwd_ranges, &sfw, NULL, 0) != 0 ||
                        y2h_train_dense_plan(&step, Y2H_DENSE_DINPUT, 0, &L->step_dx_ranges, &sbw, NULL, 0) != 0))) {
            y2_fail("training: layer %d (rnn): shape outside what the kernels take", i);
            return -1;
        }
        if (k == 1) L->dg_step = step;
        if (rnn_dweight_by_conv((long)T * B, &S->dw_conv) != 0) return -1;
        if (S->dw_conv) {
            y2h_train_conv cg = { T * B, 1, 1, s->inputs, s->outputs, 1, 0, 1, 1 };
            S->cg = cg;
            if (y2h_train_dweight_ws_bytes(&cg) == 0) { y2_fail("training: layer %d (rnn): shape outside what the kernels take", i); return -1; }
            *ws = max_z(*ws, y2h_train_dweight_ws_bytes(&cg));
            t->dw_tmp_floats = max_z(t->dw_tmp_floats, nw);
        }
        *dense_ws = max_z(*dense_ws, max_z(max_z(fw, bw), max_z(sfw, sbw)));
        if (dev_floats(&S->out, outs, e) || dev_floats(&S->delta, outs, e) || dev_floats(&S->weights, nw, e) ||
            dev_floats(&S->weight_updates, nw, e) || dev_floats(&S->biases, n, e) || dev_floats(&S->bias_updates, n, e) ||
            push(S->weights, s->weights, nw, pin, e) || push(S->biases, s->biases, n, pin, e)) return -1;
        if (!s->batch_normalize) continue;
        if (dev_floats(&S->x, outs, e) || dev_floats(&S->x_norm, outs, e) || dev_floats(&S->mean, (size_t)T * n, e) ||
            dev_floats(&S->variance, (size_t)T * n, e) || dev_floats(&S->mean_delta, n, e) || dev_floats(&S->variance_delta, n, e) ||
            dev_floats(&S->scales, n, e) || dev_floats(&S->scale_updates, n, e) || dev_floats(&S->rolling_mean, n, e) ||
            dev_floats(&S->rolling_variance, n, e) || push(S->scales, s->scales, n, pin, e) ||
            push(S->rolling_mean, s->rolling_mean, n, pin, e) || push(S->rolling_variance, s->rolling_variance, n, pin, e)) return -1;
    }
    L->out = L->sub[2].out;             /* rnn_layer.c:58-59 */
    L->delta = L->sub[2].delta;
    return 0;
}

/* forward_connected_layer behind its product, on `groups` steps of B rows from step t0: each step normalises over its own
 * rows and moves the rolling statistics once, in step order */
static int rnn_sub_forward(const layer *s, y2_tlayer *S, int t0, int groups, int B, y2_engine *e)
{
    const size_t n = s->outputs, off = (size_t)t0 * B * n;
    if (!s->batch_normalize)
        return y2h_train_bn_apply(S->out + off, NULL, NULL, NULL, NULL, NULL, S->biases, y2_act_code(s->activation), (long)groups * B, s->outputs, e->stream);
    HIP_OR_ERR(y2h_train_rnn_bn_stats(S->out + off, groups, B, s->outputs, S->mean + t0 * n, S->variance + t0 * n, S->rolling_mean,
                                      S->rolling_variance, .95f, .05f, e->stream));
    HIP_OR_ERR(y2h_train_rnn_bn_apply(S->out + off, S->x + off, S->x_norm + off, S->mean + t0 * n, S->variance + t0 * n, S->scales, S->biases,
                                      y2_act_code(s->activation), groups, B, s->outputs, e->stream));
    return 0;
}

/* backward_connected_layer in front of its products, on `groups` steps from step t0, the steps' bias and scale sums into
 * slots t0.. of the layer's [T][n] buffers.  increment_layer does not advance mean and variance: every step's backward
 * reads the LAST step's statistics with its own x and x_norm, as the compiled reference does. */
static int rnn_sub_delta(const layer *s, y2_tlayer *S, y2_tlayer *L, int t0, int groups, int T, int B, y2_engine *e)
{
    const size_t n = s->outputs, off = (size_t)t0 * B * n, last = (size_t)(T - 1) * n;
    const int bn = s->batch_normalize;
    HIP_OR_ERR(y2h_train_rnn_delta(S->out + off, S->delta + off, bn ? S->x + off : NULL, bn ? S->x_norm + off : NULL, S->scales,
                                   bn ? S->mean + last : NULL, bn ? S->variance + last : NULL, y2_act_code(s->activation), groups, B,
                                   s->outputs, L->bias_steps + t0 * n, L->scale_steps + t0 * n, S->mean_delta, S->variance_delta, e->stream));
    return 0;
}

/* the T per-step sums, added to the update buffers last step first: the order in which the reference's loop meets them */
static int rnn_sub_sums(const layer *s, y2_tlayer *S, y2_tlayer *L, int T, y2_engine *e)
{
    HIP_OR_ERR(y2h_train_rnn_sum_steps(L->bias_steps, T, s->outputs, S->bias_updates, e->stream));
    if (s->batch_normalize) HIP_OR_ERR(y2h_train_rnn_sum_steps(L->scale_steps, T, s->outputs, S->scale_updates, e->stream));
    return 0;
}

/* THE COPY POINT (rnn_layer.c:161): input.delta[t] is self.delta[t] as the self sub-layer's backward LEFT it, its activation
 * gradient and batch-norm backward applied in place -- the compiled CPU path, the project's parity.  The reference's GPU twin
 * copies before that backward (rnn_layer.c:258), which is the true gradient; the two differ whenever the self sub-layer is
 * not a plain linear one.  Every self.delta[t] is final once the chain has passed t, so all T copies are one. */
static int rnn_copy_point(const layer *l, y2_tlayer *L, y2_engine *e)
{
    HIP_OR_ERR(y2h_memcpy_d2d(L->sub[0].delta, L->sub[1].delta, (size_t)l->steps * l->batch * l->hidden * sizeof(float), e->stream));
    return 0;
}

static int forward_rnn(const layer *l, y2_tlayer *L, const float *in, y2_trainer *t, y2_engine *e)
{
    const int T = l->steps, B = l->batch;
    const size_t bh = (size_t)B * l->hidden;
    y2_tlayer *S0 = &L->sub[0], *S1 = &L->sub[1], *S2 = &L->sub[2];
    int k;
    /* state.train: slot 0 is zero at every step.  No delta is zeroed: each of the three has a first writer that stores */
    HIP_OR_ERR(y2h_memset(L->state, 0, bh * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_train_dense_forward(&S0->dg, in, S0->weights, S0->out, t->dense_ws, S0->fwd_ranges, e->stream));
    if (rnn_sub_forward(l->input_layer, S0, 0, T, B, e) != 0) return -1;
    for (k = 0; k < T; ++k) {           /* step k reads slot k and writes slot k + 1 */
        const int bn = l->self_layer->batch_normalize;
        const size_t h = l->hidden;
        if (L->fused) {         /* the product on the matrix cores and all of the below: one launch */
            HIP_OR_ERR(y2h_train_rnn_fused_forward(L->state + k * bh, S1->weights, S1->out + k * bh, bn ? S1->x + k * bh : NULL,
                                                   bn ? S1->x_norm + k * bh : NULL, bn ? S1->mean + k * h : NULL,
                                                   bn ? S1->variance + k * h : NULL, S1->rolling_mean, S1->rolling_variance, .95f, .05f,
                                                   S1->scales, S1->biases, y2_act_code(l->self_layer->activation), B, l->hidden,
                                                   S0->out + k * bh, L->state + (k + 1) * bh, e->stream));
            continue;
        }
        HIP_OR_ERR(y2h_train_dense_forward(&L->dg_step, L->state + k * bh, S1->weights, S1->out + k * bh, t->dense_ws, L->step_fwd_ranges, e->stream));
        /* statistics over the step's own rows, the rolling update, apply and the combine into slot k + 1: one launch */
        HIP_OR_ERR(y2h_train_rnn_step_finish(S1->out + k * bh, bn ? S1->x + k * bh : NULL, bn ? S1->x_norm + k * bh : NULL,
                                             bn ? S1->mean + k * h : NULL, bn ? S1->variance + k * h : NULL, S1->rolling_mean,
                                             S1->rolling_variance, .95f, .05f, S1->scales, S1->biases, y2_act_code(l->self_layer->activation),
                                             B, l->hidden, S0->out + k * bh, L->state + (k + 1) * bh, e->stream));
    }
    HIP_OR_ERR(y2h_train_dense_forward(&S2->dg, L->state + bh, S2->weights, S2->out, t->dense_ws, S2->fwd_ranges, e->stream));
    return rnn_sub_forward(l->output_layer, S2, 0, T, B, e);
}

/* in: the layer's input rows; din: where its input gradient is stored (NULL: layer 0) */
static int backward_rnn(const layer *l, y2_tlayer *L, const float *in, float *din, y2_trainer *t, y2_engine *e)
{
    const int T = l->steps, B = l->batch;
    const size_t bh = (size_t)B * l->hidden;
    y2_tlayer *S0 = &L->sub[0], *S1 = &L->sub[1], *S2 = &L->sub[2];
    int k;
    /* the output sub-layer, all steps at once; its input is slots 1..T, its input gradient the first writer of self.delta */
    if (rnn_sub_delta(l->output_layer, S2, L, 0, T, T, B, e) != 0 || rnn_sub_sums(l->output_layer, S2, L, T, e) != 0) return -1;
    if (rnn_dweight(S2, L->state + bh, t, e) != 0) return -1;
    HIP_OR_ERR(y2h_train_dense_dinput(&S2->dg, S2->delta, S2->weights, S1->delta, 0, t->dense_ws, S2->dx_ranges, e->stream));
    /* the self sub-layer's delta chain, last step first; step 0 has no input gradient */
    for (k = T - 1; k >= 0; --k) {
        if (L->fused) {         /* the delta work and the partial products in one launch, the range-order sum in a second */
            const layer *s = l->self_layer;
            const size_t n = l->hidden, last = (size_t)(T - 1) * n;
            const int bn = s->batch_normalize;
            HIP_OR_ERR(y2h_train_rnn_fused_backward(S1->out + k * bh, S1->delta + k * bh, bn ? S1->x + k * bh : NULL,
                                                    bn ? S1->x_norm + k * bh : NULL, S1->scales, bn ? S1->mean + last : NULL,
                                                    bn ? S1->variance + last : NULL, y2_act_code(s->activation), B, l->hidden, S1->weights,
                                                    L->bias_steps + k * n, L->scale_steps + k * n, S1->mean_delta, S1->variance_delta,
                                                    k > 0 ? S1->delta + (k - 1) * bh : NULL, t->step_ws, e->stream));
            continue;
        }
        if (rnn_sub_delta(l->self_layer, S1, L, k, 1, T, B, e) != 0) return -1;
        if (k > 0) HIP_OR_ERR(y2h_train_dense_dinput(&L->dg_step, S1->delta + k * bh, S1->weights, S1->delta + (k - 1) * bh, 1, t->dense_ws,
                                                     L->step_dx_ranges, e->stream));
    }
    if (rnn_sub_sums(l->self_layer, S1, L, T, e) != 0) return -1;
    if (rnn_dweight(S1, L->state, t, e) != 0) return -1;        /* its input is slots 0..T-1 */
    if (rnn_copy_point(l, L, e) != 0) return -1;
    /* the input sub-layer, all steps at once */
    if (rnn_sub_delta(l->input_layer, S0, L, 0, T, T, B, e) != 0 || rnn_sub_sums(l->input_layer, S0, L, T, e) != 0) return -1;
    if (rnn_dweight(S0, in, t, e) != 0) return -1;
    if (din) HIP_OR_ERR(y2h_train_dense_dinput(&S0->dg, S0->delta, S0->weights, din, 0, t->dense_ws, S0->dx_ranges, e->stream));
    return 0;
}

int y2_train_prepare(network *net)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t;
    float *pin, *tmp = NULL;
    size_t ws = 16, scratch = 16, dense_ws = 16, stage;
    double rnn_bytes;
    int i, rc = -1;
    if (refuse(net) != 0) return -1;
    y2_train_free(net);
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!e->stream) HIP_OR_ERR(y2h_stream_create(&e->stream));
    t = calloc(1, sizeof *t);
    t->n = net->n; t->batch = net->batch;
    t->L = calloc(net->n, sizeof *t->L);
    t->truth_floats = (size_t)net->batch * truths_per_image(net);
    e->trainer = t;
    plan_deltas(net, t);
    stage = max_z((size_t)net->batch * net->inputs, t->truth_floats);       /* y2_train_pull_input lands the truth there */
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        stage = max_z(stage, (size_t)net->batch * l->outputs);
        if (l->type == RNN) {       /* a sub-layer's rows, its weights, the state history */
            stage = max_z(stage, (size_t)(net->batch + l->batch) * l->hidden);
            stage = max_z(stage, (size_t)l->hidden * (size_t)(l->hidden > l->inputs ? l->hidden : l->inputs));
            stage = max_z(stage, (size_t)l->hidden * l->outputs);
        }
        if (l->type == CONVOLUTIONAL || l->type == CONNECTED) stage = max_z(stage, (size_t)l->n * l->c * l->size * l->size);
    }
    t->stage_floats = stage;
    rnn_bytes = rnn_device_bytes(net);
    if (y2h_host_alloc((void **)&t->h_pull, stage * sizeof(float)) != 0) { y2_fail("y2_train_prepare: no pinned memory: %s", y2h_last_error()); goto cleanup; }
    pin = t->h_pull;
    tmp = malloc(stage * sizeof(float));
    HIP_OR_CLEANUP(y2h_host_alloc((void **)&t->h_cost, (size_t)net->n * sizeof(float)));
    HIP_OR_CLEANUP(y2h_host_alloc((void **)&t->h_in, ((size_t)net->batch * net->inputs + t->truth_floats) * sizeof(float)));
    if (dev_floats(&t->d_x_nchw, (size_t)net->batch * net->inputs, e) || dev_floats(&t->d_x, (size_t)net->batch * net->inputs, e) ||
        dev_floats(&t->d_truth, t->truth_floats, e)) goto cleanup;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        y2_tlayer *L = &t->L[i];
        const size_t outs = (size_t)net->batch * l->outputs;
        if (l->type == CONNECTED || l->type == DROPOUT) {       /* the activation in front, seen through any [dropout] */
            int p = i - 1;
            while (p >= 0 && net->layers[p].type == DROPOUT) --p;
            L->src_c = p < 0 ? net->c : net->layers[p].out_c;
            L->src_h = p < 0 ? net->h : net->layers[p].out_h;
            L->src_w = p < 0 ? net->w : net->layers[p].out_w;
            if (L->src_c <= 0 || L->src_h <= 0 || L->src_w <= 0 || (long)L->src_c * L->src_h * L->src_w != l->inputs) {
                L->src_c = l->inputs; L->src_h = L->src_w = 1;
            }
        }
        if (l->type == DROPOUT) {
            L->alias = 1;
            L->out = t->L[i - 1].out; L->delta = t->L[i - 1].delta;
            if (dev_floats(&L->rnd, outs, e)) goto cleanup;
            HIP_OR_CLEANUP(y2h_host_alloc((void **)&L->h_rnd, outs * sizeof(float)));
            continue;
        }
        if (l->type == RNN) {
            if (prepare_rnn(net, i, t, e, pin, &dense_ws, &ws) != 0) {
                char why[256];
                snprintf(why, sizeof why, "%s", y2_last_error());
                y2_fail("y2_train_prepare: layer %d (rnn): its training buffers (%.1f MB for the network's recurrent layers) could not be made: %s",
                        i, rnn_bytes / 1048576., why);
                goto cleanup;
            }
            continue;
        }
        if (dev_floats(&L->out, outs, e) || dev_floats(&L->delta, outs, e)) goto cleanup;
        if (l->type == MAXPOOL) HIP_OR_CLEANUP(y2h_malloc((void **)&L->idx, outs * sizeof(int)));
        if (l->type == COST && dev_floats(&L->cost, 1, e)) goto cleanup;
        if (l->type == COST) scratch = max_z(scratch, Y2H_COST_CHUNKS * sizeof(float));
        if (l->type == REGION) {
            y2h_train_region rg = { net->batch, l->h, l->w, l->n, l->classes, l->bias_match, l->rescore, l->thresh, l->coord_scale,
                                    l->object_scale, l->noobject_scale, l->class_scale };
            L->rg = rg;
            if (y2h_train_region_scratch_bytes(&rg) == 0) { y2_fail("training: layer %d (region): shape outside what the kernels take", i); goto cleanup; }
            scratch = max_z(scratch, y2h_train_region_scratch_bytes(&rg));
            if (dev_floats(&L->cost, 1, e) || dev_floats(&L->biases, (size_t)2 * l->n, e) ||
                dev_floats((float **)&L->stats, sizeof(y2h_train_region_stats) / sizeof(float), e) ||
                push(L->biases, l->biases, (size_t)2 * l->n, pin, e)) goto cleanup;
        }
        if (l->type == DETECTION) {
            y2h_train_detection dt = { net->batch, l->side, l->n, l->classes, l->softmax, l->sqrt, l->rescore, l->forced, l->coord_scale,
                                       l->object_scale, l->noobject_scale, l->class_scale };
            L->dt = dt;
            if (y2h_train_detection_scratch_bytes(&dt) == 0) { y2_fail("training: layer %d (detection): shape outside what the kernels take", i); goto cleanup; }
            scratch = max_z(scratch, y2h_train_detection_scratch_bytes(&dt));
            if (dev_floats(&L->cost, 1, e) || dev_floats((float **)&L->dstats, sizeof(y2h_train_detection_stats) / sizeof(float), e)) goto cleanup;
        }
        if (l->type != CONVOLUTIONAL && l->type != CONNECTED) continue;
        {
            const size_t nw = (size_t)l->n * l->c * l->size * l->size;
            const long rows = (long)net->batch * l->out_h * l->out_w;
            y2h_train_conv g = { net->batch, l->h, l->w, l->c, l->n, l->size, l->pad, l->out_h, l->out_w };
            if (l->type == CONNECTED) {         /* l.n = outputs, l.c = inputs, size 1 on a 1 x 1 image (y2_cfg.c) */
                y2h_train_dense dg = { net->batch, l->inputs, l->outputs };
                size_t fw = 0, bw = 0;
                L->dg = dg;
                if (y2h_train_dense_plan(&dg, Y2H_DENSE_FORWARD, 0, &L->fwd_ranges, &fw, NULL, 0) != 0 ||
                    y2h_train_dense_plan(&dg, Y2H_DENSE_DINPUT, 0, &L->dx_ranges, &bw, NULL, 0) != 0) {
                    y2_fail("training: layer %d (connected): shape outside what the kernels take", i);
                    goto cleanup;
                }
                dense_ws = max_z(dense_ws, max_z(fw, bw));
            } else {
                L->g = g;
                if (l->out_h != l->h + 2 * l->pad - l->size + 1 || y2h_train_dweight_ws_bytes(&g) == 0) {
                    y2_fail("training: layer %d (convolutional): shape outside what the kernels take", i);
                    goto cleanup;
                }
                ws = max_z(ws, y2h_train_dweight_ws_bytes(&g));
            }
            scratch = max_z(scratch, y2h_train_reduce_scratch_bytes(rows, l->n));
            if (dev_floats(&L->weights, nw, e) || dev_floats(&L->weight_updates, nw, e) || dev_floats(&L->biases, l->n, e) ||
                dev_floats(&L->bias_updates, l->n, e)) goto cleanup;
            if (l->type == CONNECTED) y2_train_pack_dense_weights(l->weights, tmp, l->outputs, L->src_c, L->src_h, L->src_w);
            else y2_train_pack_weights(l->weights, tmp, l->n, l->c, l->size);
            if (push(L->weights, tmp, nw, pin, e) || push(L->biases, l->biases, l->n, pin, e)) goto cleanup;
            if (!l->batch_normalize) continue;
            if (dev_floats(&L->x, outs, e) || dev_floats(&L->x_norm, outs, e) || dev_floats(&L->mean, l->n, e) ||
                dev_floats(&L->variance, l->n, e) || dev_floats(&L->mean_delta, l->n, e) || dev_floats(&L->variance_delta, l->n, e) ||
                dev_floats(&L->scales, l->n, e) || dev_floats(&L->scale_updates, l->n, e) || dev_floats(&L->rolling_mean, l->n, e) ||
                dev_floats(&L->rolling_variance, l->n, e)) goto cleanup;
            if (push(L->scales, l->scales, l->n, pin, e) || push(L->rolling_mean, l->rolling_mean, l->n, pin, e) ||
                push(L->rolling_variance, l->rolling_variance, l->n, pin, e)) goto cleanup;
        }
    }
    if (t->dw_tmp_floats && dev_floats(&t->dw_tmp, t->dw_tmp_floats, e)) goto cleanup;
    if (t->step_ws_bytes) HIP_OR_CLEANUP(y2h_malloc((void **)&t->step_ws, t->step_ws_bytes));
    HIP_OR_CLEANUP(y2h_malloc((void **)&t->ws, ws));
    HIP_OR_CLEANUP(y2h_malloc((void **)&t->dense_ws, dense_ws));
    HIP_OR_CLEANUP(y2h_malloc((void **)&t->scratch, scratch));
    HIP_OR_CLEANUP(y2h_malloc((void **)&t->stage, stage * sizeof(float)));
    HIP_OR_CLEANUP(y2h_stream_sync(e->stream));
    rc = 0;
cleanup:
    free(tmp);
    if (rc != 0) y2_train_free(net);
    return rc;
}

/* ------------------------------------------------------------------ */
/* the step                                                            */
/* ------------------------------------------------------------------ */
static int forward_train(network *net, y2_trainer *t, y2_engine *e)
{
    const float *in = t->d_x;
    int i;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        y2_tlayer *L = &t->L[i];
        switch (l->type) {
        case CONVOLUTIONAL: {
            const long rows = (long)net->batch * l->out_h * l->out_w;
            HIP_OR_ERR(conv_forward(e, &L->g, in, L->weights, L->out));
            if (l->batch_normalize)
                HIP_OR_ERR(y2h_train_bn_stats(L->out, rows, l->n, L->mean, L->variance, L->rolling_mean, L->rolling_variance, t->scratch, e->stream));
            HIP_OR_ERR(y2h_train_bn_apply(L->out, L->x, L->x_norm, l->batch_normalize ? L->mean : NULL, L->variance, L->scales, L->biases,
                                          y2_act_code(l->activation), rows, l->n, e->stream));
        } break;
        case MAXPOOL:
            HIP_OR_ERR(y2h_train_maxpool_forward(in, L->out, L->idx, net->batch, l->h, l->w, l->c, l->size, l->stride, l->pad, l->out_h, l->out_w, e->stream));
            break;
        case AVGPOOL:
            HIP_OR_ERR(y2h_train_avgpool_forward(in, L->out, net->batch, l->h * l->w, l->c, e->stream));
            break;
        case SOFTMAX:
            HIP_OR_ERR(y2h_train_softmax(in, L->out, net->batch, l->inputs, l->temperature, e->stream));
            break;
        case COST:      /* forward and backward_cost_layer in one launch; over COST_CHUNKED_FROM values (a char-rnn's rows) in chunks */
            if ((long)net->batch * l->inputs >= COST_CHUNKED_FROM)
                HIP_OR_ERR(y2h_train_cost_sse_chunked(in, t->d_truth, L->out, L->delta, t->L[i - 1].delta, l->scale, (long)net->batch * l->inputs,
                                                      L->cost, t->scratch, e->stream));
            else
                HIP_OR_ERR(y2h_train_cost_sse(in, t->d_truth, L->out, L->delta, t->L[i - 1].delta, l->scale, (long)net->batch * l->inputs, L->cost, e->stream));
            break;
        case ROUTE: {
            int k, off = 0;
            for (k = 0; k < l->n; ++k) {
                const layer *src = &net->layers[l->input_layers[k]];
                HIP_OR_ERR(y2h_train_route_forward(t->L[l->input_layers[k]].out, src->out_c, L->out, l->out_c, off,
                                                   (long)net->batch * l->out_h * l->out_w, e->stream));
                off += src->out_c;
            }
        } break;
        case REORG:
            HIP_OR_ERR(y2h_reorg(in, l->c, L->out, l->out_c, net->batch, l->h, l->w, l->c, l->stride, 0, e->stream));
            break;
        case REGION:    /* forward and backward_region_layer; the last layer, so the first writer of the delta in front */
            HIP_OR_ERR(y2h_train_region_loss(&L->rg, in, L->biases, t->d_truth, *net->seen, L->out, L->delta, t->L[i - 1].delta, L->cost,
                                             L->stats, t->scratch, e->stream));
            break;
        case CONNECTED:     /* connected_layer.c:122-155; the rolling statistics move by .05 here, not by .1 */
            HIP_OR_ERR(y2h_train_dense_forward(&L->dg, in, L->weights, L->out, t->dense_ws, L->fwd_ranges, e->stream));
            if (l->batch_normalize)
                HIP_OR_ERR(y2h_train_bn_stats_rate(L->out, net->batch, l->outputs, L->mean, L->variance, L->rolling_mean, L->rolling_variance,
                                                   .95f, .05f, t->scratch, e->stream));
            HIP_OR_ERR(y2h_train_bn_apply(L->out, L->x, L->x_norm, l->batch_normalize ? L->mean : NULL, L->variance, L->scales, L->biases,
                                          y2_act_code(l->activation), net->batch, l->outputs, e->stream));
            break;
        case DROPOUT: {     /* dropout_layer.c:38-48 on the output in front, in place; rand_uniform(0, 1) per element in index order */
            const size_t n = (size_t)net->batch * l->inputs;
            size_t k;
            for (k = 0; k < n; ++k) L->h_rnd[k] = ((float)rand() / RAND_MAX * (1.f - 0.f)) + 0.f;
            HIP_OR_ERR(y2h_memcpy_h2d(L->rnd, L->h_rnd, n * sizeof(float), e->stream));
            HIP_OR_ERR(y2h_train_dropout(L->out, L->rnd, l->probability, (float)(1. / (1. - l->probability)), net->batch, L->src_c,
                                         L->src_h * L->src_w, e->stream));
        } break;
        case DETECTION:     /* forward and backward_detection_layer; the last layer, so the first writer of the delta in front */
            HIP_OR_ERR(y2h_train_detection_loss(&L->dt, in, t->d_truth, L->out, L->delta, t->L[i - 1].delta, 0, L->cost, L->dstats,
                                                t->scratch, e->stream));
            break;
        case RNN:
            if (forward_rnn(l, L, in, t, e) != 0) return -1;
            break;
        default:
            return -1;
        }
        if (l->type != COST) in = L->out;
    }
    return 0;
}

static int backward_train(network *net, y2_trainer *t, y2_engine *e)
{
    int i;
    for (i = net->n - 1; i >= 0; --i) {
        const layer *l = &net->layers[i];
        y2_tlayer *L = &t->L[i];
        const float *in = i ? t->L[i - 1].out : t->d_x;
        float *own = i ? t->L[i - 1].delta : NULL;          /* network.c:204-206: layer 0 has no state.delta */
        float *din = own && L->din_add ? t->stage : own;    /* a later writer lands in the staging buffer and is added below */
        switch (l->type) {
        case CONVOLUTIONAL: {
            const long rows = (long)net->batch * l->out_h * l->out_w;
            HIP_OR_ERR(y2h_train_act_gradient(L->out, L->delta, y2_act_code(l->activation), rows * l->n, e->stream));
            HIP_OR_ERR(y2h_train_bias_grad(L->delta, l->batch_normalize ? L->x_norm : NULL, rows, l->n, L->bias_updates,
                                           l->batch_normalize ? L->scale_updates : NULL, t->scratch, e->stream));
            if (l->batch_normalize) {
                HIP_OR_ERR(y2h_train_bn_deltas(L->delta, L->x, L->scales, L->mean, L->variance, rows, l->n, L->mean_delta, L->variance_delta,
                                               t->scratch, e->stream));
                HIP_OR_ERR(y2h_train_bn_backward(L->delta, L->x, L->scales, L->mean, L->variance, L->mean_delta, L->variance_delta, rows, l->n,
                                                 e->stream));
            }
            HIP_OR_ERR(conv_dweight(e, &L->g, in, L->delta, L->weight_updates, t->ws));
            if (din) HIP_OR_ERR(conv_dinput(e, &L->g, L->delta, L->weights, din));
        } break;
        case MAXPOOL:
            if (din) HIP_OR_ERR(y2h_train_maxpool_backward(L->delta, L->idx, din, net->batch, l->h, l->w, l->c, l->size, l->stride, l->pad,
                                                           l->out_h, l->out_w, e->stream));
            break;
        case AVGPOOL:
            if (din) HIP_OR_ERR(y2h_train_avgpool_backward(L->delta, din, net->batch, l->h * l->w, l->c, e->stream));
            break;
        case SOFTMAX:   /* softmax_layer.c:57-63: state.delta += l.delta */
            if (din) HIP_OR_ERR(y2h_memcpy_d2d(din, L->delta, (size_t)net->batch * l->inputs * sizeof(float), e->stream));
            break;
        case COST: case REGION: case DETECTION:     /* done with its forward */
            break;
        case CONNECTED:     /* connected_layer.c:157-191 */
            HIP_OR_ERR(y2h_train_act_gradient(L->out, L->delta, y2_act_code(l->activation), (long)net->batch * l->outputs, e->stream));
            HIP_OR_ERR(y2h_train_bias_grad(L->delta, l->batch_normalize ? L->x_norm : NULL, net->batch, l->outputs, L->bias_updates,
                                           l->batch_normalize ? L->scale_updates : NULL, t->scratch, e->stream));
            if (l->batch_normalize) {
                HIP_OR_ERR(y2h_train_bn_deltas(L->delta, L->x, L->scales, L->mean, L->variance, net->batch, l->outputs, L->mean_delta,
                                               L->variance_delta, t->scratch, e->stream));
                HIP_OR_ERR(y2h_train_bn_backward(L->delta, L->x, L->scales, L->mean, L->variance, L->mean_delta, L->variance_delta, net->batch,
                                                 l->outputs, e->stream));
            }
            HIP_OR_ERR(y2h_train_dense_dweight(&L->dg, in, L->delta, L->weight_updates, e->stream));
            /* always a store: a later writer lands in the staging buffer and is added below, like every other layer, so the
             * kernel's own add mode is exercised by the product test alone */
            if (din) HIP_OR_ERR(y2h_train_dense_dinput(&L->dg, L->delta, L->weights, din, 0, t->dense_ws, L->dx_ranges, e->stream));
            break;
        case RNN:
            if (backward_rnn(l, L, in, din, t, e) != 0) return -1;
            break;
        case DROPOUT:       /* dropout_layer.c:50-59: the delta in front, in place */
            if (own) HIP_OR_ERR(y2h_train_dropout(own, L->rnd, l->probability, (float)(1. / (1. - l->probability)), net->batch, L->src_c,
                                                  L->src_h * L->src_w, e->stream));
            break;
        case ROUTE: {
            int k, off = 0;
            for (k = 0; k < l->n; ++k) {
                const layer *src = &net->layers[l->input_layers[k]];
                HIP_OR_ERR(y2h_train_route_backward(L->delta, l->out_c, off, t->L[l->input_layers[k]].delta, src->out_c,
                                                    (long)net->batch * l->out_h * l->out_w, L->src_add[k], e->stream));
                off += src->out_c;
            }
        } break;
        case REORG:
            HIP_OR_ERR(y2h_train_reorg_backward(L->delta, own, net->batch, l->h, l->w, l->c, l->stride, e->stream));
            break;
        default:
            return -1;
        }
        if (own && L->din_add) HIP_OR_ERR(y2h_train_add(own, t->stage, (long)net->batch * net->layers[i - 1].outputs, e->stream));
    }
    return 0;
}

static int update_train(network *net, y2_trainer *t, y2_engine *e)
{
    const int batch = net->batch * net->subdivisions;
    const float rate = get_current_rate(*net);
    int i;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        y2_tlayer *L = &t->L[i];
        if (l->type == RNN) {           /* update_rnn_layer: three update_connected_layer calls */
            int k;
            for (k = 0; k < 3; ++k) {
                const layer *s = rnn_sub(l, k);
                y2_tlayer *S = &L->sub[k];
                HIP_OR_ERR(y2h_train_sgd(S->biases, S->bias_updates, s->outputs, rate / batch, 0.f, net->momentum, e->stream));
                if (s->batch_normalize) HIP_OR_ERR(y2h_train_sgd(S->scales, S->scale_updates, s->outputs, rate / batch, 0.f, net->momentum, e->stream));
                HIP_OR_ERR(y2h_train_sgd(S->weights, S->weight_updates, (long)s->outputs * s->inputs, rate / batch, -net->decay * batch,
                                         net->momentum, e->stream));
            }
            continue;
        }
        if (l->type != CONVOLUTIONAL && l->type != CONNECTED) continue;     /* update_connected_layer has the convolution's order */
        HIP_OR_ERR(y2h_train_sgd(L->biases, L->bias_updates, l->n, rate / batch, 0.f, net->momentum, e->stream));
        if (l->batch_normalize) HIP_OR_ERR(y2h_train_sgd(L->scales, L->scale_updates, l->n, rate / batch, 0.f, net->momentum, e->stream));
        HIP_OR_ERR(y2h_train_sgd(L->weights, L->weight_updates, (long)l->n * l->c * l->size * l->size, rate / batch, -net->decay * batch,
                                 net->momentum, e->stream));
    }
    return 0;
}

/* everything of a step behind `*net.seen += net.batch`; d_x_nchw == NULL: the trainer's NHWC input is already in place
 * (y2_train_load_detection) */
static int step_enqueue(network *net, const float *d_x_nchw, const float *d_y, float *loss)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e->trainer;
    int i, costs = 0;
    float sum = 0;
    if (d_x_nchw) {
        t->loaded = 0;
        if (net->h > 0 && net->w > 0 && net->c > 0)
            HIP_OR_ERR(y2h_nchw_to_nhwc(d_x_nchw, t->d_x, net->batch, net->c, net->h, net->w, net->c, e->stream));
        else            /* a flat input (inputs= in front of an [rnn]): rows as given */
            HIP_OR_ERR(y2h_memcpy_d2d(t->d_x, d_x_nchw, (size_t)net->batch * net->inputs * sizeof(float), e->stream));
    }
    if (d_y != t->d_truth)
        HIP_OR_ERR(y2h_memcpy_d2d(t->d_truth, d_y, t->truth_floats * sizeof(float), e->stream));
    t->dirty = 1;          /* from the first launch on: the forward pass already moves the rolling statistics */
    if (forward_train(net, t, e) != 0 || backward_train(net, t, e) != 0) return -1;
    if ((*net->seen / net->batch) % net->subdivisions == 0 && update_train(net, t, e) != 0) return -1;
    for (i = 0; i < net->n; ++i)
        if (t->L[i].cost) HIP_OR_ERR(y2h_memcpy_d2h(t->h_cost + costs++, t->L[i].cost, sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    for (i = 0, costs = 0; i < net->n; ++i)
        if (t->L[i].cost) { net->layers[i].cost[0] = t->h_cost[costs++]; sum += net->layers[i].cost[0]; }
    if (loss) *loss = sum / costs;              /* get_network_cost */
    return 0;
}

static int step_on_device(network *net, const float *d_x_nchw, const float *d_y, float *loss)
{
    *net->seen += net->batch;                   /* first, as in the reference: the update's rate reads it */
    if (step_enqueue(net, d_x_nchw, d_y, loss) == 0) return 0;
    *net->seen -= net->batch;                   /* a step that failed does not move the schedule */
    return -1;
}

static y2_trainer *trainer_for_step(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (!e) { y2_fail("y2_train_step: network has no engine (was it built by parse_network_cfg?)"); return NULL; }
    if ((!e->trainer || e->trainer->batch != net->batch) && y2_train_prepare(net) != 0) return NULL;
    if (y2h_set_device(e->device) != 0) { y2_fail("y2_train_step: %s", y2h_last_error()); return NULL; }
    return e->trainer;
}

int y2_train_step_device(network *net, const float *d_x, const float *d_y, float *loss)
{
    if (!d_x || !d_y) { y2_fail("y2_train_step_device: NULL input"); return -1; }
    if (!trainer_for_step(net)) return -1;
    return step_on_device(net, d_x, d_y, loss);
}

int y2_train_step(network *net, const float *x, const float *y, float *loss)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t;
    size_t nx, ny;
    if (!x || !y) { y2_fail("y2_train_step: NULL input"); return -1; }
    if (!(t = trainer_for_step(net))) return -1;
    nx = (size_t)net->batch * net->inputs;
    ny = t->truth_floats;
    /* pinned staging (h_in: nx + ny floats, made with the trainer): no pageable buffer of a caller is handed to an
     * asynchronous copy; the step's final wait is behind both copies, so the buffer is free again when it returns */
    memcpy(t->h_in, x, nx * sizeof(float));
    memcpy(t->h_in + nx, y, ny * sizeof(float));
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_x_nchw, t->h_in, nx * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_truth, t->h_in + nx, ny * sizeof(float), e->stream));
    if (step_on_device(net, t->d_x_nchw, t->d_truth, loss) != 0) { y2h_stream_sync(e->stream); return -1; }
    return 0;
}

float train_network_datum(network net, float *x, float *y)
{
    float loss = NAN;
    if (y2_train_step(&net, x, y, &loss) != 0) return NAN;
    return loss;
}

/* ------------------------------------------------------------------ */
/* the detection loader (data.c:664-714): frames and label rows in      */
/* ------------------------------------------------------------------ */
int y2_net_augment(network net, float *jitter, float *hue, float *saturation, float *exposure, int *random)
{
    const y2_engine *e = y2_engine_of(&net);
    const layer *last = net.layers && net.n > 0 ? &net.layers[net.n - 1] : NULL;
    if (!e || !last) { y2_fail("y2_net_augment: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (last->type != REGION) { y2_fail("y2_net_augment: layer %d (%s): the network must end in [region]", net.n - 1, get_layer_string(last->type)); return -1; }
    if (jitter) *jitter = last->jitter;
    if (random) *random = last->random;
    if (hue) *hue = e->aug_hue;
    if (saturation) *saturation = e->aug_saturation;
    if (exposure) *exposure = e->aug_exposure;
    return 0;
}

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static int grow_load(y2_trainer *t, size_t need)
{
    if (need > t->h_load_cap) {
        y2h_host_free(t->h_load); t->h_load = NULL; t->h_load_cap = 0;
        HIP_OR_ERR(y2h_host_alloc((void **)&t->h_load, need));
        t->h_load_cap = need;
    }
    if (need > t->d_load_cap) {
        y2h_free(t->d_load); t->d_load = NULL; t->d_load_cap = 0;
        HIP_OR_ERR(y2h_malloc((void **)&t->d_load, need));
        t->d_load_cap = need;
    }
    if (!t->ev_load) HIP_OR_ERR(y2h_event_create(&t->ev_load));
    return 0;
}

int y2_train_load_detection(network *net, const y2_aug_item *items, int n, int swap_rb)
{
    static const char who[] = "y2_train_load_detection";
    y2_engine *e;
    y2_trainer *t;
    size_t desc_bytes, truth_bytes, need;
    double t0, t1, t2;
    float *truth;
    int i, truths;
    if (!net || !net->layers || net->n <= 0) { y2_fail("%s: no network", who); return -1; }
    if (n != net->batch) { y2_fail("%s: %d items for a batch-%d network", who, n, net->batch); return -1; }
    if (net->c != 3) { y2_fail("%s: the network reads %d channels, the loader makes 3", who, net->c); return -1; }
    if (net->layers[net->n - 1].type != REGION) {
        y2_fail("%s: layer %d (%s): the network must end in [region] (the truth is [batch][150])", who, net->n - 1,
                get_layer_string(net->layers[net->n - 1].type));
        return -1;
    }
    if (refuse(net) != 0 || y2_aug_check(who, items, n) != 0) return -1;
    if (!(t = trainer_for_step(net))) return -1;
    e = y2_engine_of(net);
    truths = truths_per_image(net);
    desc_bytes = align_up((size_t)n * sizeof(y2h_aug), 64);
    truth_bytes = align_up(t->truth_floats * sizeof(float), 64);
    need = desc_bytes + truth_bytes + y2_aug_pack_bytes(items, n);
    t->loaded = 0;
    /* the staging buffer is free: the last load waited for its copy before it returned */
    if (grow_load(t, need) != 0) return -1;
    t0 = now_ms();
    y2_aug_pack(items, n, net->w, net->h, (y2h_aug *)t->h_load, t->h_load + desc_bytes + truth_bytes);
    truth = (float *)(t->h_load + desc_bytes);
    for (i = 0; i < n; ++i)
        if (y2_aug_truth_detection(&items[i], truths / 5, truth + (size_t)i * truths) != 0) return -1;
    t1 = now_ms();
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_load, t->h_load, need, e->stream));
    HIP_OR_ERR(y2h_event_record(t->ev_load, e->stream));
    HIP_OR_ERR(y2h_augment_to_input((const y2h_aug *)t->d_load, n, t->d_load + desc_bytes + truth_bytes, swap_rb, net->h, net->w, t->d_x,
                                    e->stream));
    HIP_OR_ERR(y2h_memcpy_d2d(t->d_truth, t->d_load + desc_bytes, t->truth_floats * sizeof(float), e->stream));
    t2 = now_ms();
    HIP_OR_ERR(y2h_event_sync(t->ev_load));
    t->load_ms[0] = (float)(t1 - t0); t->load_ms[1] = (float)(t2 - t1); t->load_ms[2] = (float)(now_ms() - t2);
    t->loaded = 1;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the classifier loader (data.c:870-879 load_data_augment)             */
/* ------------------------------------------------------------------ */
int y2_net_augment_classifier(network net, int *min_crop, int *max_crop, float *angle, float *aspect, float *hue,
                              float *saturation, float *exposure)
{
    const y2_engine *e = y2_engine_of(&net);
    if (!e) { y2_fail("y2_net_augment_classifier: network has no engine (was it built by parse_network_cfg?)"); return -1; }
    if (min_crop) *min_crop = e->aug_min_crop;
    if (max_crop) *max_crop = e->aug_max_crop;
    if (angle) *angle = e->aug_angle;
    if (aspect) *aspect = e->aug_aspect;
    if (hue) *hue = e->aug_hue;
    if (saturation) *saturation = e->aug_saturation;
    if (exposure) *exposure = e->aug_exposure;
    return 0;
}

int y2_train_load_classification(network *net, const y2_aug_cls_item *items, const float *truth, int n, int swap_rb)
{
    static const char who[] = "y2_train_load_classification";
    y2_engine *e;
    y2_trainer *t;
    y2h_aug_cls *desc;
    size_t desc_bytes, truth_bytes, need;
    double t0, t1, t2;
    if (!net || !net->layers || net->n <= 0) { y2_fail("%s: no network", who); return -1; }
    e = y2_engine_of(net);
    if (e && e->trainer) e->trainer->loaded = 0;         /* a refused load leaves nothing to step on */
    if (n != net->batch) { y2_fail("%s: %d items for a batch-%d network", who, n, net->batch); return -1; }
    if (net->c != 3) { y2_fail("%s: the network reads %d channels, the loader makes 3", who, net->c); return -1; }
    if (net->h != net->w) {
        y2_fail("%s: the network is %d x %d: the loader makes net.w x net.w crops (args.size = net.w)", who, net->w, net->h);
        return -1;
    }
    if (net->layers[net->n - 1].type == REGION) {
        y2_fail("%s: layer %d (region): the network ends in [region] (y2_train_load_detection loads a detector)", who, net->n - 1);
        return -1;
    }
    if (refuse(net) != 0) return -1;
    if (!truth) { y2_fail("%s: truth is NULL", who); return -1; }
    if (y2_aug_cls_check(who, items, n) != 0) return -1;
    if (!(t = trainer_for_step(net))) return -1;
    e = y2_engine_of(net);
    desc_bytes = align_up((size_t)n * sizeof(y2h_aug_cls), 64);
    truth_bytes = align_up(t->truth_floats * sizeof(float), 64);
    t->loaded = 0;
    t0 = now_ms();
    /* the table first, once: it says how many pixel bytes the staging buffer must hold */
    if (!(desc = malloc((size_t)n * sizeof *desc))) { y2_fail("%s: out of memory", who); return -1; }
    need = desc_bytes + truth_bytes + y2_aug_cls_describe(items, n, net->w, desc);
    /* the staging buffer is free: the last load waited for its copy before it returned */
    if (grow_load(t, need) != 0) { free(desc); return -1; }
    memcpy(t->h_load, desc, (size_t)n * sizeof *desc);
    y2_aug_cls_copy(items, n, desc, t->h_load + desc_bytes + truth_bytes);
    free(desc);
    memcpy(t->h_load + desc_bytes, truth, t->truth_floats * sizeof(float));
    t1 = now_ms();
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_load, t->h_load, need, e->stream));
    HIP_OR_ERR(y2h_event_record(t->ev_load, e->stream));
    HIP_OR_ERR(y2h_augment_cls_to_input((const y2h_aug_cls *)t->d_load, n, t->d_load + desc_bytes + truth_bytes, swap_rb, net->w, t->d_x,
                                        e->stream));
    HIP_OR_ERR(y2h_memcpy_d2d(t->d_truth, t->d_load + desc_bytes, t->truth_floats * sizeof(float), e->stream));
    t2 = now_ms();
    HIP_OR_ERR(y2h_event_sync(t->ev_load));
    t->load_ms[0] = (float)(t1 - t0); t->load_ms[1] = (float)(t2 - t1); t->load_ms[2] = (float)(now_ms() - t2);
    t->loaded = 1;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the char-rnn loader (rnn.c:86-114 get_rnn_data)                      */
/* ------------------------------------------------------------------ */
int y2_get_rnn_data(const unsigned char *text, size_t *offsets, int characters, size_t len, int batch, int steps, float *x, float *y)
{
    int i, j;
    if (!text || !offsets || !x || !y || characters <= 0 || len == 0 || batch <= 0 || steps <= 0) { y2_fail("get_rnn_data: bad arguments"); return -1; }
    for (i = 0; i < batch; ++i) {           /* checked before anything is written or moved: the reference exits half-way */
        size_t o = offsets[i];
        for (j = 0; j <= steps; ++j, ++o) {
            const unsigned char ch = text[o % len];
            if (ch == 0 || ch >= characters) { y2_fail("get_rnn_data: Bad char (byte %d at offset %zu; the network reads %d characters)", (int)ch, o % len, characters); return -1; }
        }
    }
    memset(x, 0, (size_t)batch * steps * characters * sizeof(float));
    memset(y, 0, (size_t)batch * steps * characters * sizeof(float));
    for (i = 0; i < batch; ++i)
        for (j = 0; j < steps; ++j) {
            const unsigned char curr = text[offsets[i] % len], next = text[(offsets[i] + 1) % len];
            x[((size_t)j * batch + i) * characters + curr] = 1;
            y[((size_t)j * batch + i) * characters + next] = 1;
            offsets[i] = (offsets[i] + 1) % len;
        }
    return 0;
}

int y2_train_load_rnn_data(network *net, const unsigned char *text, size_t len, size_t *offsets)
{
    static const char who[] = "y2_train_load_rnn_data";
    y2_engine *e;
    y2_trainer *t;
    unsigned char *tok;
    int T, B, i, j;
    if (!net || !net->layers || net->n <= 0) { y2_fail("%s: no network", who); return -1; }
    e = y2_engine_of(net);
    if (e && e->trainer) e->trainer->loaded = 0;         /* a refused load leaves nothing to step on */
    if (!text || !len || !offsets) { y2_fail("%s: NULL text or offsets", who); return -1; }
    /* a trainer of this batch exists only for a network y2_train_prepare accepted: the loop's calls skip the walk */
    if (!(e && e->trainer && e->trainer->batch == net->batch) && refuse(net) != 0) return -1;
    if (net->layers[0].type != RNN || truths_per_image(net) != net->inputs) {
        y2_fail("%s: the network must start with an [rnn] and end in a [cost] over as many values as it reads (one-hot in, one-hot truth)", who);
        return -1;
    }
    T = net->time_steps; B = net->batch / T;
    for (i = 0; i < B; ++i)
        for (j = 0; j <= T; ++j) {
            const unsigned char ch = text[(offsets[i] + j) % len];
            if (ch == 0 || ch >= net->inputs) { y2_fail("%s: Bad char (byte %d at offset %zu; the network reads %d characters)", who, (int)ch, (offsets[i] + j) % len, net->inputs); return -1; }
        }
    if (!(t = trainer_for_step(net))) return -1;
    e = y2_engine_of(net);
    t->loaded = 0;
    if (grow_load(t, (size_t)B * (T + 1)) != 0) return -1;   /* free: the last load waited for its copy before it returned */
    tok = t->h_load;
    for (i = 0; i < B; ++i) {
        for (j = 0; j <= T; ++j) tok[(size_t)i * (T + 1) + j] = text[(offsets[i] + j) % len];
        offsets[i] = (offsets[i] + T) % len;            /* T times (o + 1) % len */
    }
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_load, t->h_load, (size_t)B * (T + 1), e->stream));
    HIP_OR_ERR(y2h_event_record(t->ev_load, e->stream));
    HIP_OR_ERR(y2h_train_rnn_onehot(t->d_load, T, B, net->inputs, t->d_x, t->d_truth, e->stream));
    HIP_OR_ERR(y2h_event_sync(t->ev_load));         /* recorded behind the copy, in front of the kernel: the pinned bytes are free again */
    t->loaded = 1;
    return 0;
}

/* ------------------------------------------------------------------ */
/* the Go loader (go.c:92-115 random_go_moves)                          */
/* ------------------------------------------------------------------ */
int y2_train_load_go(network *net, const unsigned char *records, int n_records, const int *pick, const int *flip, const int *rot)
{
    static const char who[] = "y2_train_load_go";
    enum { P = 361, REC = 93 };
    y2_engine *e;
    y2_trainer *t;
    size_t rec_bytes, draw_bytes;
    int i, B, *draws;
    if (!net || !net->layers || net->n <= 0) { y2_fail("%s: no network", who); return -1; }
    e = y2_engine_of(net);
    if (e && e->trainer) e->trainer->loaded = 0;         /* a refused load leaves nothing to step on */
    if (net->w != 19 || net->h != 19 || net->c != 1) {
        y2_fail("%s: net: the network reads %d x %d x %d, a Go network reads 19 x 19 x 1", who, net->w, net->h, net->c);
        return -1;
    }
    if (!(e && e->trainer && e->trainer->batch == net->batch) && refuse(net) != 0) return -1;
    if (net->layers[net->n - 1].type != COST || truths_per_image(net) != P) {
        y2_fail("%s: net: the network must end in a [cost] over 361 values (one per point)", who);
        return -1;
    }
    if (!records || n_records <= 0) { y2_fail("%s: n_records = %d (or NULL records)", who, n_records); return -1; }
    if (!pick || !flip || !rot) { y2_fail("%s: pick, flip or rot is NULL", who); return -1; }
    B = net->batch;
    for (i = 0; i < B; ++i) {
        const signed char *r;
        if (pick[i] < 0 || pick[i] >= n_records) { y2_fail("%s: pick: item %d picks record %d of %d", who, i, pick[i], n_records); return -1; }
        if (flip[i] != 0 && flip[i] != 1) { y2_fail("%s: flip: item %d has flip %d (0 or 1)", who, i, flip[i]); return -1; }
        if (rot[i] < 0 || rot[i] > 3) { y2_fail("%s: rot: item %d has rot %d (0..3)", who, i, rot[i]); return -1; }
        r = (const signed char *)records + (size_t)pick[i] * REC;
        if (r[0] < 0 || r[0] > 18 || r[1] < 0 || r[1] > 18) {
            y2_fail("%s: records: record %d moves at row %d, column %d (0..18)", who, pick[i], r[0], r[1]);
            return -1;
        }
    }
    if (!(t = trainer_for_step(net))) return -1;
    e = y2_engine_of(net);
    t->loaded = 0;
    rec_bytes = align_up((size_t)B * REC, 64);
    draw_bytes = (size_t)2 * B * sizeof(int);
    if (grow_load(t, rec_bytes + draw_bytes) != 0) return -1;        /* free: the last load waited for its copy before it returned */
    draws = (int *)(t->h_load + rec_bytes);
    for (i = 0; i < B; ++i) {                           /* only the picked records go up, in batch order */
        memcpy(t->h_load + (size_t)i * REC, records + (size_t)pick[i] * REC, REC);
        draws[i] = flip[i];
        draws[B + i] = rot[i];
    }
    HIP_OR_ERR(y2h_memcpy_h2d(t->d_load, t->h_load, rec_bytes + draw_bytes, e->stream));
    HIP_OR_ERR(y2h_event_record(t->ev_load, e->stream));
    HIP_OR_ERR(y2h_go_decode(t->d_load, NULL, (const int *)(t->d_load + rec_bytes), (const int *)(t->d_load + rec_bytes) + B, B, t->d_x,
                             t->d_truth, e->stream));
    HIP_OR_ERR(y2h_event_sync(t->ev_load));
    t->loaded = 1;
    return 0;
}

int y2_train_step_loaded(network *net, float *loss)
{
    y2_engine *e = net ? y2_engine_of(net) : NULL;
    y2_trainer *t = e ? e->trainer : NULL;
    if (!t || !t->loaded || t->batch != net->batch) {
        y2_fail("y2_train_step_loaded: nothing is loaded (y2_train_load_detection / y2_train_load_classification / y2_train_load_rnn_data; set_batch_network and resize_network drop a load)");
        return -1;
    }
    HIP_OR_ERR(y2h_set_device(e->device));
    return step_on_device(net, NULL, t->d_truth, loss);
}

int y2_train_load_times(network *net, float *ms)
{
    y2_engine *e = net ? y2_engine_of(net) : NULL;
    if (!e || !e->trainer || !ms) { y2_fail("y2_train_load_times: no trainer (y2_train_load_detection / y2_train_load_classification)"); return -1; }
    memcpy(ms, e->trainer->load_ms, sizeof e->trainer->load_ms);
    return 0;
}

/* ------------------------------------------------------------------ */
/* looking at it                                                       */
/* ------------------------------------------------------------------ */
/* through the trainer's pinned landing buffer (n <= stage_floats: checked by the caller's size test) */
static int pull_flat(y2_engine *e, const float *src, float *dst, size_t n)
{
    float *pin = e->trainer->h_pull;
    if (n > e->trainer->stage_floats) { y2_fail("y2_train_pull: %zu floats exceed the staging buffer", n); return -1; }
    HIP_OR_ERR(y2h_memcpy_d2h(pin, src, n * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    memcpy(dst, pin, n * sizeof(float));
    return 0;
}

/* one array of sub-layer k of an [rnn]: activations over all T*B rows, step-major; mean and variance as the reference's
 * arrays hold them after a step, the LAST time step's */
static int pull_rnn(network *net, int i, int k, int what, float *dst, size_t n)
{
    y2_engine *e = y2_engine_of(net);
    const layer *l = &net->layers[i], *s = rnn_sub(l, k);
    const y2_tlayer *S = &e->trainer->L[i].sub[k];
    const size_t rows = (size_t)l->steps * l->batch, last = (size_t)(l->steps - 1) * s->outputs;
    const float *src = NULL;
    size_t have = s->outputs;
    switch (what) {
    case Y2_TRAIN_OUTPUT: src = S->out; have *= rows; break;
    case Y2_TRAIN_DELTA: src = S->delta; have *= rows; break;
    case Y2_TRAIN_X: src = S->x; have *= rows; break;
    case Y2_TRAIN_X_NORM: src = S->x_norm; have *= rows; break;
    case Y2_TRAIN_MEAN: src = S->mean ? S->mean + last : NULL; break;
    case Y2_TRAIN_VARIANCE: src = S->variance ? S->variance + last : NULL; break;
    case Y2_TRAIN_MEAN_DELTA: src = S->mean_delta; break;
    case Y2_TRAIN_VARIANCE_DELTA: src = S->variance_delta; break;
    case Y2_TRAIN_WEIGHT_UPDATES: src = S->weight_updates; have *= s->inputs; break;
    case Y2_TRAIN_WEIGHTS: src = S->weights; have *= s->inputs; break;
    case Y2_TRAIN_BIAS_UPDATES: src = S->bias_updates; break;
    case Y2_TRAIN_BIASES: src = S->biases; break;
    case Y2_TRAIN_SCALE_UPDATES: src = S->scale_updates; break;
    case Y2_TRAIN_SCALES: src = S->scales; break;
    case Y2_TRAIN_ROLLING_MEAN: src = S->rolling_mean; break;
    case Y2_TRAIN_ROLLING_VARIANCE: src = S->rolling_variance; break;
    }
    if (!src) { y2_fail("y2_train_pull: layer %d (rnn) sub-layer %d has no array %d", i, k, what); return -1; }
    if (n != have) { y2_fail("y2_train_pull: layer %d sub-layer %d array %d holds %zu floats, not %zu", i, k, what, have, n); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    return pull_flat(e, src, dst, n);
}

int y2_train_pull(network *net, int i, int what, float *dst, size_t n)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e ? e->trainer : NULL;
    const layer *l;
    y2_tlayer *L;
    const float *src = NULL;
    size_t have = 0;
    int image = 0, weights = 0;
    if (!t) { y2_fail("y2_train_pull: no trainer (y2_train_prepare)"); return -1; }
    if (i < 0 || i >= net->n || !dst) { y2_fail("y2_train_pull: layer %d of %d", i, net->n); return -1; }
    l = &net->layers[i];
    L = &t->L[i];
    if (what >> 8) {                                        /* Y2_TRAIN_SUB(k, what) */
        if (l->type != RNN || (what >> 8) > 3) { y2_fail("y2_train_pull: layer %d (%s) has no sub-layer %d", i, get_layer_string(l->type), (what >> 8) - 1); return -1; }
        return pull_rnn(net, i, (what >> 8) - 1, what & 255, dst, n);
    }
    if (what == Y2_TRAIN_STATE) {
        const size_t have = l->type == RNN ? (size_t)(l->steps + 1) * l->batch * l->hidden : 0;
        if (!have) { y2_fail("y2_train_pull: layer %d (%s) has no state", i, get_layer_string(l->type)); return -1; }
        if (n != have) { y2_fail("y2_train_pull: layer %d state holds %zu floats, not %zu", i, have, n); return -1; }
        HIP_OR_ERR(y2h_set_device(e->device));
        return pull_flat(e, L->state, dst, n);
    }
    switch (what) {
    case Y2_TRAIN_OUTPUT: src = L->out; image = 1; break;
    case Y2_TRAIN_DELTA: src = L->delta; image = 1; break;
    case Y2_TRAIN_X: src = L->x; image = 1; break;
    case Y2_TRAIN_X_NORM: src = L->x_norm; image = 1; break;
    case Y2_TRAIN_MEAN: src = L->mean; break;
    case Y2_TRAIN_VARIANCE: src = L->variance; break;
    case Y2_TRAIN_MEAN_DELTA: src = L->mean_delta; break;
    case Y2_TRAIN_VARIANCE_DELTA: src = L->variance_delta; break;
    case Y2_TRAIN_WEIGHT_UPDATES: src = L->weight_updates; weights = 1; break;
    case Y2_TRAIN_WEIGHTS: src = L->weights; weights = 1; break;
    case Y2_TRAIN_BIAS_UPDATES: src = L->bias_updates; break;
    case Y2_TRAIN_BIASES: src = L->biases; break;
    case Y2_TRAIN_SCALE_UPDATES: src = L->scale_updates; break;
    case Y2_TRAIN_SCALES: src = L->scales; break;
    case Y2_TRAIN_ROLLING_MEAN: src = L->rolling_mean; break;
    case Y2_TRAIN_ROLLING_VARIANCE: src = L->rolling_variance; break;
    case Y2_TRAIN_RAND: src = L->rnd; image = 1; break;
    }
    if (l->type == DROPOUT && what != Y2_TRAIN_RAND) src = NULL;    /* its output and delta are the layer's in front: pull those */
    if (l->type == REGION && !image) src = NULL;             /* its `biases` are the anchors, not a trainable array */
    if (!src) { y2_fail("y2_train_pull: layer %d (%s) has no array %d", i, get_layer_string(l->type), what); return -1; }
    have = image ? (size_t)net->batch * l->outputs : weights ? (size_t)l->n * l->c * l->size * l->size : (size_t)l->n;
    if (n != have) { y2_fail("y2_train_pull: layer %d array %d holds %zu floats, not %zu", i, what, have, n); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (l->type == REGION && what == Y2_TRAIN_DELTA && l->h * l->w > 1) {      /* the reference un-flattens only the delta */
        HIP_OR_ERR(y2h_nhwc_to_nchw(src, l->n * (5 + l->classes), t->stage, net->batch, l->n * (5 + l->classes), l->h, l->w, e->stream));
        return pull_flat(e, t->stage, dst, n);
    }
    if (image && (l->type == CONVOLUTIONAL || l->type == MAXPOOL || l->type == ROUTE || l->type == REORG) && l->out_h * l->out_w > 1) {
        HIP_OR_ERR(y2h_nhwc_to_nchw(src, l->out_c, t->stage, net->batch, l->out_c, l->out_h, l->out_w, e->stream));
        return pull_flat(e, t->stage, dst, n);
    }
    if (weights) {
        float *tmp = malloc(n * sizeof(float));
        int rc = pull_flat(e, src, tmp, n);
        if (rc == 0 && l->type == CONNECTED) y2_train_unpack_dense_weights(tmp, dst, l->outputs, L->src_c, L->src_h, L->src_w);
        else if (rc == 0) y2_train_unpack_weights(tmp, dst, l->n, l->c, l->size);
        free(tmp);
        return rc;
    }
    return pull_flat(e, src, dst, n);
}

int y2_train_pull_input(network *net, float *x_nchw, float *truth)
{
    y2_engine *e = net ? y2_engine_of(net) : NULL;
    y2_trainer *t = e ? e->trainer : NULL;
    if (!t || !t->loaded) { y2_fail("y2_train_pull_input: nothing is loaded (y2_train_load_detection / y2_train_load_classification)"); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (x_nchw && !(net->h > 0 && net->w > 0 && net->c > 0)) {        /* a flat input: rows as they are */
        if (pull_flat(e, t->d_x, x_nchw, (size_t)net->batch * net->inputs) != 0) return -1;
    } else if (x_nchw) {
        HIP_OR_ERR(y2h_nhwc_to_nchw(t->d_x, net->c, t->stage, net->batch, net->c, net->h, net->w, e->stream));
        if (pull_flat(e, t->stage, x_nchw, (size_t)net->batch * net->inputs) != 0) return -1;
    }
    if (truth && pull_flat(e, t->d_truth, truth, t->truth_floats) != 0) return -1;
    return 0;
}

int y2_train_region_stats(network *net, int i, y2_region_stats *out)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e ? e->trainer : NULL;
    if (!t) { y2_fail("y2_train_region_stats: no trainer (y2_train_prepare)"); return -1; }
    if (i < 0 || i >= net->n || !out || !t->L[i].stats) { y2_fail("y2_train_region_stats: layer %d of %d is no [region] layer", i, net->n); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    HIP_OR_ERR(y2h_memcpy_d2h(t->h_pull, t->L[i].stats, sizeof(y2h_train_region_stats), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    memcpy(out, t->h_pull, sizeof *out);     /* y2_region_stats and y2h_train_region_stats are one layout */
    return 0;
}

int y2_train_detection_stats(network *net, int i, y2_detection_stats *out)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e ? e->trainer : NULL;
    if (!t) { y2_fail("y2_train_detection_stats: no trainer (y2_train_prepare)"); return -1; }
    if (i < 0 || i >= net->n || !out || !t->L[i].dstats) { y2_fail("y2_train_detection_stats: layer %d of %d is no [detection] layer", i, net->n); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    HIP_OR_ERR(y2h_memcpy_d2h(t->h_pull, t->L[i].dstats, sizeof(y2h_train_detection_stats), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    memcpy(out, t->h_pull, sizeof *out);     /* y2_detection_stats and y2h_train_detection_stats are one layout */
    return 0;
}

int y2_train_is_dirty(const network *net)
{
    const y2_engine *e = y2_engine_of(net);
    return e && e->trainer && e->trainer->dirty;
}

/* masters -> host layer arrays; the inference arena is re-packed by whoever reads it next */
int y2_train_sync_if_dirty(network *net)
{
    y2_engine *e = y2_engine_of(net);
    y2_trainer *t = e ? e->trainer : NULL;
    int i;
    if (!t || !t->dirty) return 0;
    for (i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type == RNN) {           /* the three sub-layers' weights, biases, scales and rolling statistics */
            int k;
            for (k = 0; k < 3; ++k) {
                const layer *s = rnn_sub(l, k);
                if (y2_train_pull(net, i, Y2_TRAIN_SUB(k, Y2_TRAIN_WEIGHTS), s->weights, (size_t)s->outputs * s->inputs) != 0 ||
                    y2_train_pull(net, i, Y2_TRAIN_SUB(k, Y2_TRAIN_BIASES), s->biases, s->outputs) != 0) return -1;
                if (s->batch_normalize &&
                    (y2_train_pull(net, i, Y2_TRAIN_SUB(k, Y2_TRAIN_SCALES), s->scales, s->outputs) != 0 ||
                     y2_train_pull(net, i, Y2_TRAIN_SUB(k, Y2_TRAIN_ROLLING_MEAN), s->rolling_mean, s->outputs) != 0 ||
                     y2_train_pull(net, i, Y2_TRAIN_SUB(k, Y2_TRAIN_ROLLING_VARIANCE), s->rolling_variance, s->outputs) != 0)) return -1;
            }
            continue;
        }
        if (l->type != CONVOLUTIONAL && l->type != CONNECTED) continue;
        if (y2_train_pull(net, i, Y2_TRAIN_WEIGHTS, l->weights, (size_t)l->n * l->c * l->size * l->size) != 0 ||
            y2_train_pull(net, i, Y2_TRAIN_BIASES, l->biases, l->n) != 0) return -1;
        if (l->batch_normalize &&
            (y2_train_pull(net, i, Y2_TRAIN_SCALES, l->scales, l->n) != 0 || y2_train_pull(net, i, Y2_TRAIN_ROLLING_MEAN, l->rolling_mean, l->n) != 0 ||
             y2_train_pull(net, i, Y2_TRAIN_ROLLING_VARIANCE, l->rolling_variance, l->n) != 0)) return -1;
    }
    t->dirty = 0;
    e->weights_dirty = 1;
    e->weights_gen++;
    e->weights_external = 0;
    return 0;
}

int y2_train_sync(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (!e || !e->trainer) { y2_fail("y2_train_sync: no trainer (y2_train_prepare)"); return -1; }
    if (y2_train_sync_if_dirty(net) != 0) return -1;
    if (e->built && e->weights_dirty && y2_upload_weights(net) != 0) return -1;
    return 0;
}
