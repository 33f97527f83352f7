/*
 * [rnn] / [gru]: the host half of the recurrent layers -- the three dense blocks a layer is packed into, the form each
 * block runs in, the layer's buffers and its forward.  The kernels are in y2_recurrent.hip.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

/* A forward of T steps over B sequences:
 *   1. every step's input projection in ONE dense product over the T*B input rows (rnn: input layer; gru: input z|r|h as
 *      one product of 3*outputs columns) into d_proj;
 *   2. the step loop (skinny / reference-order forms; the matrix-core form adds its product launch in front of each) --
 *      rnn: one launch per step (self product + the state combine), writing the step's state into
 *      d_hist[t] (a second buffer: every column reads the whole previous state); gru: launch A reads the state and writes
 *      z and f = state*r, launch B reads f and column j of the state and writes column j in place;
 *   3. rnn: the output layer as ONE dense product over the T states in d_hist.
 * The state lives in d_state at the end of every forward whatever T is: a recorded graph reads it there at its next
 * replay.  Each row goes through the same per-row arithmetic whichever of the forms below runs it. */
int y2_rec_hidden(const layer *l) { return l->type == RNN ? l->hidden : l->outputs; }

/* the sub-layers of block k, stacked by rows */
static int rec_subs(const layer *l, int k, const layer **s)
{
    if (l->type == RNN) { s[0] = k == 0 ? l->input_layer : (k == 1 ? l->self_layer : l->output_layer); return 1; }
    if (k == 0) { s[0] = l->input_z_layer; s[1] = l->input_r_layer; s[2] = l->input_h_layer; return 3; }
    if (k == 1) { s[0] = l->state_z_layer; s[1] = l->state_r_layer; return 2; }
    s[0] = l->state_h_layer;
    return 1;
}

size_t y2_rec_layout(y2_ldev *d, const layer *l, size_t off)
{
    int k;
    for (k = 0; k < 3; ++k) {
        const layer *s[3];
        const int m = rec_subs(l, k, s);
        d->rd[k].n = s[0]->outputs * m; d->rd[k].k = s[0]->inputs;
        d->rd[k].bn = s[0]->batch_normalize; d->rd[k].act = s[0]->activation;
        d->rd[k].off_w = off; off = align_up(off + (size_t)d->rd[k].n * d->rd[k].k * sizeof(float), 256);
        d->rd[k].off_bias = off; off = align_up(off + d->rd[k].n * sizeof(float), 64);
        if (d->rd[k].bn) y2_bn_slots(&off, d->rd[k].n, &d->rd[k].off_mean, &d->rd[k].off_scale, &d->rd[k].off_rinv);
    }
    return off;
}

void y2_rec_pack(unsigned char *host, const y2_ldev *d, const layer *l)
{
    int k, m;
    for (k = 0; k < 3; ++k) {
        const layer *s[3];
        const int subs = rec_subs(l, k, s), K = d->rd[k].k;
        for (m = 0; m < subs; ++m) {
            const int n = s[m]->outputs, o = m * n;
            memcpy(host + d->rd[k].off_w + (size_t)o * K * sizeof(float), s[m]->weights, (size_t)n * K * sizeof(float));
            memcpy(host + d->rd[k].off_bias + o * sizeof(float), s[m]->biases, n * sizeof(float));
            if (d->rd[k].bn) {
                memcpy(host + d->rd[k].off_mean + o * sizeof(float), s[m]->rolling_mean, n * sizeof(float));
                memcpy(host + d->rd[k].off_scale + o * sizeof(float), s[m]->scales, n * sizeof(float));
                y2_fill_rinv((double *)(host + d->rd[k].off_rinv) + o, s[m]->rolling_variance, n);
            }
        }
    }
}

static void rec_args(const y2_engine *e, const y2_ldev *d, int k, const float *x, int rows, y2h_rec_args *a)
{
    memset(a, 0, sizeof *a);
    a->x = x; a->rows = rows; a->k = d->rd[k].k; a->n = d->rd[k].n;
    a->w = (const float *)(e->arena + d->rd[k].off_w);
    a->bias = (const float *)(e->arena + d->rd[k].off_bias);
    a->bn = d->rd[k].bn; a->act = y2_act_code(d->rd[k].act);
    if (a->bn) {
        a->mean = (const float *)(e->arena + d->rd[k].off_mean);
        a->scale = (const float *)(e->arena + d->rd[k].off_scale);
        a->rinv = (const double *)(e->arena + d->rd[k].off_rinv);
    }
}

/* block k as a [connected] layer over `rows` flat rows: a 1x1 convolution over a 1x1 image */
static void rec_conv_desc(const y2_engine *e, const y2_ldev *d, int k, const float *x, int rows, float *y, y2h_conv *c)
{
    memset(c, 0, sizeof *c);
    c->batch = rows; c->h = 1; c->w = 1; c->c = d->rd[k].k; c->ldx = d->rd[k].k;
    c->n = d->rd[k].n; c->size = 1; c->stride = 1; c->pad = 0; c->out_h = 1; c->out_w = 1; c->ldy = d->rd[k].n;
    c->batch_normalize = d->rd[k].bn;
    c->activation = y2_act_for_kernel(d->rd[k].act);
    c->x = x; c->y = y;
    c->ws = e->d_ws; c->ws_bytes = e->ws_bytes;
    c->w_packed = e->arena ? (const float *)(e->arena + d->rd[k].off_w) : Y2_ALIGNED_STANDIN;
    c->w_ref = c->w_packed;               /* a flat input: the packed layout is the reference's [n][k] */
    if (e->arena) {
        c->bias = (const float *)(e->arena + d->rd[k].off_bias);
        if (c->batch_normalize) {
            c->mean = (const float *)(e->arena + d->rd[k].off_mean);
            c->scale = (const float *)(e->arena + d->rd[k].off_scale);
            c->rinv = (const double *)(e->arena + d->rd[k].off_rinv);
        }
    }
}

/* The one place that decides how block k of a recurrent layer runs over `rows` rows, once per plan: in strict mode the
 * reference-order kernel; otherwise the skinny weight-streaming kernel while the rows fit it, above that the fp32
 * matrix-core [connected] path where its kernels take the shape (the plan's own buffers are aligned; a caller's input is
 * copied into an aligned one, y2_enqueue_forward), and the reference-order kernel where they do not.
 * Y2_RNN_STEP=skinny|mfma forces the step's blocks (a forced skinny step that does not fit is refused: -1). */
static int rec_form(const y2_engine *e, const y2_ldev *d, int k, int rows, int step)
{
    const char *f = step ? getenv("Y2_RNN_STEP") : NULL;
    y2h_conv c;
    if (e->strict) return Y2_REC_REF;
    if (f && strcmp(f, "skinny") == 0) return y2h_rec_skinny_ok(rows, d->rd[k].k) ? Y2_REC_SKINNY : -1;
    if (!(f && strcmp(f, "mfma") == 0) && y2h_rec_skinny_ok(rows, d->rd[k].k)) return Y2_REC_SKINNY;
    rec_conv_desc(e, d, k, Y2_ALIGNED_STANDIN, rows, Y2_ALIGNED_STANDIN, &c);
    c.w_packed = c.w_ref = Y2_ALIGNED_STANDIN;
    return y2h_conv_uses_mfma(&c) ? Y2_REC_MFMA : Y2_REC_REF;
}

/* what runs: rec_skinny_kernel, the matrix-core [connected] kernels, or rec_ref_kernel */
static const char *rec_form_name(int f) { return f == Y2_REC_REF ? "ref" : (f == Y2_REC_SKINNY ? "skinny" : "mfma"); }

/* block k runs in the step loop over B rows, or hoisted over all B*T rows (the input product; the rnn output product) */
static int rec_is_step(const layer *l, int k) { return !(k == 0 || (l->type == RNN && k == 2)); }
static int rec_rows(const layer *l, int k) { return rec_is_step(l, k) ? l->batch : l->batch * l->steps; }

/* y[rows][n] = block k over x[rows][k] in the block's form; xcopy (if set) also receives the x rows */
static int rec_dense(y2_engine *e, const y2_ldev *d, int k, const float *x, int rows, float *y, float *xcopy)
{
    y2h_rec_args a;
    y2h_conv c;
    if (d->rd[k].form != Y2_REC_MFMA) {
        rec_args(e, d, k, x, rows, &a);
        a.mode = Y2H_REC_DENSE; a.out = y; a.xcopy = xcopy;
        HIP_OR_ERR(y2h_rec_step(&a, d->rd[k].form == Y2_REC_SKINNY ? Y2H_REC_SKINNY : Y2H_REC_REF, e->stream));
        return 0;
    }
    rec_conv_desc(e, d, k, x, rows, y, &c);
    HIP_OR_ERR(y2h_conv_forward(&c, 0, e->stream));
    if (y2_activate_after(e, d->rd[k].act, y, d->rd[k].n, rows, d->rd[k].n) != 0) return -1;
    if (xcopy) HIP_OR_ERR(y2h_memcpy_d2d(xcopy, x, (size_t)rows * d->rd[k].k * sizeof(float), e->stream));
    return 0;
}

/* buffers, forms and the kernel name of recurrent layer i; the state starts at zero */
int y2_rec_plan(network *net, int i)
{
    y2_engine *e = y2_engine_of(net);
    layer *l = &net->layers[i];
    y2_ldev *d = ld_of(l);
    const int B = l->batch, T = l->steps, H = y2_rec_hidden(l);
    const size_t rows = (size_t)B * T;
    int k, tmp = 0;
    if (i > 0 && !y2_is_flat(net, y2_producer_of(net, i))) { y2_fail("layer %d (%s) needs a flat input", i, get_layer_string(l->type)); return -1; }
    y2_rec_layout(d, l, 0);                     /* the blocks' shapes (the arena offsets are laid out again with the arena) */
    for (k = 0; k < 3; ++k) {
        const int step = rec_is_step(l, k);
        d->rd[k].form = rec_form(e, d, k, rec_rows(l, k), step);
        if (d->rd[k].form < 0) {
            y2_fail("layer %d (%s): Y2_RNN_STEP=skinny, but %d sequences of %d values do not fit the skinny kernel (at most %d "
                    "rows, 64 KB of rows)", i, get_layer_string(l->type), B, H, Y2H_REC_SKINNY_MAX_ROWS);
            return -1;
        }
        if (step && d->rd[k].form == Y2_REC_MFMA) tmp = 1;
    }
    HIP_OR_ERR(y2h_malloc((void **)&d->d_state, (size_t)B * H * sizeof(float)));
    HIP_OR_ERR(y2h_memset(d->d_state, 0, (size_t)B * H * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_malloc((void **)&d->d_proj, rows * (l->type == GRU ? 3 : 1) * H * sizeof(float)));
    if (l->type == RNN) HIP_OR_ERR(y2h_malloc((void **)&d->d_hist, rows * H * sizeof(float)));
    else HIP_OR_ERR(y2h_malloc((void **)&d->d_zf, (size_t)2 * B * H * sizeof(float)));
    if (tmp) HIP_OR_ERR(y2h_malloc((void **)&d->d_tmp, (size_t)2 * B * H * sizeof(float)));
    HIP_OR_ERR(y2h_malloc((void **)&d->out_alloc, rows * l->outputs * sizeof(float)));
    d->out = d->out_alloc; d->out_ld = l->outputs;
    if (l->type == RNN)
        snprintf(d->kname, sizeof d->kname, "rnn(input:%s step:%s output:%s)", rec_form_name(d->rd[0].form),
                 rec_form_name(d->rd[1].form), rec_form_name(d->rd[2].form));
    else
        snprintf(d->kname, sizeof d->kname, "gru(input:%s step:%s+%s)", rec_form_name(d->rd[0].form), rec_form_name(d->rd[1].form),
                 rec_form_name(d->rd[2].form));
    d->kernel = d->kname;
    return 0;
}

/* split-K scratch the matrix-core forms of the recurrent products ask for */
size_t y2_rec_workspace_bytes(const network *net)
{
    const y2_engine *e = y2_engine_of(net);
    size_t need = 0, b;
    int i, k;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const y2_ldev *d = ld_of(l);
        y2h_conv c;
        if (!is_recurrent(l)) continue;
        for (k = 0; k < 3; ++k) {
            if (d->rd[k].form != Y2_REC_MFMA) continue;
            rec_conv_desc(e, d, k, Y2_ALIGNED_STANDIN, rec_rows(l, k), Y2_ALIGNED_STANDIN, &c);
            b = y2h_conv_workspace_bytes(&c);
            if (b > need) need = b;
        }
    }
    return need;
}

/* one step's block k: the skinny or reference-order kernel computes the product and the combine in one launch; the
 * matrix-core form writes the product to d_tmp and the reference-order kernel combines */
static int rec_step(y2_engine *e, const y2_ldev *d, int k, y2h_rec_args *a)
{
    if (d->rd[k].form == Y2_REC_MFMA) {
        if (rec_dense(e, d, k, a->x, a->rows, d->d_tmp, NULL) != 0) return -1;
        a->pre = d->d_tmp;
    }
    HIP_OR_ERR(y2h_rec_step(a, d->rd[k].form == Y2_REC_SKINNY ? Y2H_REC_SKINNY : Y2H_REC_REF, e->stream));
    return 0;
}

int y2_rec_forward(network *net, int i, const float *x)
{
    y2_engine *e = y2_engine_of(net);
    layer *l = &net->layers[i];
    y2_ldev *d = ld_of(l);
    const int B = l->batch, T = l->steps, H = y2_rec_hidden(l);
    const size_t bh = (size_t)B * H;
    y2h_rec_args a;
    int t;
    if (rec_dense(e, d, 0, x, B * T, d->d_proj, NULL) != 0) return -1;
    for (t = 0; t < T; ++t) {
        if (l->type == RNN) {
            const float *prev = t == 0 ? d->d_state : d->d_hist + (t - 1) * bh;
            rec_args(e, d, 1, prev, B, &a);
            a.mode = Y2H_REC_RNN; a.h = H; a.shortcut = l->shortcut;
            a.proj = d->d_proj + t * bh; a.state = prev;
            a.out = d->d_hist + t * bh;
            a.out2 = (t == T - 1 && T > 1) ? d->d_state : NULL;     /* the last step reads d_hist[T-2], not d_state */
            if (rec_step(e, d, 1, &a) != 0) return -1;
        } else {
            float *z = d->d_zf, *f = d->d_zf + bh;
            rec_args(e, d, 1, d->d_state, B, &a);
            a.mode = Y2H_REC_GRU_ZR; a.h = H;
            a.proj = d->d_proj + t * 3 * bh; a.state = d->d_state;
            a.out = z; a.out2 = f;
            if (rec_step(e, d, 1, &a) != 0) return -1;
            rec_args(e, d, 2, f, B, &a);
            a.mode = Y2H_REC_GRU_H; a.h = H;
            a.proj = d->d_proj + t * 3 * bh; a.state = d->d_state; a.z = z;
            a.out = d->d_state; a.out2 = d->out + t * bh;
            if (rec_step(e, d, 2, &a) != 0) return -1;
        }
    }
    /* rnn: the output product over the T states; at T = 1 the one step could not write d_state (every workgroup reads it),
     * so this launch, which reads d_hist[0] anyway, also copies it there */
    if (l->type == RNN && rec_dense(e, d, 2, d->d_hist, B * T, d->out, T == 1 ? d->d_state : NULL) != 0) return -1;
    return 0;
}
