/*
 * The weight arena: all weights of a network in ONE device allocation, in kernel layout ([n][kh][kw][c] filters + the
 * per-filter epilogue constants), so that a multi-GPU launcher replicates the model with a single broadcast.
 * This file lays the arena out, signs the layout, packs the host weights into it and hands it to such a launcher.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"
#include "y2_wino_rule.h"
#include "y2_winos_rule.h"
#include "y2_splitd_rule.h"
#include "y2_split_rule.h"

/* the layer types that own arena space: layout, signature and packing all iterate with this */
static int owns_arena(const layer *l)
{
    return l->type == CONVOLUTIONAL || l->type == CONNECTED || l->type == LOCAL || l->type == BATCHNORM || is_recurrent(l);
}

/* the batch-norm constants of n filters: mean, scale, and the reciprocal divisor in double */
void y2_bn_slots(size_t *off, int n, size_t *mean, size_t *scale, size_t *rinv)
{
    *mean = *off; *off = align_up(*off + n * sizeof(float), 64);
    *scale = *off; *off = align_up(*off + n * sizeof(float), 64);
    *rinv = *off; *off = align_up(*off + n * sizeof(double), 64);
}

/* blas.c:122: x / (sqrt(variance) + .000001f), the divisor evaluated in double */
void y2_fill_rinv(double *dst, const float *var, int n)
{
    int f;
    for (f = 0; f < n; ++f) dst[f] = 1.0 / (sqrt((double)var[f]) + (double).000001f);
}

/* binarize_weights, convolutional_layer.c:37-50: +-mean|w| per filter, sequential fp32 sum */
static float xnor_filter_mean(const float *w, int K)
{
    float bmean = 0;
    int q;
    for (q = 0; q < K; ++q) bmean += fabs(w[q]);
    return bmean / K;
}

/* fp32 -> IEEE half, round to nearest even (what the device's v_cvt_f16_f32 does) */
static unsigned short f32_to_f16_rne(float f)
{
    unsigned int x, sign, mant;
    int exp;
    memcpy(&x, &f, sizeof x);
    sign = (x >> 16) & 0x8000u;
    exp = (int)((x >> 23) & 0xff) - 127 + 15;
    mant = x & 0x7fffffu;
    if (((x >> 23) & 0xff) == 0xff) return (unsigned short)(sign | 0x7c00u | (mant ? 0x200u : 0));   /* inf / nan */
    if (exp >= 31) return (unsigned short)(sign | 0x7c00u);                                          /* overflow */
    if (exp <= 0) {                                                                                  /* subnormal / zero */
        unsigned int shift, half, rem;
        if (exp < -10) return (unsigned short)sign;
        mant |= 0x800000u;
        shift = (unsigned int)(14 - exp);
        half = mant >> shift;
        rem = mant & ((1u << shift) - 1);
        if (rem > (1u << (shift - 1)) || (rem == (1u << (shift - 1)) && (half & 1))) ++half;
        return (unsigned short)(sign | half);
    }
    {
        unsigned int half = ((unsigned int)exp << 10) | (mant >> 13), rem = mant & 0x1fffu;
        if (rem > 0x1000u || (rem == 0x1000u && (half & 1))) ++half;      /* may carry into the exponent: correct */
        return (unsigned short)(sign | half);
    }
}

/* lay the arena out for the current plan (which conv runs on the matrix cores is already decided): every owner's offsets,
 * and the total in arena_need */
void y2_arena_layout(network *net)
{
    y2_engine *e = y2_engine_of(net);
    size_t off = 0;
    int i;
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        y2_ldev *d = ld_of(l);
        const size_t wbytes = (size_t)l->n * l->size * l->size * l->c * sizeof(float);
        const int w_half = y2_half_weights(net, i);
        const y2_conv_form *form;
        if (!owns_arena(l)) continue;
        if (l->type == BATCHNORM) { y2_bn_slots(&off, l->c, &d->off_mean, &d->off_scale, &d->off_rinv); continue; }
        if (is_recurrent(l)) { off = y2_rec_layout(d, l, off); continue; }
        if (l->type == LOCAL) {
            d->off_w_packed = off; off = align_up(off + (size_t)l->out_h * l->out_w * l->n * l->size * l->size * l->c * (w_half ? 2 : sizeof(float)), 256);
            d->off_bias = off; off = align_up(off + (size_t)l->outputs * sizeof(float), 64);
            continue;
        }
        /* a Winograd layer keeps its form's U in place of its nine packed taps (y2_conv_forms) */
        form = &y2_conv_forms[d->form];
        d->off_w_packed = off; off = align_up(off + (form->slot_bytes ? form->slot_bytes(l) : w_half ? wbytes / 2 : wbytes), 256);
        if (d->has_w_ref) { d->off_w_ref = off; off = align_up(off + wbytes, 256); }
        d->off_bias = off; off = align_up(off + l->n * sizeof(float), 64);
        if (w_half) {
            d->off_alpha = off; off = align_up(off + l->n * sizeof(float), 64);
            d->off_beta = off; off = align_up(off + l->n * sizeof(float), 64);
        }
        if (l->batch_normalize) y2_bn_slots(&off, l->n, &d->off_mean, &d->off_scale, &d->off_rinv);
    }
    e->arena_need = off;
}

/* FNV-1a over every per-layer offset and form flag.  Ranks built from different commits of one job compare it: the
 * mixing order and the inputs are part of the format. */
static uint64_t arena_signature(const network *net)
{
    const y2_engine *e = y2_engine_of(net);
    uint64_t sig = 1469598103934665603ull;
    int i, k;
#define SIG_MIX(v) do { uint64_t v_ = (uint64_t)(v); int b_; for (b_ = 0; b_ < 8; ++b_) { sig ^= (v_ >> (8 * b_)) & 0xff; sig *= 1099511628211ull; } } while (0)
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const y2_ldev *d = ld_of(l);
        uint64_t sig_form;
        if (!owns_arena(l)) continue;
        if (is_recurrent(l)) {
            for (k = 0; k < 3; ++k) { SIG_MIX(i); SIG_MIX(d->rd[k].off_w); SIG_MIX(d->rd[k].off_bias); SIG_MIX(d->rd[k].bn ? d->rd[k].off_rinv + 1 : 0); }
            continue;
        }
        SIG_MIX(i); SIG_MIX(d->off_w_packed); SIG_MIX(d->has_w_ref ? d->off_w_ref + 1 : 0); SIG_MIX(d->off_bias);
        SIG_MIX(d->uses_mfma); SIG_MIX(y2_half_weights(net, i));
        SIG_MIX(l->batch_normalize ? d->off_rinv + 1 : 0);
        sig_form = y2_conv_forms[d->form].sig;
        if (sig_form) SIG_MIX(sig_form);       /* the filter slot holds a form's U, not the packed taps (mixed only where it does) */
    }
    SIG_MIX(e->strict); SIG_MIX(e->half); SIG_MIX(e->arena_need);
#undef SIG_MIX
    return sig;
}

/* The packed arena is only valid for the layout it was filled for: a re-plan may move a layer between the
 * matrix-core and the reference-layout form, or switch the weights to half, without changing the total size. */
int y2_arena_commit(network *net)
{
    y2_engine *e = y2_engine_of(net);
    const uint64_t sig = arena_signature(net);
    const int had_layout = e->arena_sig != 0;
    if (e->arena_need != e->arena_bytes || !e->arena) {
        if (e->arena) y2h_free(e->arena);
        e->arena = NULL;
        e->arena_bytes = e->arena_need;
        HIP_OR_ERR(y2h_malloc((void **)&e->arena, e->arena_need));
        e->arena_sig = 0;
    }
    if (sig == e->arena_sig) return 0;
    if (e->weights_external && had_layout) {
        /* a replicated rank holds no host weights to re-pack from: silently keeping (or re-uploading zeros
         * over) an arena of another layout would compute garbage */
        e->weights_external = 0;
        y2_fail("the weight arena was filled from outside (y2_weights_resident) for another plan "
                "(strict / fp16 / fusion / size changed its layout): call y2_weights_arena() again and replicate the "
                "weights for the new plan");
        return -1;
    }
    if (!e->weights_external) e->weights_dirty = 1;
    e->arena_sig = sig;
    return 0;
}

/* reference: weights [location][filter][c][kh][kw], biases [filter][location] (local_layer.c:100,111-121);
 * kernel: weights [location][filter][kh][kw][c] in fp32 or half, biases [location][filter] in fp32 */
static void pack_local(unsigned char *host, const y2_ldev *d, const layer *l, int w_half)
{
    const int locations = l->out_h * l->out_w, kk = l->size * l->size, K = kk * l->c;
    float *wp = (float *)(host + d->off_w_packed), *b = (float *)(host + d->off_bias);
    int loc, co, ci, t;
    for (loc = 0; loc < locations; ++loc)
        for (co = 0; co < l->n; ++co) {
            const float *src = l->weights + ((size_t)loc * l->n + co) * K;
            float *dst = wp + ((size_t)loc * l->n + co) * K;
            for (ci = 0; ci < l->c; ++ci)
                for (t = 0; t < kk; ++t) {
                    if (w_half) ((unsigned short *)wp)[((size_t)loc * l->n + co) * K + (size_t)t * l->c + ci] = f32_to_f16_rne(src[(size_t)ci * kk + t]);
                    else dst[(size_t)t * l->c + ci] = src[(size_t)ci * kk + t];
                }
            b[(size_t)loc * l->n + co] = l->biases[(size_t)co * locations + loc];
        }
}

/* the filters of a [convolutional] or [connected] layer in kernel layout, fp32 or half */
static void pack_filters(float *wp, const network *net, int i, int w_half)
{
    const layer *l = &net->layers[i];
    const int K = l->size * l->size * l->c;
    int co, ci, kh, kw;
    if (l->type == CONNECTED) {
        /* [outputs][inputs]: the reference flattens an image producer as [c][y][x], our activations are
         * [y][x][c], so input k = c*HW + p moves to p*C + c; a flat producer keeps its order */
        const layer *pl = i > 0 ? &net->layers[y2_producer_of(net, i)] : NULL;
        const int hw = (pl && !y2_is_flat(net, y2_producer_of(net, i))) ? pl->out_h * pl->out_w : 1;
        const int C = K / (hw > 0 ? hw : 1);
        int pix;
        for (co = 0; co < l->n; ++co)
            for (ci = 0; ci < C; ++ci)
                for (pix = 0; pix < hw; ++pix) {
                    const size_t dst = (size_t)co * K + (size_t)pix * C + ci;
                    const float v = l->weights[(size_t)co * K + (size_t)ci * hw + pix];
                    if (w_half) ((unsigned short *)wp)[dst] = f32_to_f16_rne(v);
                    else wp[dst] = v;
                }
        return;
    }
    /* reference layout [n][c][kh][kw] (im2col.c:24-27) -> kernel layout [n][kh][kw][c] */
    for (co = 0; co < l->n; ++co) {
        const float bmean = l->xnor ? xnor_filter_mean(l->weights + (size_t)co * K, K) : 0;
        for (ci = 0; ci < l->c; ++ci)
            for (kh = 0; kh < l->size; ++kh)
                for (kw = 0; kw < l->size; ++kw) {
                    const size_t dst = (size_t)co * K + (size_t)(kh * l->size + kw) * l->c + ci;
                    float v = l->weights[(((size_t)co * l->c + ci) * l->size + kh) * l->size + kw];
                    if (l->xnor) v = (v > 0) ? bmean : -bmean;
                    if (w_half) ((unsigned short *)wp)[dst] = f32_to_f16_rne(v);
                    else wp[dst] = v;
                }
    }
}

/* the filters of a Winograd layer: U[g][n][c] = component g of G g G^T of filter n, channel c (y2_wino_filter: evaluated
 * in double, rounded once), each component in the [n][c] layout the 1x1 matrix-core tiles read.  Reference layout
 * [n][c][3][3] (im2col.c:24-27). */
static void pack_wino(void *slot, const layer *l)
{
    const size_t comp = (size_t)l->n * l->c;
    float *up = slot;
    int co, ci, g;
    for (co = 0; co < l->n; ++co)
        for (ci = 0; ci < l->c; ++ci) {
            float u[16];
            y2_wino_filter(l->weights + ((size_t)co * l->c + ci) * 9, u);
            for (g = 0; g < 16; ++g) up[g * comp + (size_t)co * l->c + ci] = u[g];
        }
}

/* the filters of a stationary-Winograd layer: the same U = G g G^T (y2_wino_filter), each value where the kernel's wave
 * (filter tile, component row) and lane load it as part of one 16-byte register (y2_winos_u_index); filters past n in the
 * last 32-filter tile are zero */
static void pack_winos(void *slot, const layer *l)
{
    float *up = slot;
    int co, ci, g;
    memset(up, 0, y2_winos_u_floats(l->n) * sizeof(float));
    for (co = 0; co < l->n; ++co)
        for (ci = 0; ci < l->c; ++ci) {
            float u[16];
            y2_wino_filter(l->weights + ((size_t)co * l->c + ci) * 9, u);
            for (g = 0; g < 16; ++g) up[y2_winos_u_index(co, ci, g >> 2, g & 3)] = u[g];
        }
}

/* the filters of a split-Winograd layer: U as three bf16 planes (y2_split_rule.h), from the reference layout [n][c][3][3] */
static void pack_winox(void *slot, const layer *l) { y2_split_pack_u(slot, l->weights, l->n, l->c); }

/* the filters of a direct split layer: three bf16 planes of the reference-layout weights themselves, one run per (filter
 * tile, K-tile, tap) (y2_splitd_rule.h) */
static void pack_splitd(void *slot, const layer *l) { y2_splitd_pack_u(slot, l->weights, l->n, l->c, y2_splitd_bn(l->n, ld_of(l)->fused_pool)); }

static size_t wino_slot_bytes(const layer *l) { return (size_t)16 * l->n * l->c * sizeof(float); }
static size_t winox_slot_bytes(const layer *l) { return y2_split_bytes(y2_split_rows_pad(l->n), l->c); }
static size_t winos_slot_bytes(const layer *l) { return y2_winos_u_floats(l->n) * sizeof(float); }
static size_t splitd_slot_bytes(const layer *l) { return y2_splitd_u_elems(l->n, l->c, y2_splitd_bn(l->n, ld_of(l)->fused_pool)) * 2; }

/* the signature constants are part of the signature's format (arena_signature) */
const y2_conv_form y2_conv_forms[Y2_FORM_COUNT] = {
    [Y2_FORM_DIRECT] = { 0, NULL, NULL, y2h_conv_workspace_bytes, NULL },
    [Y2_FORM_WINO] = { 0x57494e4f, wino_slot_bytes, pack_wino, y2h_wino_workspace_bytes, y2h_conv_wino_forward },          /* V and M */
    [Y2_FORM_WINOX] = { 0x57494e58, winox_slot_bytes, pack_winox, y2h_wino_split_workspace_bytes, y2h_conv_winox_forward },
    [Y2_FORM_WINOS] = { 0x57494e53, winos_slot_bytes, pack_winos, NULL, y2h_conv_winos_forward },
    [Y2_FORM_SPLITD] = { 0x53504c44, splitd_slot_bytes, pack_splitd, NULL, y2h_conv_splitd_forward },
};

/* a [convolutional] or [connected] layer: filters, the reference-layout copy where the layer needs one, constants */
static void pack_dense(unsigned char *host, const network *net, int i)
{
    const layer *l = &net->layers[i];
    const y2_ldev *d = ld_of(l);
    const y2_conv_form *form = &y2_conv_forms[d->form];
    const int K = l->size * l->size * l->c, w_half = y2_half_weights(net, i);
    int co, f, q;
    if (form->pack) form->pack(host + d->off_w_packed, l);
    else pack_filters((float *)(host + d->off_w_packed), net, i, w_half);
    if (w_half) {
        /* folded batch-norm for the fp16 kernels: y = act(acc*alpha + beta), constants evaluated in double */
        float *al = (float *)(host + d->off_alpha), *be = (float *)(host + d->off_beta);
        for (f = 0; f < l->n; ++f) {
            double a = 1.0, bb = l->biases[f];
            if (l->batch_normalize) {
                a = (double)l->scales[f] / (sqrt((double)l->rolling_variance[f]) + (double).000001f);
                bb = (double)l->biases[f] - (double)l->rolling_mean[f] * a;
            }
            al[f] = (float)a; be[f] = (float)bb;
        }
    }
    if (d->has_w_ref) memcpy(host + d->off_w_ref, l->weights, (size_t)l->n * K * sizeof(float));
    if (d->has_w_ref && l->type == CONVOLUTIONAL && l->xnor) {
        float *wr = (float *)(host + d->off_w_ref);
        for (co = 0; co < l->n; ++co) {
            const float bmean = xnor_filter_mean(l->weights + (size_t)co * K, K);
            for (q = 0; q < K; ++q) wr[(size_t)co * K + q] = (l->weights[(size_t)co * K + q] > 0) ? bmean : -bmean;
        }
    }
    memcpy(host + d->off_bias, l->biases, l->n * sizeof(float));
    if (l->batch_normalize) {
        memcpy(host + d->off_mean, l->rolling_mean, l->n * sizeof(float));
        memcpy(host + d->off_scale, l->scales, l->n * sizeof(float));
        y2_fill_rinv((double *)(host + d->off_rinv), l->rolling_variance, l->n);
    }
}

int y2_upload_weights(network *net)
{
    y2_engine *e = y2_engine_of(net);
    /* pinned staging: no pageable buffer of ours is ever handed to an asynchronous copy */
    unsigned char *host = NULL;
    int i;
    if (y2h_host_alloc((void **)&host, e->arena_bytes ? e->arena_bytes : 16) != 0) host = NULL;
    if (!host) { y2_fail("weight upload: no pinned host memory for %zu bytes: %s", e->arena_bytes, y2h_last_error()); return -1; }
    memset(host, 0, e->arena_bytes ? e->arena_bytes : 16);
    for (i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        const y2_ldev *d = ld_of(l);
        if (!owns_arena(l)) continue;
        if (is_recurrent(l)) y2_rec_pack(host, d, l);
        else if (l->type == BATCHNORM) {
            memcpy(host + d->off_mean, l->rolling_mean, l->c * sizeof(float));
            memcpy(host + d->off_scale, l->scales, l->c * sizeof(float));
            y2_fill_rinv((double *)(host + d->off_rinv), l->rolling_variance, l->c);
        }
        else if (l->type == LOCAL) pack_local(host, d, l, y2_half_weights(net, i));
        else pack_dense(host, net, i);
    }
    if (y2h_memcpy_h2d(e->arena, host, e->arena_bytes, e->stream) != 0 || y2h_stream_sync(e->stream) != 0) {
        y2h_host_free(host);
        y2_fail("weight upload failed: %s", y2h_last_error());
        return -1;
    }
    y2h_host_free(host);
    e->weights_dirty = 0;
    return 0;
}

int y2_weights_arena(network *net, void **dev_ptr, size_t *bytes)
{
    y2_engine *e;
    int keep, trained;
    if (!y2_engine_of(net)) return -1;
    e = y2_engine_of(net);
    trained = y2_train_is_dirty(net);
    if (y2_train_sync_if_dirty(net) != 0) return -1;
    /* building must not try to upload host weights that were never loaded */
    keep = e->weights_dirty;
    if (!e->built || e->built_strict != e->strict || e->built_half != e->half || e->built_fusion != e->fusion ||
        e->built_batch != net->batch || e->built_w != net->w || e->built_h != net->h) {
        /* (re-)requesting the arena: whatever layout it had before no longer binds */
        e->weights_external = 1; e->arena_sig = 0;
        e->arena_pending = 1;                /* this build uploads nothing: the arena is uninitialised HBM until it is filled from outside */
        if (y2_engine_build(net) != 0) { e->weights_external = 0; e->arena_pending = 0; return -1; }
        e->weights_external = 0; e->weights_dirty = keep;
    }
    if (trained) {                           /* after training steps the arena handed out holds what was trained */
        if (y2_upload_weights(net) != 0) return -1;
        e->arena_pending = 0;
    }
    if (dev_ptr) *dev_ptr = e->arena;
    if (bytes) *bytes = e->arena_bytes;
    return 0;
}

void y2_weights_resident(network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (e) { e->weights_external = 1; e->weights_dirty = 0; e->arena_pending = 0; }
}
