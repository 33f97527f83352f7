/* y2_tta.c -- the reference's multi-view classifier evaluation (classifier.c), views built on the device.
 *
 *   validate_classifier_10      classifier.c:336-406   -> Y2_VIEWS_CROP10, y2_validate_classifier_10_frames
 *   validate_classifier_multi   classifier.c:531-593   -> Y2_VIEWS_MULTI,  y2_validate_classifier_multi_frames
 *   validate_classifier_full    classifier.c:408-466   -> Y2_VIEWS_FULL,   y2_validate_classifier_full_frames
 *
 * The reference builds every view on the host and predicts it at batch 1.  Here a block of frames goes up once, the
 * resizes (y2h_resize_chw, image.c:1950), the windows and mirror images (y2h_views_to_input: crop_image image.c:1512,
 * flip_image image.c:1056) and the additions (y2h_accumulate_rows: axpy_cpu, classifier.c:393,577,580) run on the
 * engine's stream around forwards of net.batch views, and the block's sums come down in one copy.  The rules of the
 * three modes are stated in include/sr_yolo2.h.
 *
 * Order of work inside a block ("size-major"): the modes that resize the network walk the scales in the caller's order
 * and, inside a scale, the distinct resized sizes in order of first appearance; the network is resized once per such
 * size and all views of that size run before the next.  One image has one size per scale, so its accumulator still
 * receives scale 0's unflipped view, scale 0's flipped view, scale 1's unflipped view, ... exactly as the reference's
 * image-major loop adds them, while the plan is rebuilt once per distinct size instead of once per image and scale.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

static const int default_scales[] = {224, 288, 320, 352, 384};      /* classifier.c:550 */
static const int crop_shift = 32;                                   /* classifier.c:375 */
/* the ten windows of validate_classifier_10 in its order (classifier.c:378-388): five of the frame, five of its mirror
 * image.  (0,0) is the top-left window of the (w+32) x (h+32) frame, not its centre; the others reach 32 pixels past an
 * edge and repeat it (constrain_int in crop_image) */
static const int crop_dx[5] = {-32, 32, 0, -32, 32}, crop_dy[5] = {-32, -32, 0, 32, 32};

static size_t block_bytes_override;
static unsigned long view_resizes;

void y2_set_view_block_bytes(size_t bytes) { block_bytes_override = bytes; }
unsigned long y2_view_resizes(void) { return view_resizes; }

static size_t block_budget(void)
{
    const char *env = getenv("Y2_VIEW_BLOCK_BYTES");
    if (block_bytes_override) return block_bytes_override;
    if (env && atoll(env) > 0) return (size_t)atoll(env);
    return Y2_VIEW_BLOCK_BYTES;
}

typedef struct { int w, h; } dims;

/* resize_min's dimensions (image.c:1662-1672), integer arithmetic */
static void resize_min_dims(int w, int h, int min, int *rw, int *rh)
{
    if (w < h) { *rh = (h * min) / w; *rw = min; }
    else { *rw = (w * min) / h; *rh = min; }
}

/* the scale of stage j: none for CROP10, the caller's for MULTI, the network's width on entry for FULL (classifier.c:436) */
static int stage_scale(int mode, const int *scales, int j, int scale_full)
{
    return mode == Y2_VIEWS_MULTI ? scales[j] : (mode == Y2_VIEWS_FULL ? scale_full : 0);
}

/* the size frame f has in front of the crops at stage j: (net.w+32, net.h+32) for CROP10 (load_image_color(path, w+shift,
 * h+shift), classifier.c:376), resize_min(im, scale) for the others */
static void stage_dims(int mode, const image *f, int net_w, int net_h, int scale, int *rw, int *rh)
{
    if (mode == Y2_VIEWS_CROP10) { *rw = net_w + crop_shift; *rh = net_h + crop_shift; }
    else resize_min_dims(f->w, f->h, scale, rw, rh);
}

/* Would resize_network(net, w, h) go through, and leave every layer a positive size?  The walk of network.c:322-388
 * without its side effects.  Returns -1 or the index of the layer that cannot follow. */
static int resize_refused_by(const network *net, int w, int h)
{
    int i, bad = -1;
    dims *out = calloc(net->n, sizeof(dims));
    if (!out) return 0;
    for (i = 0; i < net->n && bad < 0; ++i) {
        const layer *l = &net->layers[i];
        int ow = w, oh = h;
        switch (l->type) {
        case CONVOLUTIONAL: ow = (w + 2 * l->pad - l->size) / l->stride + 1; oh = (h + 2 * l->pad - l->size) / l->stride + 1; break;
        case MAXPOOL: ow = (w + 2 * l->pad) / l->stride; oh = (h + 2 * l->pad) / l->stride; break;
        case CROP: ow = l->scale * w; oh = l->scale * h; break;
        case REORG:
            if (l->reverse) { ow = w * l->stride; oh = h * l->stride; } else { ow = w / l->stride; oh = h / l->stride; }
            break;
        case ROUTE: ow = out[l->input_layers[0]].w; oh = out[l->input_layers[0]].h; break;
        case REGION: case COST: case SOFTMAX: break;
        case AVGPOOL: i = net->n; continue;      /* network.c:366: layers behind an avgpool keep their size */
        default: bad = i; continue;
        }
        if (ow <= 0 || oh <= 0) bad = i;
        out[i].w = w = ow; out[i].h = h = oh;
    }
    free(out);
    return bad;
}

static int views_check(const char *who, const network *net, int mode, const image *frames, int n, const int *scales,
                       int nscales, const float *sums)
{
    int i, j;
    char why[256];
    if (!net || !net->layers || net->n <= 0) { y2_fail("%s: net is NULL or empty", who); return -1; }
    if (mode != Y2_VIEWS_CROP10 && mode != Y2_VIEWS_MULTI && mode != Y2_VIEWS_FULL) { y2_fail("%s: mode %d is none of Y2_VIEWS_CROP10 / _MULTI / _FULL", who, mode); return -1; }
    if (n <= 0) { y2_fail("%s: n = %d frames", who, n); return -1; }
    if (!frames) { y2_fail("%s: frames is NULL", who); return -1; }
    if (!sums) { y2_fail("%s: sums is NULL", who); return -1; }
    if (scales && nscales <= 0) { y2_fail("%s: nscales = %d with a scale list", who, nscales); return -1; }
    if (scales) for (j = 0; j < nscales; ++j) if (scales[j] <= 0) { y2_fail("%s: scales[%d] = %d", who, j, scales[j]); return -1; }
    if (net->hierarchy && y2_hierarchy_refusal(net, why, sizeof why)) { y2_fail("%s: %s", who, why); return -1; }
    for (i = 0; i < net->n; ++i)
        if (is_recurrent(&net->layers[i])) { y2_fail("%s: layer %d (%s): a recurrent network has no image views", who, i, get_layer_string(net->layers[i].type)); return -1; }
    if (net->w <= 0 || net->h <= 0 || net->c <= 0 || net->batch <= 0) { y2_fail("%s: the network input must be an image (h, w, c > 0)", who); return -1; }
    for (i = 0; i < n; ++i) {
        const image *f = &frames[i];
        if (!f->data) { y2_fail("%s: frame %d: data is NULL", who, i); return -1; }
        if (f->w <= 0 || f->h <= 0) { y2_fail("%s: frame %d: size %d x %d", who, i, f->w, f->h); return -1; }
        if (f->c < net->c) { y2_fail("%s: frame %d: the frame has %d planes, the network reads %d", who, i, f->c, net->c); return -1; }
    }
    if (mode == Y2_VIEWS_CROP10) return 0;
    {   /* resize_network's own refusal (network.c:383-385), before anything is resized */
        const int bad = resize_refused_by(net, net->w, net->h);
        if (bad >= 0) { y2_fail("%s: layer %d ([%s]) cannot be resized (resize_network)", who, bad, get_layer_string(net->layers[bad].type)); return -1; }
    }
    for (i = 0; i < n; ++i)
        for (j = 0; j < nscales; ++j) {
            const int scale = mode == Y2_VIEWS_FULL ? net->w : (scales ? scales[j] : default_scales[j]);
            int rw, rh, bad;
            resize_min_dims(frames[i].w, frames[i].h, scale, &rw, &rh);
            bad = rw > 0 && rh > 0 ? resize_refused_by(net, rw, rh) : 0;
            if (bad >= 0) { y2_fail("%s: frame %d: at scale %d it is %d x %d, too small for layer %d", who, i, scale, rw, rh, bad); return -1; }
        }
    return 0;
}

static int grow_buffers(y2_engine *e, size_t host_bytes, size_t dev_bytes)
{
    if (host_bytes > e->h_tta_cap) {
        y2h_host_free(e->h_tta); e->h_tta = NULL; e->h_tta_cap = 0;
        HIP_OR_ERR(y2h_host_alloc((void **)&e->h_tta, host_bytes));
        e->h_tta_cap = host_bytes;
    }
    if (dev_bytes > e->d_tta_cap) {
        y2h_free(e->d_tta); e->d_tta = NULL; e->d_tta_cap = 0;
        HIP_OR_ERR(y2h_malloc((void **)&e->d_tta, dev_bytes));
        e->d_tta_cap = dev_bytes;
    }
    return 0;
}

/* One block: frames [first, first+cnt).  Layout of the pinned staging buffer and of the front of the HBM arena:
 * [view table: forwards x batch][owner table: forwards x batch][hierarchy table: forwards x batch, hierarchical networks
 * only][source planes of the frames]; behind it in HBM the current stage's resized copies, the resize scratch and the
 * accumulators.  The hierarchy table is the row mask of y2h_hierarchy_rows: 1 where hierarchy_predictions(.., 1) is applied
 * to the slot's prediction before it is added -- every view of CROP10 (classifier.c:392) and FULL (:453), but of MULTI only
 * the unflipped views (:576): the reference adds the flipped view's prediction as network_predict left it (:579-580). */
static int run_block(network *net, int mode, const image *frames, int first, int cnt, const int *scales, int nstages,
                     int scale_full, int outputs, float *sums, unsigned char *done)
{
    y2_engine *e = y2_engine_of(net);
    const int batch = net->batch, c = net->c, per = mode == Y2_VIEWS_CROP10 ? 10 : (mode == Y2_VIEWS_MULTI ? 2 : 1);
    const int crop_w = net->w, crop_h = net->h;         /* CROP10's window; the other modes' window is the whole image */
    const long forwards_max = ((long)cnt * per + batch - 1) / batch + (long)cnt;   /* every size group may end in a partial forward */
    const size_t slots = (size_t)forwards_max * nstages * batch;
    const int hier = net->hierarchy != NULL;
    const size_t desc_bytes = align_up(slots * sizeof(y2h_view), 256), owner_bytes = align_up(slots * sizeof(int), 256);
    const size_t mask_bytes = hier ? owner_bytes : 0, tables_bytes = desc_bytes + owner_bytes + mask_bytes;
    size_t src_floats = 0, res_floats = 0, tmp_floats = 0, acc_floats = (size_t)cnt * outputs, up_bytes, off;
    size_t *src_off = calloc(cnt, sizeof(size_t)), *res_off = calloc(cnt, sizeof(size_t));
    dims *sz = calloc(cnt, sizeof(dims));
    y2h_view *desc;
    int *owner, *hmask;
    float *d_src, *d_res, *d_tmp, *d_acc;
    size_t slot = 0;
    int i, j, k, v, rc = -1;
    if (!src_off || !res_off || !sz) { y2_fail("out of memory"); goto cleanup; }
    for (i = 0; i < cnt; ++i) {
        const image *f = &frames[first + i];
        src_off[i] = src_floats;
        src_floats += align_up((size_t)c * f->h * f->w, 4);          /* every source starts on a 16-byte boundary */
    }
    for (j = 0; j < nstages; ++j) {
        size_t stage = 0;
        for (i = 0; i < cnt; ++i) {
            const image *f = &frames[first + i];
            int rw, rh;
            stage_dims(mode, f, crop_w, crop_h, stage_scale(mode, scales, j, scale_full), &rw, &rh);
            if (rw == f->w && rh == f->h) continue;
            stage += align_up((size_t)c * rh * rw, 4);
            if ((size_t)c * f->h * rw > tmp_floats) tmp_floats = (size_t)c * f->h * rw;
        }
        if (stage > res_floats) res_floats = stage;
    }
    up_bytes = tables_bytes + src_floats * sizeof(float);
    if (grow_buffers(e, up_bytes, up_bytes + (res_floats + align_up(tmp_floats, 4) + acc_floats) * sizeof(float)) != 0) goto cleanup;
    desc = (y2h_view *)e->h_tta;
    owner = (int *)(e->h_tta + desc_bytes);
    hmask = (int *)(e->h_tta + desc_bytes + owner_bytes);
    d_src = (float *)(e->d_tta + tables_bytes);
    d_res = d_src + src_floats;
    d_tmp = d_res + res_floats;
    d_acc = d_tmp + align_up(tmp_floats, 4);
    memset(e->h_tta, 0, tables_bytes);
    for (i = 0; i < cnt; ++i) {
        const image *f = &frames[first + i];
        memcpy(e->h_tta + tables_bytes + src_off[i] * sizeof(float), f->data, (size_t)c * f->h * f->w * sizeof(float));
    }
    /* pass 1 (host only): the view and owner tables of every forward of the block, in the order pass 2 launches them */
    for (j = 0; j < nstages; ++j) {
        memset(done, 0, cnt);
        off = 0;
        for (i = 0; i < cnt; ++i) {
            const image *f = &frames[first + i];
            stage_dims(mode, f, crop_w, crop_h, stage_scale(mode, scales, j, scale_full), &sz[i].w, &sz[i].h);
            res_off[i] = (size_t)-1;
            if (sz[i].w == f->w && sz[i].h == f->h) continue;
            res_off[i] = off;
            off += align_up((size_t)c * sz[i].h * sz[i].w, 4);
        }
        for (i = 0; i < cnt; ++i) {
            int fill = 0;
            if (done[i]) continue;
            /* the group of frame i: every frame not yet done with its size at this stage (CROP10: all of them) */
            for (k = i; k < cnt; ++k) {
                if (done[k] || sz[k].w != sz[i].w || sz[k].h != sz[i].h) continue;
                for (v = 0; v < per; ++v) {
                    y2h_view *d = &desc[slot];
                    d->src = res_off[k] == (size_t)-1 ? (long long)src_off[k] : (long long)(src_floats + res_off[k]);
                    d->sw = sz[k].w; d->sh = sz[k].h;
                    d->dx = mode == Y2_VIEWS_CROP10 ? crop_dx[v % 5] : 0;
                    d->dy = mode == Y2_VIEWS_CROP10 ? crop_dy[v % 5] : 0;
                    d->flip = mode == Y2_VIEWS_CROP10 ? v >= 5 : v;
                    owner[slot] = k;
                    if (hier) hmask[slot] = !(mode == Y2_VIEWS_MULTI && d->flip);
                    ++slot;
                    if (++fill == batch) fill = 0;
                }
                done[k] = 1;
            }
            for (; fill > 0 && fill < batch; ++fill) owner[slot++] = -1;     /* the group's last forward: unused slots */
        }
    }
    if (slot > slots) { y2_fail("y2_classifier_view_sums: internal error (%zu view slots, %zu planned)", slot, slots); goto cleanup; }
    /* pass 2: one upload, then everything on the engine's stream */
    HIP_OR_CLEANUP(y2h_memcpy_h2d(e->d_tta, e->h_tta, up_bytes, e->stream));
    HIP_OR_CLEANUP(y2h_memset(d_acc, 0, acc_floats * sizeof(float), e->stream));
    slot = 0;
    for (j = 0; j < nstages; ++j) {
        memset(done, 0, cnt);
        off = 0;
        for (i = 0; i < cnt; ++i) {
            const image *f = &frames[first + i];
            stage_dims(mode, f, crop_w, crop_h, stage_scale(mode, scales, j, scale_full), &sz[i].w, &sz[i].h);
            if (sz[i].w == f->w && sz[i].h == f->h) continue;            /* resize_min returns the image itself (image.c:1673) */
            HIP_OR_CLEANUP(y2h_resize_chw(d_src + src_off[i], c, f->h, f->w, d_tmp, d_res + off, sz[i].h, sz[i].w, e->stream));
            off += align_up((size_t)c * sz[i].h * sz[i].w, 4);
        }
        for (i = 0; i < cnt; ++i) {
            long views = 0;
            const float *rows;
            if (done[i]) continue;
            for (k = i; k < cnt; ++k)
                if (!done[k] && sz[k].w == sz[i].w && sz[k].h == sz[i].h) { done[k] = 1; views += per; }
            if (mode != Y2_VIEWS_CROP10 && (net->w != sz[i].w || net->h != sz[i].h)) {
                if (resize_network(net, sz[i].w, sz[i].h) != 0) goto cleanup;
                ++view_resizes;
            }
            if (y2_prepare(net) != 0) goto cleanup;
            for (; views > 0; views -= batch) {
                const int used = views < batch ? (int)views : batch;
                HIP_OR_CLEANUP(y2h_views_to_input((const y2h_view *)e->d_tta + slot, used, d_src, batch, c, net->h, net->w, e->d_in_nchw, e->stream));
                if (y2_engine_forward(net, e->d_in_nchw) != 0) goto cleanup;
                if (y2_output_device(net, &rows) != 0) goto cleanup;
                if (hier && y2_hierarchy_device(net, (float *)rows, batch, 1, (const int *)(e->d_tta + desc_bytes + owner_bytes) + slot) != 0) goto cleanup;
                HIP_OR_CLEANUP(y2h_accumulate_rows(d_acc, rows, outputs, (const int *)(e->d_tta + desc_bytes) + slot, batch, outputs, e->stream));
                slot += batch;
            }
        }
    }
    HIP_OR_CLEANUP(y2h_memcpy_d2h(sums + (size_t)first * outputs, d_acc, acc_floats * sizeof(float), e->stream));
    HIP_OR_CLEANUP(y2h_stream_sync(e->stream));
    rc = 0;
cleanup:
    free(src_off); free(res_off); free(sz);
    return rc;
}

/* bytes a block of frames [first, first+cnt) keeps in HBM: sources, the largest stage's resized copies, accumulators */
static size_t block_need(const network *net, int mode, const image *frames, int first, int cnt, const int *scales,
                         int nstages, int scale_full, int outputs)
{
    size_t src = 0, res = 0;
    int i, j;
    for (i = 0; i < cnt; ++i) src += (size_t)net->c * frames[first + i].h * frames[first + i].w;
    for (j = 0; j < nstages; ++j) {
        size_t stage = 0;
        for (i = 0; i < cnt; ++i) {
            int rw, rh;
            stage_dims(mode, &frames[first + i], net->w, net->h, stage_scale(mode, scales, j, scale_full), &rw, &rh);
            if (rw != frames[first + i].w || rh != frames[first + i].h) stage += (size_t)net->c * rh * rw;
        }
        if (stage > res) res = stage;
    }
    return (src + res + (size_t)cnt * outputs) * sizeof(float);
}

static int view_sums(const char *who, network *net, int mode, const image *frames, int n, const int *scales, int nscales,
                     float *sums)
{
    const int stages_in = mode == Y2_VIEWS_MULTI ? (scales ? nscales : (int)(sizeof default_scales / sizeof default_scales[0])) : 1;
    int w0, h0, outputs, first, rc = 0;
    unsigned char *done;
    size_t budget;
    if (views_check(who, net, mode, frames, n, mode == Y2_VIEWS_MULTI ? scales : NULL, stages_in, sums) != 0) return -1;
    if (mode == Y2_VIEWS_MULTI && !scales) scales = default_scales;
    w0 = net->w; h0 = net->h;
    if (y2_prepare(net) != 0) return -1;
    HIP_OR_ERR(y2h_set_device(y2_engine_of(net)->device));
    if (net->hierarchy && y2_hierarchy_leaves(net) != 0) return -1;     /* the one wait the leaf flags may cost, before the blocks */
    outputs = get_network_output_size(*net);
    budget = block_budget();
    done = malloc(n);
    if (!done) { y2_fail("out of memory"); return -1; }
    for (first = 0; first < n && rc == 0; ) {
        int cnt = 1;
        /* a block is a run of consecutive frames that fits the budget (one frame always goes, whatever its size) */
        while (first + cnt < n && block_need(net, mode, frames, first, cnt + 1, scales, stages_in, w0, outputs) <= budget) ++cnt;
        rc = run_block(net, mode, frames, first, cnt, scales, stages_in, w0, outputs, sums, done);
        first += cnt;
    }
    free(done);
    /* the size the caller's network had; its plan is rebuilt at the next predict, as after any resize_network */
    if ((net->w != w0 || net->h != h0) && resize_network(net, w0, h0) != 0) rc = -1;
    return rc;
}

int y2_classifier_view_sums(network *net, int mode, const image *frames, int n, const int *scales, int nscales, float *sums)
{
    return view_sums("y2_classifier_view_sums", net, mode, frames, n, scales, nscales, sums);
}

/* the books of the reference's loops (classifier.c:397-404, :457-464, :584-591) over the summed predictions */
static int validate_views(const char *who, network *net, int mode, const image *frames, int n, const int *scales, int nscales,
                          const int *truth, int classes, int topk, float *top1_out, float *topk_out)
{
    float *sums = NULL, avg_acc = 0, avg_topk = 0;
    int *indexes = NULL, i, j, rc = -1, outputs;
    if (!net || !net->layers) { y2_fail("%s: net is NULL or empty", who); return -1; }
    if (n <= 0) { y2_fail("%s: n = %d frames", who, n); return -1; }
    if (!truth) { y2_fail("%s: truth is NULL", who); return -1; }
    outputs = get_network_output_size(*net);
    if (classes <= 0 || classes > outputs) { y2_fail("%s: classes = %d against %d network outputs", who, classes, outputs); return -1; }
    if (topk <= 0 || topk > classes) { y2_fail("%s: topk = %d of %d classes", who, topk, classes); return -1; }
    sums = calloc((size_t)n * outputs, sizeof(float));
    indexes = calloc(topk, sizeof(int));
    if (!sums || !indexes) { y2_fail("out of memory"); goto done; }
    if (view_sums(who, net, mode, frames, n, scales, nscales, sums) != 0) goto done;
    for (i = 0; i < n; ++i) {
        top_k(sums + (size_t)i * outputs, classes, topk, indexes);
        if (indexes[0] == truth[i]) avg_acc += 1;
        for (j = 0; j < topk; ++j) if (indexes[j] == truth[i]) avg_topk += 1;
        printf("%d: top 1: %f, top %d: %f\n", i, avg_acc / (i + 1), topk, avg_topk / (i + 1));
    }
    if (top1_out) *top1_out = avg_acc / n;
    if (topk_out) *topk_out = avg_topk / n;
    rc = 0;
done:
    free(sums); free(indexes);
    return rc;
}

int y2_validate_classifier_10_frames(network net, const image *frames, int n, const int *truth, int classes, int topk,
                                     float *top1, float *topk_out)
{
    return validate_views("y2_validate_classifier_10_frames", &net, Y2_VIEWS_CROP10, frames, n, NULL, 0, truth, classes, topk, top1, topk_out);
}

int y2_validate_classifier_multi_frames(network *net, const image *frames, int n, const int *scales, int nscales,
                                        const int *truth, int classes, int topk, float *top1, float *topk_out)
{
    return validate_views("y2_validate_classifier_multi_frames", net, Y2_VIEWS_MULTI, frames, n, scales, nscales, truth, classes, topk, top1, topk_out);
}

int y2_validate_classifier_full_frames(network *net, const image *frames, int n, const int *truth, int classes, int topk,
                                       float *top1, float *topk_out)
{
    return validate_views("y2_validate_classifier_full_frames", net, Y2_VIEWS_FULL, frames, n, NULL, 0, truth, classes, topk, top1, topk_out);
}
