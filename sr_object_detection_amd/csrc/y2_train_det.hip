// Training kernels of the detector's tail (gfx950): the [region] head in training mode after src_yolo2/region_layer.c:144-321
// (CPU branch, DOABS 1, flat softmax) with backward_region_layer (:323-326), the two directions of [route]
// (route_layer.c:73-101) on dense NHWC tensors, the backward of a non-reverse [reorg] (reorg_layer.c:87-94) and the plain
// add a delta with more than one writer needs.  The [detection] head of YOLOv1 (detection_layer.c:49-222) is below the region head:
// detection_cells (one thread per image and cell), the region head's region_sumsq, detection_finish.
//
// The region head is four launches on one stream:
//   region_cells    one thread per (image, cell, anchor): activation, predicted box, best IoU over the image's truths,
//                   the no-object delta and (while seen < 12800) the prior-box delta; the thread writes its whole delta
//                   row, zeros included, so no memset precedes it
//   region_truths   one wave per image walks that image's truths IN ORDER (a later truth that picks the same (cell, anchor)
//                   owns the row); every lane computes the same scalars, lane 0 stores the box and objectness deltas, the
//                   lanes share the class deltas -- a class column is always written by the same lane, so program order
//                   keeps the reference's last-writer-wins
//   region_sumsq    delta -> the preceding layer's delta, and fixed chunks of sum delta^2
//   region_finish   one thread adds the chunks, the per-workgroup objectness sums and the per-image statistics in index
//                   order
// No floating-point atomic anywhere: the bytes do not depend on how the launches were scheduled.  The statistics are
// accumulated in double (they are sums of values the reference prints, not values the step goes on with).
#include "y2_common.hpp"

namespace {

constexpr int TRUTHS = 30;                 // region_layer.c:222 / :259
constexpr int CELL_BLOCK = 256;
constexpr int SUM_BLOCK = 256;
constexpr int SUM_CHUNK = 4096;            // floats per workgroup of region_sumsq

struct Box { float x, y, w, h; };

__device__ __forceinline__ float logistic_f(float x) { return (float)(1. / (1. + exp(-(double)x))); }
__device__ __forceinline__ float logistic_grad(float x) { return (1 - x) * x; }

// box.c:67-97
__device__ __forceinline__ float overlap1(float x1, float w1, float x2, float w2)
{
    const float l1 = x1 - w1 / 2, l2 = x2 - w2 / 2;
    const float left = l1 > l2 ? l1 : l2;
    const float r1 = x1 + w1 / 2, r2 = x2 + w2 / 2;
    const float right = r1 < r2 ? r1 : r2;
    return right - left;
}

__device__ __forceinline__ float box_iou(const Box &a, const Box &b)
{
    const float w = overlap1(a.x, a.w, b.x, b.w);
    const float h = overlap1(a.y, a.h, b.y, b.h);
    const float inter = (w < 0 || h < 0) ? 0 : w * h;
    const float uni = a.w * a.h + b.w * b.h - inter;
    return inter / uni;
}

// get_region_box (:73-85)
__device__ __forceinline__ Box region_box(const float *x, const float *anchors, int n, int i, int j, int w, int h)
{
    Box b;
    b.x = (i + logistic_f(x[0])) / w;
    b.y = (j + logistic_f(x[1])) / h;
    b.w = (float)(exp((double)x[2]) * anchors[2 * n] / w);
    b.h = (float)(exp((double)x[3]) * anchors[2 * n + 1] / h);
    return b;
}

// delta_region_box (:87-106)
__device__ __forceinline__ float delta_box(const Box &truth, const float *x, const float *anchors, int n, int i, int j, int w, int h,
                                           float *delta, float scale, bool store)
{
    const Box pred = region_box(x, anchors, n, i, j, w, h);
    const float iou = box_iou(pred, truth);
    const float tx = truth.x * w - i, ty = truth.y * h - j;
    const float tw = (float)log((double)(truth.w * w / anchors[2 * n]));
    const float th = (float)log((double)(truth.h * h / anchors[2 * n + 1]));
    if (store) {
        const float lx = logistic_f(x[0]), ly = logistic_f(x[1]);
        delta[0] = scale * (tx - lx) * logistic_grad(lx);
        delta[1] = scale * (ty - ly) * logistic_grad(ly);
        delta[2] = scale * (tw - x[2]);
        delta[3] = scale * (th - x[3]);
    }
    return iou;
}

// the image's truths into LDS; the list ends at the first x == 0 (:224)
__device__ __forceinline__ int load_truths(const float *__restrict__ truth, float *tr, int *count)
{
    for (int e = threadIdx.x; e < TRUTHS * 5; e += blockDim.x) tr[e] = truth[e];
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        while (t < TRUTHS && tr[t * 5] != 0) ++t;
        *count = t;
    }
    __syncthreads();
    return *count;
}

__global__ __launch_bounds__(CELL_BLOCK) void region_cells(y2h_train_region g, const float *__restrict__ in,
                                                           const float *__restrict__ anchors, const float *__restrict__ truth,
                                                           int seen, float *__restrict__ out, float *__restrict__ delta,
                                                           double *__restrict__ anyobj_part)
{
    __shared__ float tr[TRUTHS * 5];
    __shared__ int nt_s;
    __shared__ double sh[CELL_BLOCK];
    const int b = blockIdx.y, size = 5 + g.classes, boxes = g.h * g.w * g.n;
    const int nt = load_truths(truth + (size_t)b * TRUTHS * 5, tr, &nt_s);
    const int idx = blockIdx.x * CELL_BLOCK + threadIdx.x;
    double any = 0.;
    if (idx < boxes) {
        const int n = idx % g.n, cell = idx / g.n, i = cell % g.w, j = cell / g.w;
        const size_t row = ((size_t)b * boxes + idx) * size;
        const float *x = in + row;
        float *o = out + row, *d = delta + row;
        for (int k = 0; k < 4; ++k) o[k] = x[k];
        const float obj = logistic_f(x[4]);
        o[4] = obj;
        softmax_seq(x + 5, g.classes, 1.f, o + 5);
        const Box pred = region_box(x, anchors, n, i, j, g.w, g.h);
        float best = 0;
        for (int t = 0; t < nt; ++t) {
            const Box tb = { tr[t * 5], tr[t * 5 + 1], tr[t * 5 + 2], tr[t * 5 + 3] };
            const float iou = box_iou(pred, tb);
            if (iou > best) best = iou;
        }
        any = obj;
        for (int k = 0; k < size; ++k) d[k] = 0.f;
        d[4] = (best > g.thresh) ? 0.f : g.noobject_scale * ((0 - obj) * logistic_grad(obj));
        if (seen < 12800) {
            Box prior;
            prior.x = (float)((i + .5) / g.w);
            prior.y = (float)((j + .5) / g.h);
            prior.w = anchors[2 * n] / g.w;
            prior.h = anchors[2 * n + 1] / g.h;
            delta_box(prior, x, anchors, n, i, j, g.w, g.h, d, .01f, true);
        }
    }
    sh[threadIdx.x] = any;
    __syncthreads();
    for (int s = CELL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) anyobj_part[(size_t)b * gridDim.x + blockIdx.x] = sh[0];
}

// per image: avg_iou, avg_cat, avg_obj, recall, count, class_count
__global__ __launch_bounds__(64) void region_truths(y2h_train_region g, const float *__restrict__ anchors,
                                                    const float *__restrict__ truth, const float *__restrict__ out,
                                                    float *__restrict__ delta, double *__restrict__ image_stats)
{
    __shared__ float tr[TRUTHS * 5];
    __shared__ int nt_s;
    const int b = blockIdx.x, size = 5 + g.classes, boxes = g.h * g.w * g.n, lane = threadIdx.x;
    const int nt = load_truths(truth + (size_t)b * TRUTHS * 5, tr, &nt_s);
    double s_iou = 0., s_cat = 0., s_obj = 0., s_recall = 0.;
    int count = 0;
    for (int t = 0; t < nt; ++t) {
        const Box tb = { tr[t * 5], tr[t * 5 + 1], tr[t * 5 + 2], tr[t * 5 + 3] };
        const int i = (int)(tb.x * g.w), j = (int)(tb.y * g.h);
        // the reference indexes outside its arrays here; such a truth is skipped whole (differences)
        if (i < 0 || i >= g.w || j < 0 || j >= g.h) continue;
        const Box shift = { 0, 0, tb.w, tb.h };
        const size_t cell_row = ((size_t)b * boxes + (size_t)(j * g.w + i) * g.n) * size;
        float best_iou = 0;
        int best_n = 0;
        for (int n = 0; n < g.n; ++n) {
            Box pred = region_box(out + cell_row + (size_t)n * size, anchors, n, i, j, g.w, g.h);
            if (g.bias_match) {
                pred.w = anchors[2 * n] / g.w;
                pred.h = anchors[2 * n + 1] / g.h;
            }
            pred.x = 0;
            pred.y = 0;
            const float iou = box_iou(pred, shift);
            if (iou > best_iou) { best_iou = iou; best_n = n; }
        }
        const float *x = out + cell_row + (size_t)best_n * size;
        float *d = delta + cell_row + (size_t)best_n * size;
        const float iou = delta_box(tb, x, anchors, best_n, i, j, g.w, g.h, d, g.coord_scale, lane == 0);
        if (iou > .5f) s_recall += 1;
        s_iou += iou;
        const float obj = x[4];
        s_obj += obj;
        if (lane == 0) d[4] = g.object_scale * ((g.rescore ? iou : 1.f) - obj) * logistic_grad(obj);
        const int cls = (int)tr[t * 5 + 4];
        for (int k = lane; k < g.classes; k += 64) d[5 + k] = g.class_scale * (((k == cls) ? 1 : 0) - x[5 + k]);
        if (cls >= 0 && cls < g.classes) s_cat += x[5 + cls];
        ++count;
    }
    if (lane == 0) {
        double *st = image_stats + (size_t)b * 6;
        st[0] = s_iou; st[1] = s_cat; st[2] = s_obj; st[3] = s_recall; st[4] = count; st[5] = count;
    }
}

template <bool ADD>
__global__ __launch_bounds__(SUM_BLOCK) void region_sumsq(const float *__restrict__ delta, float *__restrict__ delta_prev, long n,
                                                          float *__restrict__ part)
{
    __shared__ float sh[SUM_BLOCK];
    const long e0 = (long)blockIdx.x * SUM_CHUNK, e1 = (e0 + SUM_CHUNK < n) ? e0 + SUM_CHUNK : n;
    float s = 0.f;
    for (long e = e0 + threadIdx.x; e < e1; e += SUM_BLOCK) {
        const float d = delta[e];
        if (ADD) delta_prev[e] += d;       // axpy_cpu(.., 1, l.delta, 1, state.delta, 1): a later writer adds,
        else delta_prev[e] = d;            // the first one finds the zeroed delta
        s += d * d;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = SUM_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void region_finish(y2h_train_region g, const float *__restrict__ part, int parts, const double *__restrict__ anyobj_part,
                              int any_parts, const double *__restrict__ image_stats, float *__restrict__ cost,
                              y2h_train_region_stats *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float sum = 0.f;
    for (int p = 0; p < parts; ++p) sum += part[p];
    const float mag = sqrtf(sum);                                   // mag_array
    cost[0] = (float)pow((double)mag, 2.);
    double any = 0., st[6] = { 0., 0., 0., 0., 0., 0. };
    for (int p = 0; p < any_parts; ++p) any += anyobj_part[p];
    for (int b = 0; b < g.batch; ++b)
        for (int k = 0; k < 6; ++k) st[k] += image_stats[(size_t)b * 6 + k];
    const int count = (int)st[4], class_count = (int)st[5];
    stats->avg_iou = (float)st[0] / count;                          // the printf of :320: float / int, NaN when count == 0
    stats->avg_class = (float)st[1] / class_count;
    stats->avg_obj = (float)st[2] / count;
    stats->avg_noobj = (float)any / (g.w * g.h * g.n * g.batch);
    stats->recall = (float)st[3] / count;
    stats->count = count;
    stats->class_count = class_count;
}

// ---- the [detection] head (YOLOv1) in training mode, detection_layer.c:49-222 ----
// An image's row is [cells][classes] class scores | [cells][n] objectness | [cells][n][4] boxes.  A cell writes only its
// own entries of out and delta, all of them (zeros included), so one thread per (image, cell) needs no memset and no order.
constexpr int DET_BLOCK = 64;

// box.c:99-105: the four squares, their sum and the root in double
__device__ __forceinline__ float box_rmse(const Box &a, const Box &b)
{
    return (float)sqrt(pow((double)(a.x - b.x), 2.) + pow((double)(a.y - b.y), 2.) + pow((double)(a.w - b.w), 2.) +
                       pow((double)(a.h - b.h), 2.));
}

__device__ __forceinline__ Box det_box(const float *o, int side, int sq)
{
    Box b = { o[0] / side, o[1] / side, o[2], o[3] };
    if (sq) { b.w = b.w * b.w; b.h = b.h * b.h; }
    return b;
}

// per workgroup: sums of iou, positive class, all classes, chosen objectness, every objectness, and the object count
__global__ __launch_bounds__(DET_BLOCK) void detection_cells(y2h_train_detection g, const float *__restrict__ in,
                                                             const float *__restrict__ truth, float *__restrict__ out,
                                                             float *__restrict__ delta, double *__restrict__ stat_part)
{
    __shared__ double sh[6][DET_BLOCK];
    const int cells = g.side * g.side, per = (1 + 4) * g.n + g.classes, tper = 1 + 4 + g.classes;
    const long idx = (long)blockIdx.x * DET_BLOCK + threadIdx.x;
    double st[6] = { 0., 0., 0., 0., 0., 0. };
    if (idx < (long)g.batch * cells) {
        const int b = (int)(idx / cells), i = (int)(idx % cells);
        const size_t image = (size_t)b * cells * per;
        const float *t = truth + (size_t)idx * tper;
        const size_t cls = image + (size_t)i * g.classes, obj = image + (size_t)cells * g.classes + (size_t)i * g.n;
        const size_t box = image + (size_t)cells * (g.classes + g.n) + (size_t)i * g.n * 4;
        if (g.softmax) softmax_seq(in + cls, g.classes, 1.f, out + cls);
        else for (int j = 0; j < g.classes; ++j) out[cls + j] = in[cls + j];
        for (int j = 0; j < g.n; ++j) {
            const float p = in[obj + j];
            out[obj + j] = p;
            delta[obj + j] = g.noobject_scale * (0 - p);
            st[4] += p;
        }
        for (int j = 0; j < 4 * g.n; ++j) { out[box + j] = in[box + j]; delta[box + j] = 0.f; }
        const int is_obj = (int)t[0];
        if (!is_obj) {
            for (int j = 0; j < g.classes; ++j) delta[cls + j] = 0.f;
        } else {
            for (int j = 0; j < g.classes; ++j) {
                const float p = out[cls + j];
                delta[cls + j] = g.class_scale * (t[1 + j] - p);
                if (t[1 + j]) st[1] += p;
                st[2] += p;
            }
            const float *tb = t + 1 + g.classes;
            const Box tr = { tb[0] / g.side, tb[1] / g.side, tb[2], tb[3] };
            int best = -1;
            float best_iou = 0, best_rmse = 20;
            for (int j = 0; j < g.n; ++j) {
                const Box o = det_box(out + box + 4 * j, g.side, g.sqrt);
                const float iou = box_iou(o, tr), rmse = box_rmse(o, tr);
                if (best_iou > 0 || iou > 0) {
                    if (iou > best_iou) { best_iou = iou; best = j; }
                } else if (rmse < best_rmse) {
                    best_rmse = rmse;
                    best = j;
                }
            }
            if (g.forced) best = (tr.w * tr.h < .1) ? 1 : 0;
            // no box won (every IoU 0 or NaN and every rmse >= 20 or NaN), or forced names box 1 of a one-box head: the
            // reference goes on with entries that are not this cell's; here the cell keeps its no-object and class deltas
            if (best >= 0 && best < g.n) {
                const float *o = out + box + 4 * best;
                const float iou = box_iou(det_box(o, g.side, g.sqrt), tr), p = out[obj + best];
                st[3] += p;
                delta[obj + best] = g.rescore ? g.object_scale * (iou - p) : (float)((double)g.object_scale * (1. - (double)p));
                float *d = delta + box + 4 * best;
                d[0] = g.coord_scale * (tb[0] - o[0]);
                d[1] = g.coord_scale * (tb[1] - o[1]);
                if (g.sqrt) {
                    d[2] = (float)((double)g.coord_scale * (sqrt((double)tb[2]) - (double)o[2]));
                    d[3] = (float)((double)g.coord_scale * (sqrt((double)tb[3]) - (double)o[3]));
                } else {
                    d[2] = g.coord_scale * (tb[2] - o[2]);
                    d[3] = g.coord_scale * (tb[3] - o[3]);
                }
                st[0] += iou;
                st[5] += 1.;
            }
        }
    }
    for (int k = 0; k < 6; ++k) sh[k][threadIdx.x] = st[k];
    __syncthreads();
    for (int s = DET_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 6; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 6) stat_part[(size_t)blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void detection_finish(y2h_train_detection g, const float *__restrict__ part, int parts,
                                 const double *__restrict__ stat_part, int stat_parts, float *__restrict__ cost,
                                 y2h_train_detection_stats *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float sum = 0.f;
    for (int p = 0; p < parts; ++p) sum += part[p];
    const float mag = sqrtf(sum);                                   // mag_array
    cost[0] = (float)pow((double)mag, 2.);
    double st[6] = { 0., 0., 0., 0., 0., 0. };
    for (int p = 0; p < stat_parts; ++p)
        for (int k = 0; k < 6; ++k) st[k] += stat_part[(size_t)p * 6 + k];
    const int count = (int)st[5];
    stats->avg_iou = (float)st[0] / count;                          // the printf of :214: float / int, NaN when count == 0
    stats->avg_cat = (float)st[1] / count;
    stats->avg_allcat = (float)st[2] / (count * g.classes);
    stats->avg_obj = (float)st[3] / count;
    stats->avg_anyobj = (float)st[4] / (g.batch * g.side * g.side * g.n);
    stats->count = count;
}

__global__ void route_fwd(const float *__restrict__ src, int c, float *__restrict__ dst, int ldc, int off, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        dst[(e / c) * ldc + off + (int)(e % c)] = src[e];
}

template <bool ADD>
__global__ void route_bwd(const float *__restrict__ droute, int ldc, int off, float *__restrict__ dsrc, int c, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const float v = droute[(e / c) * ldc + off + (int)(e % c)];
        if (ADD) dsrc[e] += v;
        else dsrc[e] = v;
    }
}

__global__ void add_to(float *__restrict__ dst, const float *__restrict__ src, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) dst[e] += src[e];
}

// reorg_cpu(l.delta, w, h, c, batch, stride, forward = 1, state.delta): dx[out_index(f)] = dy[f] over the flat [c][h][w]
// iteration space f; out_index is a bijection, so every dx element is gathered from the one f that lands on it.  dx is
// NHWC [h][w][c]; dy is NHWC in the layer's output label [c*s*s][h/s][w/s].
__global__ __launch_bounds__(256) void reorg_bwd(const float *__restrict__ dy, float *__restrict__ dx, int h, int w, int c, int s,
                                                 long total)
{
    const int oc_small = c / (s * s), oc = c * s * s, oh = h / s, ow = w / s;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int ci = (int)(idx % c);
        const long ipix = idx / c;
        const int xi = (int)(ipix % w), yi = (int)((ipix / w) % h);
        const long b = ipix / ((long)w * h);
        const long q = ((long)ci * h + yi) * w + xi;              // flat index of this dx element = out_index(f)
        const int w2 = (int)(q % ((long)w * s));
        const int h2 = (int)((q / ((long)w * s)) % ((long)h * s));
        const int c2 = (int)(q / ((long)w * s * h * s));
        const int i = w2 / s, j = h2 / s, k = ((h2 % s) * s + (w2 % s)) * oc_small + c2;
        const long f = i + (long)w * (j + (long)h * k);           // flat index into dy, decoded in its label geometry
        const int xo = (int)(f % ow), yo = (int)((f / ow) % oh), co = (int)(f / ((long)ow * oh));
        dx[idx] = dy[((b * oh + yo) * (long)ow + xo) * oc + co];
    }
}

inline int cell_blocks(const y2h_train_region *g) { return (g->h * g->w * g->n + CELL_BLOCK - 1) / CELL_BLOCK; }
inline long region_floats(const y2h_train_region *g) { return (long)g->batch * g->h * g->w * g->n * (5 + g->classes); }
inline int sum_parts(const y2h_train_region *g) { return (int)((region_floats(g) + SUM_CHUNK - 1) / SUM_CHUNK); }

inline bool region_ok(const y2h_train_region *g)
{
    return g && g->batch > 0 && g->batch <= 65535 && g->h > 0 && g->w > 0 && g->n > 0 && g->classes > 0 &&
           (long)g->h * g->w * g->n * (5 + g->classes) < 2147483647L && region_floats(g) < 2147483647L;
}

inline long detection_floats(const y2h_train_detection *g) { return (long)g->batch * g->side * g->side * (5 * g->n + g->classes); }
inline int detection_blocks(const y2h_train_detection *g) { return (int)(((long)g->batch * g->side * g->side + DET_BLOCK - 1) / DET_BLOCK); }
inline int detection_parts(const y2h_train_detection *g) { return (int)((detection_floats(g) + SUM_CHUNK - 1) / SUM_CHUNK); }

inline bool detection_ok(const y2h_train_detection *g)
{
    return g && g->batch > 0 && g->side > 0 && g->side <= 4096 && g->n > 0 && g->classes > 0 &&
           (long)g->side * g->side * (5L * g->n + g->classes) < 2147483647L && detection_floats(g) < 2147483647L;
}

}  // namespace

extern "C" {

size_t y2h_train_region_scratch_bytes(const y2h_train_region *g)
{
    if (!region_ok(g)) return 0;
    return ((size_t)g->batch * cell_blocks(g) + (size_t)g->batch * 6) * sizeof(double) + (size_t)sum_parts(g) * sizeof(float);
}

int y2h_train_region_loss(const y2h_train_region *g, const float *in, const float *anchors, const float *truth, int seen, float *out,
                          float *delta, float *delta_prev, float *cost, y2h_train_region_stats *stats, void *scratch, y2h_stream s)
{
    if (!region_ok(g) || !in || !anchors || !truth || !out || !delta || !delta_prev || !cost || !stats || !scratch) return Y2H_EINVAL;
    const int cb = cell_blocks(g), parts = sum_parts(g);
    double *any_part = (double *)scratch, *image_stats = any_part + (size_t)g->batch * cb;
    float *part = (float *)(image_stats + (size_t)g->batch * 6);
    region_cells<<<dim3(cb, g->batch), CELL_BLOCK, 0, S(s)>>>(*g, in, anchors, truth, seen, out, delta, any_part);
    Y2H_LAUNCH_CHECK();
    region_truths<<<g->batch, 64, 0, S(s)>>>(*g, anchors, truth, out, delta, image_stats);
    Y2H_LAUNCH_CHECK();
    region_sumsq<false><<<parts, SUM_BLOCK, 0, S(s)>>>(delta, delta_prev, region_floats(g), part);
    Y2H_LAUNCH_CHECK();
    region_finish<<<1, 64, 0, S(s)>>>(*g, part, parts, any_part, g->batch * cb, image_stats, cost, stats);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

size_t y2h_train_detection_scratch_bytes(const y2h_train_detection *g)
{
    if (!detection_ok(g)) return 0;
    return (size_t)detection_blocks(g) * 6 * sizeof(double) + (size_t)detection_parts(g) * sizeof(float);
}

int y2h_train_detection_loss(const y2h_train_detection *g, const float *in, const float *truth, float *out, float *delta,
                             float *delta_prev, int add, float *cost, y2h_train_detection_stats *stats, void *scratch, y2h_stream s)
{
    if (!detection_ok(g) || !in || !truth || !out || !delta || !delta_prev || !cost || !stats || !scratch) return Y2H_EINVAL;
    const int blocks = detection_blocks(g), parts = detection_parts(g);
    double *stat_part = (double *)scratch;
    float *part = (float *)(stat_part + (size_t)blocks * 6);
    detection_cells<<<blocks, DET_BLOCK, 0, S(s)>>>(*g, in, truth, out, delta, stat_part);
    Y2H_LAUNCH_CHECK();
    if (add) region_sumsq<true><<<parts, SUM_BLOCK, 0, S(s)>>>(delta, delta_prev, detection_floats(g), part);
    else region_sumsq<false><<<parts, SUM_BLOCK, 0, S(s)>>>(delta, delta_prev, detection_floats(g), part);
    Y2H_LAUNCH_CHECK();
    detection_finish<<<1, 64, 0, S(s)>>>(*g, part, parts, stat_part, blocks, cost, stats);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_route_forward(const float *src, int c, float *dst, int ldc, int off, long pixels, y2h_stream s)
{
    if (!src || !dst || c <= 0 || off < 0 || ldc < off + c || pixels <= 0 || pixels * ldc >= 2147483647L) return Y2H_EINVAL;
    route_fwd<<<y2h_grid(pixels * c, 256), 256, 0, S(s)>>>(src, c, dst, ldc, off, pixels * c);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_route_backward(const float *droute, int ldc, int off, float *dsrc, int c, long pixels, int add, y2h_stream s)
{
    if (!droute || !dsrc || c <= 0 || off < 0 || ldc < off + c || pixels <= 0 || pixels * ldc >= 2147483647L) return Y2H_EINVAL;
    if (add) route_bwd<true><<<y2h_grid(pixels * c, 256), 256, 0, S(s)>>>(droute, ldc, off, dsrc, c, pixels * c);
    else route_bwd<false><<<y2h_grid(pixels * c, 256), 256, 0, S(s)>>>(droute, ldc, off, dsrc, c, pixels * c);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_add(float *dst, const float *src, long n, y2h_stream s)
{
    if (!dst || !src || n <= 0) return Y2H_EINVAL;
    add_to<<<y2h_grid(n, 256), 256, 0, S(s)>>>(dst, src, n);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_reorg_backward(const float *dy, float *dx, int batch, int h, int w, int c, int stride, y2h_stream s)
{
    if (!dy || !dx || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || stride <= 0) return Y2H_EINVAL;
    if (c % (stride * stride) != 0 || h % stride != 0 || w % stride != 0 || (long)batch * h * w * c >= 2147483647L) return Y2H_EINVAL;
    const long total = (long)batch * h * w * c;
    reorg_bwd<<<y2h_grid(total, 256), 256, 0, S(s)>>>(dy, dx, h, w, c, stride, total);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

}  // extern "C"
