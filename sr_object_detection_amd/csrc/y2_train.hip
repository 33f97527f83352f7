// Training kernels (gfx950): forward in training mode, backward and the SGD update of the convolutional classifier stack,
// loop nest by loop nest after src_yolo2 (convolutional_layer.c:435-528, batchnorm_layer.c:74-155, blas.c:83-126,
// maxpool_layer.c:79-117, avgpool_layer.c:40-69, softmax_layer.c:49-63, cost_layer.c:75-93).
//
// The three products of a convolution are ONE kernel template, an implicit GEMM C[I][J] = sum_r A(i, r) * B(r, j) on the
// fp32 matrix cores.  A is always a gather from an NHWC tensor through (pixel, tap) coordinates, so no im2col buffer
// exists; which GEMM index is the pixel and which the tap is what tells the three forms apart:
//   FWD  i = output pixel, r = tap (ky, kx, ci)   A = x    B = w[r][j]
//   DX   i = input pixel,  r = tap (ky, kx, f)    A = dy   B = w[(ky, kx, j)][f]
//   DW   i = tap (ky, kx, ci), r = output pixel   A = x    B = dy[r][j]      (split over r, partial tiles, second pass)
// Edges (rows, columns, the reduction's tail, padding) are guarded in the gathers: every shape takes this kernel.
// Nothing here uses a floating-point atomic: every reduction is a fixed split followed by a fixed-order second pass.
// The forms, the tile, the gather and the accepted shapes are shared with the bf16 template (y2_train_bf16.hip): y2_train_geo.hpp.
#include "y2_train_geo.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int KT = 16;            // reduction depth of one staging step
constexpr int LDR = KT + 1;       // LDS row pitch of an operand staged [index][r] (its global rows run along r)
constexpr int LDI = TB + 32;      // LDS row pitch of an operand staged [r][index]: the two k rows a wave reads hit disjoint banks
constexpr int LDS_FLOATS = (TB * LDR > KT * LDI) ? TB * LDR : KT * LDI;

// blockIdx.z = the reduction range; a launch with ranges writes range z's tile to dst + z * I * J
template <int MODE>
__global__ __launch_bounds__(256) void train_gemm(const float *__restrict__ asrc, const float *__restrict__ bsrc,
                                                  float *__restrict__ dst, Geo g, int range)
{
    constexpr bool A_RC = MODE != DW, B_RC = MODE == DX;
    __shared__ float As[LDS_FLOATS], Bs[LDS_FLOATS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int wi = wave & 1, wj = wave >> 1;
    const int i0 = blockIdx.x * TB, j0 = blockIdx.y * TB;
    const int rbeg = blockIdx.z * range;
    const int rend = (rbeg + range < g.R) ? rbeg + range : g.R;
    const int ph = MODE == DX ? g.H : g.OH, pw = MODE == DX ? g.W : g.OW;      // what a pixel index counts
    const int tch = MODE == DX ? g.N : g.C;                                   // what a tap's channel counts
    dst += (size_t)blockIdx.z * g.I * g.J;

    // the part of each thread's four A / B elements that does not move with r
    Pix pa[4];
    Tap ta_fixed;
    if (A_RC) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pa[e] = pix_of(i0 + (t >> 4) + 16 * e, g.I, ph, pw);
    } else {
        ta_fixed = tap_of(i0 + (t & 63), g.I, g.K, tch);
    }

    float ra[4], rb[4];
    auto fetch = [&](int r0) {
        if (A_RC) {
            const Tap ta = tap_of(r0 + (t & 15), rend, g.K, tch);
#pragma unroll
            for (int e = 0; e < 4; ++e) ra[e] = a_val<MODE>(asrc, g, pa[e], ta);
            if (B_RC) {                                   // DX: B's r is the same tap
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + (t >> 4) + 16 * e;
                    rb[e] = (ta.ok && j < g.J) ? bsrc[((size_t)(ta.ky * g.K + ta.kx) * g.C + j) * g.N + ta.ch] : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) ra[e] = a_val<MODE>(asrc, g, pix_of(r0 + (t >> 6) + 4 * e, rend, ph, pw), ta_fixed);
        }
        if (!B_RC) {
            const int j = j0 + (t & 63);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + (t >> 6) + 4 * e;
                rb[e] = (r < rend && j < g.J) ? bsrc[(size_t)r * g.J + j] : 0.f;
            }
        }
    };

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    if (rbeg < rend) fetch(rbeg);
    for (int r0 = rbeg; r0 < rend; r0 += KT) {
        __syncthreads();                                  // the previous step's fragments have been read
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (A_RC) As[((t >> 4) + 16 * e) * LDR + (t & 15)] = ra[e];
            else As[((t >> 6) + 4 * e) * LDI + (t & 63)] = ra[e];
            if (B_RC) Bs[((t >> 4) + 16 * e) * LDR + (t & 15)] = rb[e];
            else Bs[((t >> 6) + 4 * e) * LDI + (t & 63)] = rb[e];
        }
        __syncthreads();
        if (r0 + KT < rend) fetch(r0 + KT);               // the next step's loads fly under this step's MFMAs
#pragma unroll
        for (int k2 = 0; k2 < KT / 2; ++k2) {
            const int k = 2 * k2 + lh;
            const float a = A_RC ? As[(wi * 32 + li) * LDR + k] : As[k * LDI + wi * 32 + li];
            const float b = B_RC ? Bs[(wj * 32 + li) * LDR + k] : Bs[k * LDI + wj * 32 + li];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    const int col = j0 + wj * 32 + li;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = i0 + wi * 32 + (v >> 2) * 8 + lh * 4 + (v & 3);
        if (row < g.I && col < g.J) dst[(size_t)row * g.J + col] = acc[v];
    }
}

// dw[e] += the partial tiles in range order
__global__ void dweight_finish(const float *__restrict__ ws, float *__restrict__ dw, long n, int splits)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float s = ws[e];
        for (int k = 1; k < splits; ++k) s += ws[(size_t)k * n + e];
        dw[e] += s;
    }
}

// ---- per-channel reductions over rows of an NHWC tensor: P row chunks -> part[2][P][c], then one thread per channel ----
enum { R_SUM = 0, R_VAR = 1, R_BIAS = 2, R_BNDELTA = 3 };

inline int chunks_of(long rows) { long p = rows / 64; return (int)(p < 1 ? 1 : (p > 512 ? 512 : p)); }

template <int MODE>
__global__ __launch_bounds__(256) void col_partial(const float *__restrict__ a, const float *__restrict__ b,
                                                   const float *__restrict__ scales, const float *__restrict__ mean,
                                                   long rows, int C, int P, float *__restrict__ part)
{
    __shared__ float sh[2][8][32];
    const int c = blockIdx.y * 32 + threadIdx.x, ty = threadIdx.y;
    const long chunk = (rows + P - 1) / P, r0 = blockIdx.x * chunk, r1 = (r0 + chunk < rows) ? r0 + chunk : rows;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        const float m = (MODE == R_VAR || MODE == R_BNDELTA) ? mean[c] : 0.f;
        const float sc = (MODE == R_BNDELTA) ? scales[c] : 0.f;
        for (long r = r0 + ty; r < r1; r += 8) {
            const float v = a[r * C + c];
            if (MODE == R_SUM) s0 += v;
            if (MODE == R_VAR) { const float d = v - m; s0 += d * d; }
            if (MODE == R_BIAS) { s0 += v; if (b) s1 += v * b[r * C + c]; }
            if (MODE == R_BNDELTA) { const float d = v * sc; s0 += d; s1 += d * (b[r * C + c] - m); }
        }
    }
    sh[0][ty][threadIdx.x] = s0;
    sh[1][ty][threadIdx.x] = s1;
    __syncthreads();
    if (ty < 2 && c < C) {
        float s = sh[ty][0][threadIdx.x];
        for (int k = 1; k < 8; ++k) s += sh[ty][k][threadIdx.x];
        part[((size_t)ty * P + blockIdx.x) * C + c] = s;
    }
}

struct Finish { float *o0, *o1, *roll0, *roll1; const float *mean, *variance; float scale, keep, take; };

template <int MODE>
__global__ void col_finish(const float *__restrict__ part, int C, int P, Finish f)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f, s1 = 0.f;
    for (int p = 0; p < P; ++p) { s0 += part[(size_t)p * C + c]; s1 += part[((size_t)P + p) * C + c]; }
    if (MODE == R_SUM) f.o0[c] = s0 * f.scale;                                       // mean_cpu
    if (MODE == R_VAR) {                                                             // variance_cpu, then the rolling statistics
        const float var = s0 * f.scale;
        f.o0[c] = var;
        f.roll0[c] = f.roll0[c] * f.keep + f.take * f.mean[c];
        f.roll1[c] = f.roll1[c] * f.keep + f.take * var;
    }
    if (MODE == R_BIAS) { f.o0[c] += s0; if (f.o1) f.o1[c] += s1; }
    if (MODE == R_BNDELTA) {
        const float var = f.variance[c];
        f.o0[c] = (float)((double)s0 * (-1. / sqrt((double)(var + .00001f))));
        f.o1[c] = (float)((double)s1 * (-.5 * pow((double)(var + .00001f), (double)(float)(-3. / 2.))));
    }
}

template <int MODE>
int col_reduce(const float *a, const float *b, const float *scales, const float *mean, long rows, int C, float *scratch,
               const Finish &f, y2h_stream s)
{
    const int P = chunks_of(rows);
    col_partial<MODE><<<dim3(P, (C + 31) / 32), dim3(32, 8), 0, S(s)>>>(a, b, scales, mean, rows, C, P, scratch);
    Y2H_LAUNCH_CHECK();
    col_finish<MODE><<<(C + 63) / 64, 64, 0, S(s)>>>(scratch, C, P, f);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

__device__ __forceinline__ float gradient_any(float y, int act)      // activations.h:56-82, on the layer's OUTPUT
{
    switch (act) {
    case Y2H_ACT_LEAKY: return (y > 0) ? 1.f : .1f;
    case Y2H_ACT_LOGISTIC: return (1 - y) * y;
    case Y2H_ACT_RELU: return (float)(y > 0);
    }
    return 1.f;
}

__global__ void bn_apply(float *__restrict__ y, float *__restrict__ x, float *__restrict__ x_norm,
                         const float *__restrict__ mean, const float *__restrict__ variance, const float *__restrict__ scales,
                         const float *__restrict__ biases, int act, long n, int C)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        float v = y[e];
        if (mean) {
            x[e] = v;
            v = (float)((double)(v - mean[c]) / (sqrt((double)variance[c]) + (double).000001f));    // normalize_cpu
            x_norm[e] = v;
            v *= scales[c];
        }
        y[e] = activate_any(v + biases[c], act);
    }
}

__global__ void act_gradient(const float *__restrict__ y, float *__restrict__ delta, int act, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        delta[e] *= gradient_any(y[e], act);
}

__global__ void bn_backward(float *__restrict__ delta, const float *__restrict__ x, const float *__restrict__ scales,
                            const float *__restrict__ mean, const float *__restrict__ variance,
                            const float *__restrict__ mean_delta, const float *__restrict__ variance_delta, long n, int C, long rows)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const float d = delta[e] * scales[c];                                         // scale_bias
        delta[e] = (float)((double)d * 1. / (sqrt((double)variance[c]) + (double).00001f) +
                           (double)variance_delta[c] * 2. * (double)(x[e] - mean[c]) / (double)rows +
                           (double)(mean_delta[c] / (float)rows));                     // normalize_delta_cpu
    }
}

__global__ void maxpool_fwd(const float *__restrict__ x, float *__restrict__ y, int *__restrict__ idx, int B, int H, int W, int C,
                            int size, int stride, int pad, int OH, int OW)
{
    const long n = (long)B * OH * OW * C;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        long q = e / C;
        const int ox = (int)(q % OW); q /= OW;
        const int oy = (int)(q % OH);
        const int b = (int)(q / OH);
        float best = -FLT_MAX;
        int where = -1;
        for (int ky = 0; ky < size; ++ky)
            for (int kx = 0; kx < size; ++kx) {
                const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
                const bool valid = iy >= 0 && iy < H && ix >= 0 && ix < W;
                const float v = valid ? x[((size_t)(b * H + iy) * W + ix) * C + c] : -FLT_MAX;
                if (v > best) { best = v; where = iy * W + ix; }
            }
        y[e] = best;
        idx[e] = where;
    }
}

__global__ void maxpool_bwd(const float *__restrict__ dy, const int *__restrict__ idx, float *__restrict__ dx, int B, int H, int W,
                            int C, int size, int stride, int pad, int OH, int OW)
{
    const long n = (long)B * H * W * C;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        long q = e / C;
        const int ix = (int)(q % W); q /= W;
        const int iy = (int)(q % H);
        const int b = (int)(q / H);
        // windows oy with oy*stride - pad <= iy <= oy*stride - pad + size - 1
        const int ty = iy + pad, tx = ix + pad;
        const int oy0 = ty - size + 1 > 0 ? (ty - size + 1 + stride - 1) / stride : 0, oy1 = ty / stride < OH - 1 ? ty / stride : OH - 1;
        const int ox0 = tx - size + 1 > 0 ? (tx - size + 1 + stride - 1) / stride : 0, ox1 = tx / stride < OW - 1 ? tx / stride : OW - 1;
        const int me = iy * W + ix;
        float s = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                const size_t o = ((size_t)(b * OH + oy) * OW + ox) * C + c;
                if (idx[o] == me) s += dy[o];
            }
        dx[e] = s;
    }
}

__global__ void avgpool_fwd(const float *__restrict__ x, float *__restrict__ y, int B, int HW, int C)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * C) return;
    const int b = e / C, c = e - b * C;
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += x[((size_t)b * HW + p) * C + c];
    y[e] = s / HW;
}

__global__ void avgpool_bwd(const float *__restrict__ dy, float *__restrict__ dx, int B, int HW, int C)
{
    const long n = (long)B * HW * C;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C), b = (int)(e / ((long)HW * C));
        dx[e] = dy[b * C + c] / HW;
    }
}

__global__ void softmax_rows(const float *__restrict__ x, float *__restrict__ y, int rows, int n, float temp)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) softmax_seq(x + (size_t)r * n, n, temp, y + (size_t)r * n);
}

// one workgroup: lane sums in index stride order, then a fixed tree
__global__ __launch_bounds__(256) void cost_sse(const float *__restrict__ pred, const float *__restrict__ truth,
                                                float *__restrict__ error, float *__restrict__ delta,
                                                float *__restrict__ delta_prev, float scale, long n, float *__restrict__ cost)
{
    __shared__ float sh[256];
    float s = 0.f;
    for (long e = threadIdx.x; e < n; e += 256) {
        const float d = truth[e] - pred[e];
        const float sq = d * d;
        error[e] = sq;
        delta[e] = d;
        delta_prev[e] = scale * d;
        s += sq;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) cost[0] = sh[0];
}

// chunk b of gridDim.x: the same lane sums and tree over its contiguous part -> part[b]
__global__ __launch_bounds__(256) void cost_sse_chunk(const float *__restrict__ pred, const float *__restrict__ truth,
                                                      float *__restrict__ error, float *__restrict__ delta,
                                                      float *__restrict__ delta_prev, float scale, long n, float *__restrict__ part)
{
    __shared__ float sh[256];
    const long chunk = (n + gridDim.x - 1) / gridDim.x, e0 = blockIdx.x * chunk, e1 = e0 + chunk < n ? e0 + chunk : n;
    float s = 0.f;
    for (long e = e0 + threadIdx.x; e < e1; e += 256) {
        const float d = truth[e] - pred[e];
        const float sq = d * d;
        error[e] = sq;
        delta[e] = d;
        delta_prev[e] = scale * d;
        s += sq;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void cost_sse_sum(const float *__restrict__ part, int chunks, float *__restrict__ cost)
{
    float s = 0.f;
    for (int b = 0; b < chunks; ++b) s += part[b];
    cost[0] = s;
}

// dropout_layer.c:38-59 on a dense NHWC tensor; the draws are indexed as the reference's [batch][c][hw]
__global__ void dropout_apply(float *__restrict__ x, const float *__restrict__ rnd, float probability, float scale, long n, int c, int hw)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(e % c);
        const long q = e / c, b = q / hw;
        const float r = rnd[(b * c + ci) * hw + (q - b * hw)];
        x[e] = (r < probability) ? 0.f : x[e] * scale;
    }
}

__global__ void sgd(float *__restrict__ w, float *__restrict__ u, long n, float rate, float wd, float momentum)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float up = u[e], wv = w[e];
        if (wd != 0.f) up += wd * wv;
        wv += rate * up;
        w[e] = wv;
        u[e] = up * momentum;
    }
}

}  // namespace

int y2_train_dweight_finish(const float *ws, float *dw, long n, int splits, y2h_stream s)
{
    dweight_finish<<<y2h_grid(n, 256), 256, 0, S(s)>>>(ws, dw, n, splits);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" {

int y2h_train_conv_forward(const y2h_train_conv *c, const float *x, const float *w, float *y, y2h_stream s)
{
    Geo g;
    if (!x || !w || !y || geo_of(c, FWD, &g) != Y2H_OK) return Y2H_EINVAL;
    train_gemm<FWD><<<tiles_of(g, 1), 256, 0, S(s)>>>(x, w, y, g, g.R);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_conv_dinput(const y2h_train_conv *c, const float *dy, const float *w, float *dx, y2h_stream s)
{
    Geo g;
    if (!dy || !w || !dx || geo_of(c, DX, &g) != Y2H_OK) return Y2H_EINVAL;
    train_gemm<DX><<<tiles_of(g, 1), 256, 0, S(s)>>>(dy, w, dx, g, g.R);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

/* ranges of the weight gradient's reduction: about eight workgroups per CU (2048 in all; with two per CU the counters
 * showed a quarter of the forward form's resident waves and twice its run time), at least 256 pixels per range */
int y2h_train_dweight_splits(const y2h_train_conv *c)
{
    Geo g;
    if (geo_of(c, DW, &g) != Y2H_OK) return 0;
    const long tiles = (long)((g.I + TB - 1) / TB) * ((g.J + TB - 1) / TB);
    long want = (2048 + tiles - 1) / tiles, most = (g.R + 255) / 256;
    if (want > most) want = most;
    if (want > 256) want = 256;
    return (int)(want < 1 ? 1 : want);
}

size_t y2h_train_dweight_ws_bytes(const y2h_train_conv *c)
{
    Geo g;
    if (geo_of(c, DW, &g) != Y2H_OK) return 0;
    return (size_t)y2h_train_dweight_splits(c) * g.I * g.J * sizeof(float);
}

int y2h_train_conv_dweight(const y2h_train_conv *c, const float *x, const float *dy, float *dw, float *ws, y2h_stream s)
{
    Geo g;
    if (!x || !dy || !dw || !ws || geo_of(c, DW, &g) != Y2H_OK) return Y2H_EINVAL;
    const int splits = y2h_train_dweight_splits(c);
    train_gemm<DW><<<tiles_of(g, splits), 256, 0, S(s)>>>(x, dy, ws, g, dweight_range(g, splits));
    Y2H_LAUNCH_CHECK();
    return y2_train_dweight_finish(ws, dw, (long)g.I * g.J, splits, s);
}

size_t y2h_train_reduce_scratch_bytes(long rows, int c)
{
    if (rows <= 0 || c <= 0) return 0;
    return (size_t)2 * chunks_of(rows) * c * sizeof(float);
}

int y2h_train_bn_stats(const float *x, long rows, int c, float *mean, float *variance, float *rolling_mean,
                       float *rolling_variance, float *scratch, y2h_stream s)
{
    return y2h_train_bn_stats_rate(x, rows, c, mean, variance, rolling_mean, rolling_variance, .9f, .1f, scratch, s);
}

int y2h_train_bn_stats_rate(const float *x, long rows, int c, float *mean, float *variance, float *rolling_mean,
                            float *rolling_variance, float keep, float take, float *scratch, y2h_stream s)
{
    if (!x || !mean || !variance || !rolling_mean || !rolling_variance || !scratch || rows < 2 || c <= 0) return Y2H_EINVAL;
    Finish f = {};
    f.o0 = mean; f.scale = (float)(1. / (double)rows);
    int rc = col_reduce<R_SUM>(x, nullptr, nullptr, nullptr, rows, c, scratch, f, s);
    if (rc != Y2H_OK) return rc;
    f.o0 = variance; f.scale = (float)(1. / (double)(rows - 1)); f.mean = mean; f.roll0 = rolling_mean; f.roll1 = rolling_variance; f.keep = keep; f.take = take;
    return col_reduce<R_VAR>(x, nullptr, nullptr, mean, rows, c, scratch, f, s);
}

int y2h_train_bias_grad(const float *delta, const float *x_norm, long rows, int c, float *bias_updates, float *scale_updates,
                        float *scratch, y2h_stream s)
{
    if (!delta || !bias_updates || !scratch || rows <= 0 || c <= 0 || (x_norm != nullptr) != (scale_updates != nullptr)) return Y2H_EINVAL;
    Finish f = {};
    f.o0 = bias_updates; f.o1 = scale_updates;
    return col_reduce<R_BIAS>(delta, x_norm, nullptr, nullptr, rows, c, scratch, f, s);
}

int y2h_train_bn_deltas(const float *delta, const float *x, const float *scales, const float *mean, const float *variance,
                        long rows, int c, float *mean_delta, float *variance_delta, float *scratch, y2h_stream s)
{
    if (!delta || !x || !scales || !mean || !variance || !mean_delta || !variance_delta || !scratch || rows <= 0 || c <= 0) return Y2H_EINVAL;
    Finish f = {};
    f.o0 = mean_delta; f.o1 = variance_delta; f.variance = variance;
    return col_reduce<R_BNDELTA>(delta, x, scales, mean, rows, c, scratch, f, s);
}

int y2h_train_bn_backward(float *delta, const float *x, const float *scales, const float *mean, const float *variance,
                          const float *mean_delta, const float *variance_delta, long rows, int c, y2h_stream s)
{
    if (!delta || !x || !scales || !mean || !variance || !mean_delta || !variance_delta || rows <= 0 || c <= 0) return Y2H_EINVAL;
    bn_backward<<<y2h_grid(rows * c, 256), 256, 0, S(s)>>>(delta, x, scales, mean, variance, mean_delta, variance_delta, rows * c, c, rows);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_bn_apply(float *y, float *x, float *x_norm, const float *mean, const float *variance, const float *scales,
                       const float *biases, int act, long rows, int c, y2h_stream s)
{
    if (!y || !biases || rows <= 0 || c <= 0) return Y2H_EINVAL;
    if (mean && (!x || !x_norm || !variance || !scales)) return Y2H_EINVAL;
    bn_apply<<<y2h_grid(rows * c, 256), 256, 0, S(s)>>>(y, x, x_norm, mean, variance, scales, biases, act, rows * c, c);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_act_gradient(const float *y, float *delta, int act, long n, y2h_stream s)
{
    if (!y || !delta || n <= 0) return Y2H_EINVAL;
    if (act != Y2H_ACT_LINEAR && act != Y2H_ACT_LEAKY && act != Y2H_ACT_LOGISTIC && act != Y2H_ACT_RELU) return Y2H_EINVAL;
    if (act == Y2H_ACT_LINEAR) return Y2H_OK;
    act_gradient<<<y2h_grid(n, 256), 256, 0, S(s)>>>(y, delta, act, n);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

static int pool_ok(const void *a, const void *b, int batch, int h, int w, int c, int size, int stride, int pad, int out_h, int out_w)
{
    return a && b && batch > 0 && h > 0 && w > 0 && c > 0 && size > 0 && stride > 0 && pad >= 0 && out_h > 0 && out_w > 0 &&
           (long)batch * h * w * c < 2147483647L && (long)batch * out_h * out_w * c < 2147483647L;
}

int y2h_train_maxpool_forward(const float *x, float *y, int *idx, int batch, int h, int w, int c, int size, int stride, int pad,
                              int out_h, int out_w, y2h_stream s)
{
    if (!idx || !pool_ok(x, y, batch, h, w, c, size, stride, pad, out_h, out_w)) return Y2H_EINVAL;
    maxpool_fwd<<<y2h_grid((long)batch * out_h * out_w * c, 256), 256, 0, S(s)>>>(x, y, idx, batch, h, w, c, size, stride, pad, out_h, out_w);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_maxpool_backward(const float *dy, const int *idx, float *dx, int batch, int h, int w, int c, int size, int stride,
                               int pad, int out_h, int out_w, y2h_stream s)
{
    if (!idx || !pool_ok(dy, dx, batch, h, w, c, size, stride, pad, out_h, out_w)) return Y2H_EINVAL;
    maxpool_bwd<<<y2h_grid((long)batch * h * w * c, 256), 256, 0, S(s)>>>(dy, idx, dx, batch, h, w, c, size, stride, pad, out_h, out_w);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_avgpool_forward(const float *x, float *y, int batch, int hw, int c, y2h_stream s)
{
    if (!x || !y || batch <= 0 || hw <= 0 || c <= 0 || (long)batch * hw * c >= 2147483647L) return Y2H_EINVAL;
    avgpool_fwd<<<(batch * c + 255) / 256, 256, 0, S(s)>>>(x, y, batch, hw, c);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_avgpool_backward(const float *dy, float *dx, int batch, int hw, int c, y2h_stream s)
{
    if (!dy || !dx || batch <= 0 || hw <= 0 || c <= 0 || (long)batch * hw * c >= 2147483647L) return Y2H_EINVAL;
    avgpool_bwd<<<y2h_grid((long)batch * hw * c, 256), 256, 0, S(s)>>>(dy, dx, batch, hw, c);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_softmax(const float *x, float *y, int rows, int n, float temperature, y2h_stream s)
{
    if (!x || !y || rows <= 0 || n <= 0) return Y2H_EINVAL;
    softmax_rows<<<(rows + 63) / 64, 64, 0, S(s)>>>(x, y, rows, n, temperature);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_cost_sse(const float *pred, const float *truth, float *error, float *delta, float *delta_prev, float scale, long n,
                       float *cost, y2h_stream s)
{
    if (!pred || !truth || !error || !delta || !delta_prev || !cost || n <= 0) return Y2H_EINVAL;
    cost_sse<<<1, 256, 0, S(s)>>>(pred, truth, error, delta, delta_prev, scale, n, cost);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_cost_sse_chunked(const float *pred, const float *truth, float *error, float *delta, float *delta_prev, float scale,
                               long n, float *cost, float *scratch, y2h_stream s)
{
    if (!pred || !truth || !error || !delta || !delta_prev || !cost || !scratch || n <= 0) return Y2H_EINVAL;
    cost_sse_chunk<<<Y2H_COST_CHUNKS, 256, 0, S(s)>>>(pred, truth, error, delta, delta_prev, scale, n, scratch);
    Y2H_LAUNCH_CHECK();
    cost_sse_sum<<<1, 1, 0, S(s)>>>(scratch, Y2H_COST_CHUNKS, cost);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_dropout(float *x, const float *rnd, float probability, float scale, int batch, int c, int hw, y2h_stream s)
{
    if (!x || !rnd || batch <= 0 || c <= 0 || hw <= 0 || (long)batch * c * hw >= 2147483647L) return Y2H_EINVAL;
    const long n = (long)batch * c * hw;
    dropout_apply<<<y2h_grid(n, 256), 256, 0, S(s)>>>(x, rnd, probability, scale, n, c, hw);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_sgd(float *w, float *updates, long n, float rate, float wd, float momentum, y2h_stream s)
{
    if (!w || !updates || n <= 0) return Y2H_EINVAL;
    sgd<<<y2h_grid(n, 256), 256, 0, S(s)>>>(w, updates, n, rate, wd, momentum);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

}  // extern "C"
