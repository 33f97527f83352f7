// Training kernels of an [rnn] layer (gfx950): what back-propagation through time needs beside the three products of a
// dense layer (y2_train_dense.hip).  The three [connected] sub-layers of an [rnn] run T time steps of B rows each
// (rows are step-major, t*B + b), and the reference normalises, and sums its gradients, per step
// (rnn_layer.c:83-172 over connected_layer.c:122-191).  A "group" below is one time step's B rows of a [T][B][C] tensor.
//
//   group_stats   per (step, column) mean and variance (/(B-1)) over the step's own B rows: one launch for all T steps
//   roll_stats    rolling = keep * rolling + take * new, once per step IN STEP ORDER (one thread per column walks t)
//   group_apply   bn_apply of y2_train.hip with the step's own mean / variance
//   delta_group   backward_connected_layer up to the products, per step: gradient_array, the step's bias and scale sums
//                 (-> [T][C]), scale_bias, mean_delta, variance_delta, normalize_delta in place.  Its mean and variance
//                 are ONE row for every step: increment_layer (rnn_layer.c:11-27) advances output, delta, x and x_norm
//                 but not mean and variance, so the reference's backward of every step reads the LAST step's statistics
//   sum_steps     bias_updates += the per-step sums, in the reference's order (the last step first)
//   combine       state[t+1] = input.output[t] + self.output[t]  (fill 0, axpy, axpy: (0 + a) + b)
//   step_finish   group_stats, roll_stats, group_apply and combine of ONE step in one launch: the self sub-layer's chain
//   add_transposed  weight_updates[o][k] += dw[k][o], behind a weight gradient made by the convolution template at size 1
//   onehot        get_rnn_data's two one-hot tensors (rnn.c:86-114) from the B x (T+1) bytes the streams read
//
// A workgroup is 32 columns x 16 row lanes of one group: lane ty sums rows ty, ty+16, ... and the 16 partial sums are
// added in lane order, so every sum has one fixed order; no atomics.  (The step-by-step launches of the self sub-layer are
// latency-bound -- one group, hidden / 32 workgroups: with 8 row lanes a lane walked 16 rows of B = 128 one after the other
// and delta_group took 22 us a step at hidden 1024; 16 lanes walk 8.)
#include "y2_common.hpp"

namespace {

constexpr int COLS = 32, LANES = 16;     // the workgroup; LANES is the chunk of a group's rows

// sums of up to four values over the row lanes, lane 0 first; every thread of a column returns the same totals
template <int N>
__device__ __forceinline__ void lane_sums(float (&v)[N], float (*sh)[LANES][COLS])
{
    const int tx = threadIdx.x, ty = threadIdx.y;
    __syncthreads();                                      // the buffer's previous use has been read
#pragma unroll
    for (int k = 0; k < N; ++k) sh[k][ty][tx] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float s = sh[k][0][tx];
        for (int l = 1; l < LANES; ++l) s += sh[k][l][tx];
        v[k] = s;
    }
}

__global__ __launch_bounds__(COLS * LANES) void group_stats(const float *__restrict__ x, int B, int C, float *__restrict__ mean,
                                                            float *__restrict__ variance)
{
    __shared__ float sh[1][LANES][COLS];
    const int c = blockIdx.x * COLS + threadIdx.x, t = blockIdx.y;
    const bool in = c < C;
    const float *g = x + (size_t)t * B * C;
    float s[1] = { 0.f };
    if (in) for (int r = threadIdx.y; r < B; r += LANES) s[0] += g[(size_t)r * C + c];
    lane_sums(s, sh);
    const float m = s[0] * (float)(1. / B);                                     // mean_cpu
    s[0] = 0.f;
    if (in) for (int r = threadIdx.y; r < B; r += LANES) { const float d = g[(size_t)r * C + c] - m; s[0] += d * d; }
    lane_sums(s, sh);
    if (in && threadIdx.y == 0) {
        mean[(size_t)t * C + c] = m;
        variance[(size_t)t * C + c] = s[0] * (float)(1. / (B - 1));             // variance_cpu
    }
}

__global__ void roll_stats(const float *__restrict__ mean, const float *__restrict__ variance, int T, int C,
                           float *__restrict__ rolling_mean, float *__restrict__ rolling_variance, float keep, float take)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float rm = rolling_mean[c], rv = rolling_variance[c];
    for (int t = 0; t < T; ++t) {
        rm = rm * keep + take * mean[(size_t)t * C + c];
        rv = rv * keep + take * variance[(size_t)t * C + c];
    }
    rolling_mean[c] = rm;
    rolling_variance[c] = rv;
}

__global__ void group_apply(float *__restrict__ y, float *__restrict__ x, float *__restrict__ x_norm, const float *__restrict__ mean,
                            const float *__restrict__ variance, const float *__restrict__ scales, const float *__restrict__ biases,
                            int act, int group, int C)
{
    // blockIdx.y is the step: the index inside a group fits 32 bits, so the column costs a 32-bit remainder
    const size_t g0 = (size_t)blockIdx.y * group, s0 = (size_t)blockIdx.y * C;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < group; i += gridDim.x * blockDim.x) {
        const int c = i % C;
        const size_t e = g0 + i, st = s0 + c;
        float v = y[e];
        x[e] = v;
        v = (float)((double)(v - mean[st]) / (sqrt((double)variance[st]) + (double).000001f));      // normalize_cpu
        x_norm[e] = v;
        y[e] = activate_any(v * scales[c] + biases[c], act);
    }
}

// One time step of the self sub-layer behind its product, one launch: the step's statistics over its B rows, the rolling
// update, x, x_norm, scale, bias, activation, and the combine with the hoisted input projection into the next state slot.
// A workgroup owns its 32 columns and all B rows, so nothing waits on another workgroup.  mean == nullptr: no batch norm.
__global__ __launch_bounds__(COLS * LANES) void step_finish(float *__restrict__ y, float *__restrict__ x, float *__restrict__ x_norm,
                                                            float *__restrict__ mean, float *__restrict__ variance,
                                                            float *__restrict__ rolling_mean, float *__restrict__ rolling_variance,
                                                            float keep, float take, const float *__restrict__ scales,
                                                            const float *__restrict__ biases, int act, int B, int C,
                                                            const float *__restrict__ proj, float *__restrict__ next)
{
    __shared__ float sh[1][LANES][COLS];
    const int c = blockIdx.x * COLS + threadIdx.x;
    const bool in = c < C, bn = mean != nullptr;
    float m = 0.f, var = 0.f;
    if (bn) {
        float s[1] = { 0.f };
        if (in) for (int r = threadIdx.y; r < B; r += LANES) s[0] += y[(size_t)r * C + c];
        lane_sums(s, sh);
        m = s[0] * (float)(1. / B);                                              // mean_cpu
        s[0] = 0.f;
        if (in) for (int r = threadIdx.y; r < B; r += LANES) { const float d = y[(size_t)r * C + c] - m; s[0] += d * d; }
        lane_sums(s, sh);
        var = s[0] * (float)(1. / (B - 1));                                      // variance_cpu
        if (in && threadIdx.y == 0) {
            mean[c] = m;
            variance[c] = var;
            rolling_mean[c] = rolling_mean[c] * keep + take * m;
            rolling_variance[c] = rolling_variance[c] * keep + take * var;
        }
    }
    if (!in) return;
    const float sc = bn ? scales[c] : 1.f, bias = biases[c];
    for (int r = threadIdx.y; r < B; r += LANES) {
        const size_t e = (size_t)r * C + c;
        float v = y[e];
        if (bn) {
            x[e] = v;
            v = (float)((double)(v - m) / (sqrt((double)var) + (double).000001f));              // normalize_cpu
            x_norm[e] = v;
            v *= sc;
        }
        v = activate_any(v + bias, act);
        y[e] = v;
        next[e] = (0.f + proj[e]) + v;
    }
}

__device__ __forceinline__ float gradient_of(float y, int act)       // activations.h:56-82, on the layer's OUTPUT
{
    switch (act) {
    case Y2H_ACT_LEAKY: return (y > 0) ? 1.f : .1f;
    case Y2H_ACT_LOGISTIC: return (1 - y) * y;
    case Y2H_ACT_RELU: return (float)(y > 0);
    }
    return 1.f;
}

__global__ __launch_bounds__(COLS * LANES) void delta_group(const float *__restrict__ out, float *__restrict__ delta,
                                                            const float *__restrict__ x, const float *__restrict__ x_norm,
                                                            const float *__restrict__ scales, const float *__restrict__ mean,
                                                            const float *__restrict__ variance, int act, int B, int C,
                                                            float *__restrict__ bias_steps, float *__restrict__ scale_steps,
                                                            float *__restrict__ mean_delta, float *__restrict__ variance_delta)
{
    __shared__ float sh[4][LANES][COLS];
    const int c = blockIdx.x * COLS + threadIdx.x, t = blockIdx.y;
    const bool in = c < C, bn = mean != nullptr;
    const size_t g0 = (size_t)t * B * C;
    const float m = (in && bn) ? mean[c] : 0.f, var = (in && bn) ? variance[c] : 1.f, sc = (in && bn) ? scales[c] : 1.f;
    float s[4] = { 0.f, 0.f, 0.f, 0.f };         // bias, scale, mean_delta and variance_delta sums
    if (in) for (int r = threadIdx.y; r < B; r += LANES) {
        const size_t e = g0 + (size_t)r * C + c;
        const float d = delta[e] * gradient_of(out[e], act);                     // gradient_array
        delta[e] = d;
        s[0] += d;
        if (bn) {
            const float ds = d * sc;                                             // scale_bias
            s[1] += d * x_norm[e];                                               // backward_scale_cpu
            s[2] += ds;
            s[3] += ds * (x[e] - m);
        }
    }
    lane_sums(s, sh);
    if (!in) return;
    if (threadIdx.y == 0) {
        bias_steps[(size_t)t * C + c] = s[0];
        if (bn) scale_steps[(size_t)t * C + c] = s[1];
    }
    if (!bn) return;
    const float md = (float)((double)s[2] * (-1. / sqrt((double)(var + .00001f))));                          // mean_delta_cpu
    const float vd = (float)((double)s[3] * (-.5 * pow((double)(var + .00001f), (double)(float)(-3. / 2.))));  // variance_delta_cpu
    if (threadIdx.y == 0 && t == 0) { mean_delta[c] = md; variance_delta[c] = vd; }   // what the reference's arrays hold at the end
    for (int r = threadIdx.y; r < B; r += LANES) {        // normalize_delta_cpu; a lane re-reads the rows it wrote itself
        const size_t e = g0 + (size_t)r * C + c;
        const float d = delta[e] * sc;
        delta[e] = (float)((double)d * 1. / (sqrt((double)var) + (double).00001f) + (double)vd * 2. * (double)(x[e] - m) / (double)B +
                           (double)(md / (float)B));
    }
}

__global__ void sum_steps(const float *__restrict__ steps, int T, int C, float *__restrict__ dst)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float v = dst[c];
    for (int t = T - 1; t >= 0; --t) v += steps[(size_t)t * C + c];
    dst[c] = v;
}

__global__ void combine(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ dst, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) dst[e] = (0.f + a[e]) + b[e];
}

// x[t*B + b][c] = (c == tok[b][t]), y[t*B + b][c] = (c == tok[b][t + 1]); tok is [B][T + 1] bytes, each below C
__global__ void onehot(const unsigned char *__restrict__ tok, int T, int B, int C, float *__restrict__ x, float *__restrict__ y, long n)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long row = e / C;
        const int t = (int)(row / B), b = (int)(row % B);
        const unsigned char *s = tok + (size_t)b * (T + 1) + t;
        x[e] = c == s[0] ? 1.f : 0.f;
        y[e] = c == s[1] ? 1.f : 0.f;
    }
}

// dst[o][k] += src[k][o]: a weight gradient made as [inputs][outputs] (the convolution template's layout) into the
// [outputs][inputs] update buffer; 32 x 32 tiles through LDS so that both sides move whole rows
__global__ __launch_bounds__(256) void add_transposed(float *__restrict__ dst, const float *__restrict__ src, int O, int K)
{
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int k = k0 + r, o = o0 + threadIdx.x;
        tile[r][threadIdx.x] = (k < K && o < O) ? src[(size_t)k * O + o] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int o = o0 + r, k = k0 + threadIdx.x;
        if (o < O && k < K) dst[(size_t)o * K + k] += tile[threadIdx.x][r];
    }
}

// ---- the fused step kernels: one launch per time step forward, two backward ----
// A workgroup is 1024 threads, 16 waves, and owns 32 columns of the self sub-layer and ALL B rows, so the step's batch
// statistics need no other workgroup: nothing waits on another workgroup, a time step is a launch boundary.
// Forward: the waves are 4 row tiles of 32 rows x 4 quarters of K = hidden; each holds one 32 x 32 accumulator tile of
// v_mfma_f32_32x32x2_f32 (16 VGPRs; a lane owns one state row and one weight row and reads 16 consecutive floats of each per
// 32-step, as dense_forward does).  The quarters add their tiles into one [rows][32] LDS tile in quarter order; then the 1024
// threads are 32 columns x 32 row lanes and run step_finish's epilogue from that tile.
// Backward: the 32 x 32 lanes run delta_group's work for the workgroup's 32 outputs and leave the final delta in the LDS tile
// (and in HBM); then wave w takes the (row tile, 32 input columns) pairs w, w + 16, ... of  delta[B][32] x W_self[32][hidden]
// -> partial [range = workgroup][B][hidden]; a second launch adds the partials in range order into delta[t-1].
// The bound (y2h_train_rnn_fused_fits): 4 row tiles of 32 rows -> B <= 128 (a fifth tile would need a second accumulator per
// wave or a 20-wave workgroup); LDS is the tile, 128 x 33 floats, and the 4 x 32 x 33 reduction floats, 33.8 KB of 160 KB;
// the backward partials, hidden / 32 x B x hidden floats, are kept below 256 MiB.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FROWS = 128, FPITCH = 33, FLANES = 32, FQ = 4;

struct Fused {
    const float *in, *w;             // forward: state slot t [B][H]; backward: the self sub-layer's output [B][H]; W_self [H][H]
    float *y, *x, *x_norm, *mean, *variance, *rolling_mean, *rolling_variance;
    const float *scales, *biases, *proj;
    float *next, *delta, *bias_step, *scale_step, *mean_delta, *variance_delta, *ws;
    float keep, take;
    int act, B, H, vec;
};

// sums of N values over the 32 row lanes, lane 0 first; every thread of a column gets the totals
template <int N>
__device__ __forceinline__ void lanes32(float (&v)[N], float (*red)[FLANES][FPITCH], int tx, int ty)
{
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][ty][tx] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float s = red[k][0][tx];
        for (int l = 1; l < FLANES; ++l) s += red[k][l][tx];
        v[k] = s;
    }
}

__global__ __launch_bounds__(1024) void fused_forward(Fused p)
{
    __shared__ float tile[FROWS * FPITCH];
    __shared__ float red[1][FLANES][FPITCH];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int rt = wave & 3, q = wave >> 2, c0 = blockIdx.x * 32, H = p.H, B = p.B, rts = (B + 31) / 32;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    if (rt < rts) {
        const long steps = (H + 31) / 32;
        const int k0 = (int)(q * steps / FQ) * 32, k1 = (q + 1 == FQ) ? H : (int)((q + 1) * steps / FQ) * 32;
        // a row past B / a column past H reads the last one (in bounds); its products land in entries never used
        const int b = rt * 32 + li < B ? rt * 32 + li : B - 1, o = c0 + li < H ? c0 + li : H - 1;
        const float *xr = p.in + (size_t)b * H, *wr = p.w + (size_t)o * H;
        for (int k = k0; k < k1; k += 32) {
            float xa[16], wa[16];
            const int kk = k + 16 * lh;
            if (p.vec && k + 32 <= k1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 xq = *(const f32x4 *)(xr + kk + 4 * j), wq = *(const f32x4 *)(wr + kk + 4 * j);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { xa[4 * j + u] = xq[u]; wa[4 * j + u] = wq[u]; }
                }
            } else {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const bool ok = kk + u < k1;
                    xa[u] = ok ? xr[kk + u] : 0.f;
                    wa[u] = ok ? wr[kk + u] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u], wa[u], acc, 0, 0, 0);
        }
    }
    for (int qq = 0; qq < FQ; ++qq) {                    // the K quarters, in quarter order
        if (q == qq && rt < rts) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = rt * 32 + (v >> 2) * 8 + lh * 4 + (v & 3);
                tile[row * FPITCH + li] = qq ? tile[row * FPITCH + li] + acc[v] : acc[v];
            }
        }
        __syncthreads();
    }
    // step_finish's epilogue, the product read from the tile
    const int tx = t & 31, ty = t >> 5, c = c0 + tx;
    const bool in = c < H, bn = p.mean != nullptr;
    float m = 0.f, var = 0.f;
    if (bn) {
        float s[1] = { 0.f };
        if (in) for (int r = ty; r < B; r += FLANES) s[0] += tile[r * FPITCH + tx];
        lanes32(s, red, tx, ty);
        m = s[0] * (float)(1. / B);
        s[0] = 0.f;
        if (in) for (int r = ty; r < B; r += FLANES) { const float d = tile[r * FPITCH + tx] - m; s[0] += d * d; }
        lanes32(s, red, tx, ty);
        var = s[0] * (float)(1. / (B - 1));
        if (in && ty == 0) {
            p.mean[c] = m;
            p.variance[c] = var;
            p.rolling_mean[c] = p.rolling_mean[c] * p.keep + p.take * m;
            p.rolling_variance[c] = p.rolling_variance[c] * p.keep + p.take * var;
        }
    }
    if (!in) return;
    const float sc = bn ? p.scales[c] : 1.f, bias = p.biases[c];
    for (int r = ty; r < B; r += FLANES) {
        const size_t e = (size_t)r * H + c;
        float v = tile[r * FPITCH + tx];
        if (bn) {
            p.x[e] = v;
            v = (float)((double)(v - m) / (sqrt((double)var) + (double).000001f));
            p.x_norm[e] = v;
            v *= sc;
        }
        v = activate_any(v + bias, p.act);
        p.y[e] = v;
        p.next[e] = (0.f + p.proj[e]) + v;
    }
}

__device__ __forceinline__ float fused_gradient(float y, int act)
{
    switch (act) {
    case Y2H_ACT_LEAKY: return (y > 0) ? 1.f : .1f;
    case Y2H_ACT_LOGISTIC: return (1 - y) * y;
    case Y2H_ACT_RELU: return (float)(y > 0);
    }
    return 1.f;
}

__global__ __launch_bounds__(1024) void fused_backward(Fused p)
{
    __shared__ float tile[FROWS * FPITCH];
    __shared__ float red[4][FLANES][FPITCH];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5, o0 = blockIdx.x * 32, c = o0 + tx, H = p.H, B = p.B;
    const bool in = c < H, bn = p.mean != nullptr;
    const float m = (in && bn) ? p.mean[c] : 0.f, var = (in && bn) ? p.variance[c] : 1.f, sc = (in && bn) ? p.scales[c] : 1.f;
    float s[4] = { 0.f, 0.f, 0.f, 0.f };
    for (int r = ty; r < B; r += FLANES) {
        float d = 0.f;
        if (in) {
            const size_t e = (size_t)r * H + c;
            d = p.delta[e] * fused_gradient(p.in[e], p.act);
            s[0] += d;
            if (bn) {
                const float ds = d * sc;
                s[1] += d * p.x_norm[e];
                s[2] += ds;
                s[3] += ds * (p.x[e] - m);
            }
        }
        tile[r * FPITCH + tx] = d;                         // a column past H holds zeros: it adds nothing to the product
    }
    lanes32(s, red, tx, ty);
    if (in && ty == 0) {
        p.bias_step[c] = s[0];
        if (bn) p.scale_step[c] = s[1];
    }
    if (bn) {
        const float md = (float)((double)s[2] * (-1. / sqrt((double)(var + .00001f))));
        const float vd = (float)((double)s[3] * (-.5 * pow((double)(var + .00001f), (double)(float)(-3. / 2.))));
        if (in && ty == 0) { p.mean_delta[c] = md; p.variance_delta[c] = vd; }
        if (in) for (int r = ty; r < B; r += FLANES) {     // a lane re-reads the rows it wrote itself
            const float d = tile[r * FPITCH + tx] * sc;
            tile[r * FPITCH + tx] = (float)((double)d * 1. / (sqrt((double)var) + (double).00001f) +
                                            (double)vd * 2. * (double)(p.x[(size_t)r * H + c] - m) / (double)B + (double)(md / (float)B));
        }
    }
    if (in) for (int r = ty; r < B; r += FLANES) p.delta[(size_t)r * H + c] = tile[r * FPITCH + tx];
    __syncthreads();
    if (!p.ws) return;                                      // step 0: no input gradient
    const int wave = t >> 6, lane = t & 63, li = lane & 31, lh = lane >> 5, rts = (B + 31) / 32, kts = (H + 31) / 32;
    for (int id = wave; id < rts * kts; id += 16) {
        const int rt = id % rts, col = (id / rts) * 32 + li;
        const int arow = rt * 32 + li < B ? rt * 32 + li : B - 1;      // rows past B: results never stored
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int oo = o0 + 2 * u + lh;
            const float wv = (oo < H && col < H) ? p.w[(size_t)oo * H + col] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[arow * FPITCH + 2 * u + lh], wv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = rt * 32 + (v >> 2) * 8 + lh * 4 + (v & 3);
            if (row < B && col < H) p.ws[((size_t)blockIdx.x * B + row) * H + col] = acc[v];
        }
    }
}

// dprev[e] += the partials in range order
__global__ void fused_reduce(const float *__restrict__ ws, float *__restrict__ dprev, long n, int ranges)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float s = ws[e];
        for (int r = 1; r < ranges; ++r) s += ws[(size_t)r * n + e];
        dprev[e] += s;
    }
}

inline bool groups_ok(int T, int B, int C) { return T > 0 && T <= 65535 && B > 0 && C > 0 && (long)T * B * C < (1L << 40); }

}  // namespace

extern "C" {

int y2h_train_rnn_bn_stats(const float *x, int T, int B, int C, float *mean, float *variance, float *rolling_mean,
                           float *rolling_variance, float keep, float take, y2h_stream s)
{
    if (!x || !mean || !variance || !rolling_mean || !rolling_variance || !groups_ok(T, B, C) || B < 2) return Y2H_EINVAL;
    group_stats<<<dim3((C + COLS - 1) / COLS, T), dim3(COLS, LANES), 0, S(s)>>>(x, B, C, mean, variance);
    Y2H_LAUNCH_CHECK();
    roll_stats<<<(C + 63) / 64, 64, 0, S(s)>>>(mean, variance, T, C, rolling_mean, rolling_variance, keep, take);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_bn_apply(float *y, float *x, float *x_norm, const float *mean, const float *variance, const float *scales,
                           const float *biases, int act, int T, int B, int C, y2h_stream s)
{
    if (!y || !x || !x_norm || !mean || !variance || !scales || !biases || !groups_ok(T, B, C)) return Y2H_EINVAL;
    if ((long)B * C >= 2147483647L - 256L * 4096) return Y2H_EINVAL;
    group_apply<<<dim3(y2h_grid((long)B * C, 256), T), 256, 0, S(s)>>>(y, x, x_norm, mean, variance, scales, biases, act, B * C, C);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_fused_fits(int B, int hidden)
{
    if (B < 1 || hidden < 1) return 0;
    if (B > FROWS) return 0;                                              // 4 row tiles of 32 rows, one accumulator tile per wave
    if ((size_t)(FROWS * FPITCH + 4 * FLANES * FPITCH) * sizeof(float) > 160u * 1024) return 0;      // LDS per CU
    if ((hidden + 31) / 32 > 65535) return 0;
    if (y2h_train_rnn_fused_ws_bytes(B, hidden) > ((size_t)256 << 20)) return 0;
    return 1;
}

size_t y2h_train_rnn_fused_ws_bytes(int B, int hidden)
{
    if (B < 1 || hidden < 1) return 0;
    return (size_t)((hidden + 31) / 32) * B * hidden * sizeof(float);
}

int y2h_train_rnn_fused_forward(const float *state, const float *w, float *y, float *x, float *x_norm, float *mean, float *variance,
                                float *rolling_mean, float *rolling_variance, float keep, float take, const float *scales,
                                const float *biases, int act, int B, int H, const float *proj, float *next, y2h_stream s)
{
    if (!state || !w || !y || !biases || !proj || !next || !y2h_train_rnn_fused_fits(B, H)) return Y2H_EINVAL;
    if (mean && (!x || !x_norm || !variance || !rolling_mean || !rolling_variance || !scales || B < 2)) return Y2H_EINVAL;
    Fused p = {};
    p.in = state; p.w = w; p.y = y; p.x = x; p.x_norm = x_norm; p.mean = mean; p.variance = variance;
    p.rolling_mean = rolling_mean; p.rolling_variance = rolling_variance; p.scales = scales; p.biases = biases; p.proj = proj;
    p.next = next; p.keep = keep; p.take = take; p.act = act; p.B = B; p.H = H;
    p.vec = H % 4 == 0 && (((uintptr_t)state | (uintptr_t)w) % 16) == 0;
    fused_forward<<<(H + 31) / 32, 1024, 0, S(s)>>>(p);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_fused_backward(const float *out, float *delta, const float *x, const float *x_norm, const float *scales,
                                 const float *mean, const float *variance, int act, int B, int H, const float *w, float *bias_step,
                                 float *scale_step, float *mean_delta, float *variance_delta, float *dprev, float *ws, y2h_stream s)
{
    if (!out || !delta || !bias_step || !y2h_train_rnn_fused_fits(B, H)) return Y2H_EINVAL;
    if (mean && (!x || !x_norm || !scales || !variance || !scale_step || !mean_delta || !variance_delta)) return Y2H_EINVAL;
    if (dprev && (!w || !ws)) return Y2H_EINVAL;
    Fused p = {};
    p.in = out; p.w = w; p.delta = delta; p.x = const_cast<float *>(x); p.x_norm = const_cast<float *>(x_norm); p.scales = scales;
    p.mean = const_cast<float *>(mean); p.variance = const_cast<float *>(variance); p.act = act; p.B = B; p.H = H;
    p.bias_step = bias_step; p.scale_step = scale_step; p.mean_delta = mean_delta; p.variance_delta = variance_delta;
    p.ws = dprev ? ws : nullptr;
    const int ranges = (H + 31) / 32;
    fused_backward<<<ranges, 1024, 0, S(s)>>>(p);
    Y2H_LAUNCH_CHECK();
    if (dprev) {
        const long n = (long)B * H;
        fused_reduce<<<y2h_grid(n, 256), 256, 0, S(s)>>>(ws, dprev, n, ranges);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}

int y2h_train_rnn_step_finish(float *y, float *x, float *x_norm, float *mean, float *variance, float *rolling_mean,
                              float *rolling_variance, float keep, float take, const float *scales, const float *biases, int act,
                              int B, int C, const float *proj, float *next, y2h_stream s)
{
    if (!y || !biases || !proj || !next || !groups_ok(1, B, C)) return Y2H_EINVAL;
    if (mean && (!x || !x_norm || !variance || !rolling_mean || !rolling_variance || !scales || B < 2)) return Y2H_EINVAL;
    step_finish<<<dim3((C + COLS - 1) / COLS), dim3(COLS, LANES), 0, S(s)>>>(y, x, x_norm, mean, variance, rolling_mean, rolling_variance,
                                                                           keep, take, scales, biases, act, B, C, proj, next);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_delta(const float *out, float *delta, const float *x, const float *x_norm, const float *scales, const float *mean,
                        const float *variance, int act, int T, int B, int C, float *bias_steps, float *scale_steps,
                        float *mean_delta, float *variance_delta, y2h_stream s)
{
    if (!out || !delta || !bias_steps || !groups_ok(T, B, C)) return Y2H_EINVAL;
    if (mean && (!x || !x_norm || !scales || !variance || !scale_steps || !mean_delta || !variance_delta)) return Y2H_EINVAL;
    delta_group<<<dim3((C + COLS - 1) / COLS, T), dim3(COLS, LANES), 0, S(s)>>>(out, delta, x, x_norm, scales, mean, variance, act, B, C,
                                                                              bias_steps, scale_steps, mean_delta, variance_delta);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_sum_steps(const float *steps, int T, int C, float *dst, y2h_stream s)
{
    if (!steps || !dst || T <= 0 || C <= 0) return Y2H_EINVAL;
    sum_steps<<<(C + 63) / 64, 64, 0, S(s)>>>(steps, T, C, dst);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_combine(const float *a, const float *b, float *dst, long n, y2h_stream s)
{
    if (!a || !b || !dst || n <= 0) return Y2H_EINVAL;
    combine<<<y2h_grid(n, 256), 256, 0, S(s)>>>(a, b, dst, n);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_add_transposed(float *dst, const float *src, int outputs, int inputs, y2h_stream s)
{
    if (!dst || !src || outputs <= 0 || inputs <= 0 || (outputs + 31) / 32 > 65535) return Y2H_EINVAL;
    add_transposed<<<dim3((inputs + 31) / 32, (outputs + 31) / 32), dim3(32, 8), 0, S(s)>>>(dst, src, outputs, inputs);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2h_train_rnn_onehot(const unsigned char *tok, int T, int B, int C, float *x, float *y, y2h_stream s)
{
    if (!tok || !x || !y || !groups_ok(T, B, C)) return Y2H_EINVAL;
    const long n = (long)T * B * C;
    onehot<<<y2h_grid(n, 256), 256, 0, S(s)>>>(tok, T, B, C, x, y, n);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

}  // extern "C"
