// [rnn] / [gru] time steps (include/y2_hip.h y2h_rec_step).  Compiled with -ffp-contract=off: the epilogue and the
// combines follow the reference's operation order, each product and sum rounded on its own.
//
// At batch 1 a step is a 1024 x 1024 matrix-vector product: 4 MB of weights against 4 KB of state.  The skinny kernel
// streams the weights once per step; a step's cost is its launch and the weight stream (L2 / Infinity Cache), not
// arithmetic.
#include "y2_common.hpp"

namespace {

// the sub-layer's epilogue: forward_connected_layer (connected_layer.c:122-155) after the gemm
__device__ __forceinline__ float rec_epilogue(const y2h_rec_args &a, int j, float v)
{
    if (a.bn) {
        const float d = v - a.mean[j];                  // normalize_cpu (blas.c:122), the divisor in double
        v = (float)((double)d * a.rinv[j]);
        v = v * a.scale[j];                             // scale_bias
    }
    v = v + a.bias[j];                                  // add_bias / axpy
    return activate_any(v, a.act);
}

__device__ __forceinline__ float sigma(float x) { return (float)(1. / (1. + exp(-(double)x))); }   // activations.h:35

// the mode's combine for row r, column j of the dense product (value v after the epilogue)
__device__ __forceinline__ void rec_combine(const y2h_rec_args &a, int r, int j, float v)
{
    const int h = a.h;
    switch (a.mode) {
    case Y2H_REC_DENSE:
        a.out[(size_t)r * a.n + j] = v;
        break;
    case Y2H_REC_RNN: {                                 // rnn_layer.c:103-111: fill/copy, axpy(in), axpy(self)
        const size_t o = (size_t)r * h + j;
        const float base = a.shortcut ? a.state[o] : 0.f;
        const float s = (base + a.proj[o]) + v;
        a.out[o] = s;
        if (a.out2) a.out2[o] = s;
    } break;
    case Y2H_REC_GRU_ZR:                                // gru_layer.c:152-163: z = iz + sz, r = ir + sr, sigma, f = state * r
        if (j < h) a.out[(size_t)r * h + j] = sigma(a.proj[(size_t)r * 3 * h + j] + v);
        else {
            const int c = j - h;
            const float rr = sigma(a.proj[(size_t)r * 3 * h + h + c] + v);
            a.out2[(size_t)r * h + c] = a.state[(size_t)r * h + c] * rr;
        }
        break;
    case Y2H_REC_GRU_H: {                               // gru_layer.c:165-178, weighted_sum_cpu (blas.c:49-55)
        const size_t o = (size_t)r * h + j;
        const float hh = sigma(a.proj[(size_t)r * 3 * h + 2 * h + j] + v);
        const float z = a.z[o], st = a.state[o];
        const float y = z * st + (1 - z) * hh;
        a.out[o] = y;
        a.out2[o] = y;
    } break;
    }
}

// one thread per (row, column): the dot product in gemm_nt's order (0 + sum, product and sum rounded separately), or the
// value another kernel produced (`pre`)
__global__ __launch_bounds__(256) void rec_ref_kernel(y2h_rec_args a)
{
    const long total = (long)a.rows * a.n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int j = (int)(idx % a.n), r = (int)(idx / a.n);
        float v;
        if (a.pre) v = a.pre[idx];
        else {
            const float *xr = a.x + (size_t)r * a.k, *wr = a.w + (size_t)j * a.k;
            float sum = 0.f;
            for (int q = 0; q < a.k; ++q) {
                const float prod = xr[q] * wr[q];
                sum = sum + prod;
            }
            v = rec_epilogue(a, j, 0.f + sum);
        }
        rec_combine(a, r, j, v);
    }
    if (a.xcopy)
        for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < (long)a.rows * a.k; idx += (long)gridDim.x * 256) a.xcopy[idx] = a.x[idx];
}

// Weight streaming for up to MB rows.  A workgroup of W waves owns W columns, wave w column W*g + w.  The x rows sit in
// LDS ([rows][k], staged once per workgroup); lane l reads the 16-byte chunks l, l+64, ... of the column's weight row.
// Per row the 64 partial sums are combined by a fixed xor butterfly, so the result does not depend on timing.  Staging
// reads rows*k*4 bytes per workgroup against W*k*4 bytes of weights, so W grows with the rows (rec_waves): the staging
// stays at most half of the weight stream (a loop over several columns per wave instead spills scalar registers at
// 8 rows).
__host__ __device__ constexpr int rec_waves(int mb) { return mb >= 4 ? 16 : 4; }

template <int MB, bool VEC>
__global__ __launch_bounds__(64 * rec_waves(MB)) void rec_skinny_kernel(y2h_rec_args a)
{
    constexpr int NT = 64 * rec_waves(MB);
    extern __shared__ float xs[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nx = a.rows * a.k;
    if (VEC) {
        const float4 *src = (const float4 *)a.x;
        for (int i = tid; i < (nx >> 2); i += NT) ((float4 *)xs)[i] = src[i];
    } else {
        for (int i = tid; i < nx; i += NT) xs[i] = a.x[i];
    }
    __syncthreads();
    if (a.xcopy && blockIdx.x == 0)
        for (int i = tid; i < nx; i += NT) a.xcopy[i] = xs[i];
    {
        const int j = blockIdx.x * rec_waves(MB) + (tid >> 6);
        if (j >= a.n) return;
        float acc[MB];
#pragma unroll
        for (int r = 0; r < MB; ++r) acc[r] = 0.f;
        const float *wr = a.w + (size_t)j * a.k;
        if (VEC) {
            const int k4 = a.k >> 2;
#pragma unroll 4
            for (int q = lane; q < k4; q += 64) {
                const float4 w4 = ((const float4 *)wr)[q];     // plain loads: the next step wants this row in L2 again
#pragma unroll
                for (int r = 0; r < MB; ++r) {
                    if (r < a.rows) {
                        const float4 x4 = ((const float4 *)(xs + (size_t)r * a.k))[q];
                        acc[r] += w4.x * x4.x;
                        acc[r] += w4.y * x4.y;
                        acc[r] += w4.z * x4.z;
                        acc[r] += w4.w * x4.w;
                    }
                }
            }
        } else {
            for (int q = lane; q < a.k; q += 64) {
                const float w1 = wr[q];
#pragma unroll
                for (int r = 0; r < MB; ++r)
                    if (r < a.rows) acc[r] += w1 * xs[(size_t)r * a.k + q];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int r = 0; r < MB; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
        // lane r finishes row r (a compile-time select chain: no dynamically indexed register array)
        float v = acc[0];
#pragma unroll
        for (int r = 1; r < MB; ++r) v = (lane == r) ? acc[r] : v;
        if (lane < a.rows) rec_combine(a, lane, j, rec_epilogue(a, j, v));
    }
}

template <int MB>
hipError_t launch_skinny(const y2h_rec_args &a, hipStream_t s)
{
    const size_t lds = (size_t)a.rows * a.k * sizeof(float);
    const bool vec = (a.k % 4) == 0 && ((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.w % 16) == 0;
    const void *fn = vec ? (const void *)rec_skinny_kernel<MB, true> : (const void *)rec_skinny_kernel<MB, false>;
    hipError_t e = y2h_lds_limit(fn, lds);
    if (e != hipSuccess) return e;
    constexpr int W = rec_waves(MB);
    const dim3 grid((unsigned)((a.n + W - 1) / W));
    if (vec) hipLaunchKernelGGL((rec_skinny_kernel<MB, true>), grid, dim3(64 * W), lds, s, a);
    else hipLaunchKernelGGL((rec_skinny_kernel<MB, false>), grid, dim3(64 * W), lds, s, a);
    return hipSuccess;
}

// ---- character generation and scoring (include/y2_hip.h y2h_rnn_*) ----
// The per-character loop of test_char_rnn (rnn.c:266-278) without a host round trip: the sampled character becomes the
// next input row in HBM.  All three kernels are latency-bound; none waits on another workgroup.

// One workgroup per sequence b: rnn.c:273-275 (threshold) and sample_array (utils.c:520-531) on row b of the network's
// output.  The workgroup thresholds the row into LDS; the two ordered fp32 reductions -- sum_array's ascending sum from 0
// (utils.c:407) and the running subtraction that decides the index -- are then walked by one thread in the reference's
// order, eight values per LDS round trip (the walk is what this kernel costs: a dependent chain of n adds and n
// subtractions).  scale_array's product a[i] * s is formed where the subtraction reads it: the same fp32 product, rounded
// on its own (-ffp-contract=off).  The row itself is only read; `probs`, if set, gets it as the network produced it.
#define Y2_DRAW(val, idx) do { r = r - (val) * s; if (c < 0 && r <= 0) c = (idx); } while (0)
__global__ __launch_bounds__(256) void rec_sample_kernel(const float *out, int ld, int n, const float *u, const int *prev,
                                                         int *next, float *x, float *probs)
{
    extern __shared__ float4 sv4[];
    float *sv = (float *)sv4;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *row = out + (size_t)b * ld;
    for (int i = tid; i < n; i += 256) {
        const float v = row[i];
        sv[i] = ((double)v < .0001) ? 0.f : v;              // rnn.c:274, compared in double
    }
    if (probs)
        for (int i = tid; i < ld; i += 256) probs[(size_t)b * ld + i] = row[i];
    __syncthreads();
    if (tid != 0) return;
    float sum = 0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        const float4 p = sv4[i >> 2], q = sv4[(i >> 2) + 1];
        sum += p.x; sum += p.y; sum += p.z; sum += p.w;
        sum += q.x; sum += q.y; sum += q.z; sum += q.w;
    }
    for (; i < n; ++i) sum += sv[i];
    const float s = (float)(1. / sum);                      // scale_array's float argument: the divide in double
    float r = u[b];
    int c = -1;                                             // the first i with r <= 0; later subtractions do not move it
    for (i = 0; i + 8 <= n && c < 0; i += 8) {
        const float4 p = sv4[i >> 2], q = sv4[(i >> 2) + 1];
        Y2_DRAW(p.x, i); Y2_DRAW(p.y, i + 1); Y2_DRAW(p.z, i + 2); Y2_DRAW(p.w, i + 3);
        Y2_DRAW(q.x, i + 4); Y2_DRAW(q.y, i + 5); Y2_DRAW(q.z, i + 6); Y2_DRAW(q.w, i + 7);
    }
    for (; i < n && c < 0; ++i) Y2_DRAW(sv[i], i);
    if (c < 0) c = n - 1;                                   // nothing qualifies (a zero or NaN sum too): utils.c:530
    x[(size_t)b * n + prev[b]] = 0.f;                       // rnn.c:269, 267: the one-hot row, in place
    x[(size_t)b * n + c] = 1.f;
    next[b] = c;
}
#undef Y2_DRAW

// x[r][j] = (tok[r] == j): the one-hot input rows of one forward, step-major like tok
__global__ __launch_bounds__(256) void rec_feed_kernel(const int *tok, float *x, int rows, int inputs)
{
    const long total = (long)rows * inputs;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int r = (int)(idx / inputs), j = (int)(idx - (long)r * inputs);
        x[idx] = (tok[r] == j) ? 1.f : 0.f;
    }
}

// p_next[r] = out[r][next[r]] (rnn.c:414 reads out[next]); probs, if set, gets every row
__global__ __launch_bounds__(256) void rec_score_kernel(const float *out, int ld, const int *next, int rows, float *p_next, float *probs)
{
    const long total = probs ? (long)rows * ld : rows;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        if (idx < rows) p_next[idx] = out[idx * ld + next[idx]];
        if (probs) probs[idx] = out[idx];
    }
}

}  // namespace

// rows bounded by the accumulators a lane keeps (16 rows spill scalar registers), the staged rows by 64 KB of LDS
extern "C" int y2h_rec_skinny_ok(int rows, int k)
{
    return rows >= 1 && rows <= Y2H_REC_SKINNY_MAX_ROWS && k >= 1 && (size_t)rows * k * sizeof(float) <= 65536;
}

extern "C" int y2h_rec_step(const y2h_rec_args *a, int form, y2h_stream s)
{
    if (!a || !a->out || a->rows <= 0 || a->n <= 0 || a->mode < Y2H_REC_DENSE || a->mode > Y2H_REC_GRU_H) return Y2H_EINVAL;
    if (!a->pre && (!a->x || !a->w || !a->bias || a->k <= 0)) return Y2H_EINVAL;
    if (!a->pre && a->bn && (!a->mean || !a->rinv || !a->scale)) return Y2H_EINVAL;
    if (a->act < 0 || a->act > Y2H_ACT_LHTAN) return Y2H_EINVAL;
    if (a->mode != Y2H_REC_DENSE && (!a->proj || !a->state || a->h <= 0)) return Y2H_EINVAL;
    if (a->mode == Y2H_REC_RNN && a->n != a->h) return Y2H_EINVAL;
    if (a->mode == Y2H_REC_GRU_ZR && (a->n != 2 * a->h || !a->out2)) return Y2H_EINVAL;
    if (a->mode == Y2H_REC_GRU_H && (a->n != a->h || !a->out2 || !a->z)) return Y2H_EINVAL;
    if (form == Y2H_REC_SKINNY) {
        if (a->pre || !y2h_rec_skinny_ok(a->rows, a->k)) return Y2H_EINVAL;
        hipError_t e;
        if (a->rows <= 1) e = launch_skinny<1>(*a, S(s));
        else if (a->rows <= 2) e = launch_skinny<2>(*a, S(s));
        else if (a->rows <= 4) e = launch_skinny<4>(*a, S(s));
        else e = launch_skinny<8>(*a, S(s));
        Y2H_CHECK(e);
    } else if (form == Y2H_REC_REF) {
        hipLaunchKernelGGL(rec_ref_kernel, dim3(y2h_grid((long)a->rows * a->n, 256)), dim3(256), 0, S(s), *a);
    } else return Y2H_EINVAL;
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

static unsigned long g_sample_launches = 0;
extern "C" unsigned long y2h_rnn_sample_launches(void) { return g_sample_launches; }

extern "C" int y2h_rnn_sample(const float *out, int outputs, int n, int seqs, const float *u, const int *prev, int *next,
                              float *x, float *probs, y2h_stream s)
{
    const size_t lds = ((size_t)n + 3) / 4 * sizeof(float4);
    if (!out || !u || !prev || !next || !x || seqs <= 0 || n <= 0 || n > outputs || lds > 65536) return Y2H_EINVAL;
    Y2H_CHECK(y2h_lds_limit((const void *)rec_sample_kernel, lds));
    hipLaunchKernelGGL(rec_sample_kernel, dim3((unsigned)seqs), dim3(256), lds, S(s), out, outputs, n, u, prev, next, x, probs);
    Y2H_LAUNCH_CHECK();
    ++g_sample_launches;
    return Y2H_OK;
}

extern "C" int y2h_rnn_feed(const int *tok, float *x, int rows, int inputs, y2h_stream s)
{
    if (!tok || !x || rows <= 0 || inputs <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(rec_feed_kernel, dim3(y2h_grid((long)rows * inputs, 256)), dim3(256), 0, S(s), tok, x, rows, inputs);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_rnn_score(const float *out, int outputs, const int *next, int rows, float *p_next, float *probs, y2h_stream s)
{
    if (!out || !next || !p_next || rows <= 0 || outputs <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(rec_score_kernel, dim3(y2h_grid(probs ? (long)rows * outputs : rows, 256)), dim3(256), 0, S(s), out, outputs,
                       next, rows, p_next, probs);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
