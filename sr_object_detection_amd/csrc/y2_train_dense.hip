// Training kernels of a dense ([connected]) layer (gfx950): the three products of connected_layer.c:122-190 on the fp32
// matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulation), fp32 in and out in every training
// precision -- y2_train_set_precision steers the convolutions' products only.
//
//   forward   y[b][o]   = sum_k x[b][k] * w[o][k]
//   dweight   dw[o][k] += sum_b d[b][o] * x[b][k]
//   dinput    dx[b][k]  = sum_o d[b][o] * w[o][k]        (or += : `add`)
//
// batch is small and the weights are the traffic (tiny-yolo-v1: 1470 x 12544 floats, 73.7 MB, against 32 rows), so every
// kernel is laid out around one pass over w / dw, and the 64 x 64 tile of train_gemm, which would put the forward product
// on 23 workgroups, is not used:
//   forward   one wave per (32 outputs, K range).  A lane owns one weight row and one x row and reads 16 consecutive floats
//             of each per 32-step (the order of k inside a sum is free as long as both operands agree), the next step's
//             loads fly under this step's MFMAs.  The K ranges are whole 32-steps; with more than one, range r writes its
//             raw sums to ws[r][batch][outputs] and a second launch adds them in ascending range order.
//   dinput    one workgroup per (128 inputs, range of outputs): four waves share 64 outputs of d at a time through LDS,
//             each streams its own 32 columns of w (128 contiguous bytes per weight row).  Ranges and second pass as above.
//   dweight   a rank-`batch` update: one wave per (32 outputs, 32 inputs) reads d and x (small; they stay in L2), and reads
//             and writes every weight-gradient element once.
// Rows beyond 32 run as further row passes (grid.y) of forward and dinput; dweight walks all rows.  Edges (rows, outputs,
// inputs, the ranges' tails) are guarded in the loads and stores: every batch, inputs, outputs >= 1 takes these kernels.
// No floating-point atomics: the result depends on the shape (and Y2_TRAIN_DENSE_KSPLIT) alone.
#include "y2_common.hpp"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int ROWS = 32;          // rows of one pass: the matrix instruction's M
constexpr int KSTEP = 32;         // forward: k per trip, the granule of its ranges
constexpr int OSTEP = 64;         // dinput: outputs per LDS chunk, the granule of its ranges
constexpr int LDA = OSTEP + 1;    // LDS row pitch of the d chunk

// range r of `ranges` over the `step`-granules of `total`: whole granules, dealt as evenly as integers allow; the last
// range also takes the tail shorter than a granule
__host__ __device__ inline void range_of(int total, int step, int ranges, int r, int *lo, int *hi)
{
    const long steps = (total + step - 1) / step;
    *lo = (int)(r * steps / ranges) * step;
    *hi = (r + 1 == ranges) ? total : (int)((r + 1) * steps / ranges) * step;
}

struct Dense {
    const float *a;               // the small operand: x (forward, dweight: also d in `d`) or d (dinput)
    const float *d;
    const float *w;               // [outputs][inputs]
    float *dst, *ws;
    int batch, inputs, outputs, ranges, tiles, add;
};

// the tile of one wave: acc[v] is row (v >> 2) * 8 + lh * 4 + (v & 3), column li
__device__ __forceinline__ void store_tile(const Dense &p, const f32x16 &acc, int r, int row0, int rows, int col, int cols, int lh)
{
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = row0 + (v >> 2) * 8 + lh * 4 + (v & 3);
        if (row >= rows || col >= cols) continue;
        const size_t e = (size_t)row * cols + col;
        if (p.ranges > 1) p.ws[(size_t)r * rows * cols + e] = acc[v];
        else p.dst[e] = p.add ? p.dst[e] + acc[v] : acc[v];
    }
}

// VEC: inputs % 4 == 0 and 16-byte aligned x and w, so a whole step is four 16-byte loads per operand; a step that crosses
// the range's end, and every step otherwise, takes the same elements one by one behind their guards
template <bool VEC>
__global__ __launch_bounds__(256) void dense_forward(Dense p)
{
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)p.tiles * p.ranges) return;
    const int tile = (int)(item % p.tiles), r = (int)(item / p.tiles);
    const int b0 = blockIdx.y * ROWS, o0 = tile * ROWS;
    int k0, k1;
    range_of(p.inputs, KSTEP, p.ranges, r, &k0, &k1);
    // a row past the batch / the outputs reads the last one (in bounds); its products land in tile entries never stored
    const int b = b0 + li < p.batch ? b0 + li : p.batch - 1, o = o0 + li < p.outputs ? o0 + li : p.outputs - 1;
    const float *xr = p.a + (size_t)b * p.inputs, *wr = p.w + (size_t)o * p.inputs;

    float xa[16], wa[16], xb[16], wb[16];
    auto fetch = [&](int k, float *xv, float *wv) {
        const int kk = k + 16 * lh;
        if (VEC && k + KSTEP <= k1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 xq = *(const f32x4 *)(xr + kk + 4 * q), wq = *(const f32x4 *)(wr + kk + 4 * q);
#pragma unroll
                for (int u = 0; u < 4; ++u) { xv[4 * q + u] = xq[u]; wv[4 * q + u] = wq[u]; }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const bool ok = kk + u < k1;
                xv[u] = ok ? xr[kk + u] : 0.f;
                wv[u] = ok ? wr[kk + u] : 0.f;
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    if (k0 < k1) fetch(k0, xa, wa);
    for (int k = k0; k < k1; k += 2 * KSTEP) {
        if (k + KSTEP < k1) fetch(k + KSTEP, xb, wb);
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u], wa[u], acc, 0, 0, 0);
        if (k + KSTEP >= k1) break;
        if (k + 2 * KSTEP < k1) fetch(k + 2 * KSTEP, xa, wa);
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[u], wb[u], acc, 0, 0, 0);
    }
    store_tile(p, acc, r, b0, p.batch, o0 + li, p.outputs, lh);
}

__global__ __launch_bounds__(256) void dense_dinput(Dense p)
{
    __shared__ float As[ROWS * LDA];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int b0 = blockIdx.y * ROWS, r = blockIdx.z;
    const int col = blockIdx.x * 4 * ROWS + wave * ROWS + li;
    int o0, o1;
    range_of(p.outputs, OSTEP, p.ranges, r, &o0, &o1);
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int o = o0; o < o1; o += OSTEP) {
        float wv[OSTEP / 2];
#pragma unroll
        for (int c = 0; c < OSTEP / 2; ++c) {
            const int oo = o + 2 * c + lh;
            wv[c] = (oo < o1 && col < p.inputs) ? p.w[(size_t)oo * p.inputs + col] : 0.f;
        }
        __syncthreads();                                  // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < ROWS * OSTEP / 256; ++e) {
            const int idx = t + 256 * e, rr = idx / OSTEP, cc = idx % OSTEP;
            As[rr * LDA + cc] = (b0 + rr < p.batch && o + cc < o1) ? p.a[(size_t)(b0 + rr) * p.outputs + o + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < OSTEP / 2; ++c)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[li * LDA + 2 * c + lh], wv[c], acc, 0, 0, 0);
    }
    store_tile(p, acc, r, b0, p.batch, col, p.inputs, lh);
}

__global__ __launch_bounds__(256) void dense_dweight(Dense p)
{
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int k0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS, o0 = blockIdx.y * ROWS;
    if (k0 >= p.inputs) return;
    const int o = o0 + li, col = k0 + li;
    float old[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {                        // the read of the read-modify-write flies under the product
        const int row = o0 + (v >> 2) * 8 + lh * 4 + (v & 3);
        old[v] = (row < p.outputs && col < p.inputs) ? p.dst[(size_t)row * p.inputs + col] : 0.f;
    }
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int b = 0; b < p.batch; b += 16) {               // sixteen rows' loads in flight; rows past the batch are zero
        float dv[8], xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int bb = b + 2 * u + lh;
            dv[u] = (bb < p.batch && o < p.outputs) ? p.d[(size_t)bb * p.outputs + o] : 0.f;
            xv[u] = (bb < p.batch && col < p.inputs) ? p.a[(size_t)bb * p.inputs + col] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[u], xv[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = o0 + (v >> 2) * 8 + lh * 4 + (v & 3);
        if (row < p.outputs && col < p.inputs) p.dst[(size_t)row * p.inputs + col] = old[v] + acc[v];
    }
}

// dst[e] (+)= the partial sums of ws in range order
__global__ void dense_finish(const float *__restrict__ ws, float *__restrict__ dst, long n, int ranges, int add)
{
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float s = ws[e];
        for (int k = 1; k < ranges; ++k) s += ws[(size_t)k * n + e];
        dst[e] = add ? dst[e] + s : s;
    }
}

inline bool shape_ok(const y2h_train_dense *g)
{
    return g && g->batch > 0 && g->inputs > 0 && g->outputs > 0 && (long)g->batch * g->inputs < 2147483647L &&
           (long)g->batch * g->outputs < 2147483647L && (long)(g->batch + ROWS - 1) / ROWS <= 65535 &&
           (long)(g->outputs + ROWS - 1) / ROWS <= 65535;
}

// Y2_TRAIN_DENSE_KSPLIT=n forces the range count of forward and dinput (tests; clamped to the granules of the layer)
inline int forced_ranges(int forced)
{
    if (forced > 0) return forced;
    const char *ks = getenv("Y2_TRAIN_DENSE_KSPLIT");
    const int n = ks ? atoi(ks) : 0;
    return n > 0 ? n : 0;
}

}  // namespace

extern "C" {

/* Host arithmetic only (no GPU).  forward: one wave per (32 outputs, range), about two waves per SIMD of 256 CUs (2048)
 * with two steps of loads in flight each; a range keeps at least four 32-steps.  dinput: one workgroup per (128 inputs,
 * range), about two per CU (512); a range keeps at least two 64-chunks.  The partial sums are then a few per cent of the
 * weights' bytes at the shapes that matter (tiny-yolo-v1 at 32 rows: 8.5 MB and 9.6 MB beside 73.7 MB). */
int y2h_train_dense_plan(const y2h_train_dense *g, int product, int forced, int *ranges, size_t *ws_bytes, int *bounds, int max_bounds)
{
    if (!shape_ok(g) || (product != Y2H_DENSE_FORWARD && product != Y2H_DENSE_DINPUT)) return Y2H_EINVAL;
    const int fwd = product == Y2H_DENSE_FORWARD;
    const int total = fwd ? g->inputs : g->outputs, step = fwd ? KSTEP : OSTEP, cols = fwd ? g->outputs : g->inputs;
    const long passes = (g->batch + ROWS - 1) / ROWS;
    const long items = passes * (fwd ? (cols + ROWS - 1) / ROWS : (cols + 4 * ROWS - 1) / (4 * ROWS));
    const int steps = (total + step - 1) / step;
    long n = forced_ranges(forced);
    if (n <= 0) {
        n = ((fwd ? 2048 : 512) + items - 1) / items;
        if (n > steps / (fwd ? 4 : 2)) n = steps / (fwd ? 4 : 2);
    }
    if (n > steps) n = steps;
    if (n > 65535) n = 65535;
    if (n < 1) n = 1;
    if (ranges) *ranges = (int)n;
    if (ws_bytes) *ws_bytes = n > 1 ? (size_t)n * g->batch * cols * sizeof(float) : 0;
    for (int r = 0; bounds && r < n && r + 1 < max_bounds; ++r) range_of(total, step, (int)n, r, &bounds[r], &bounds[r + 1]);
    return Y2H_OK;
}

int y2h_train_dense_forward(const y2h_train_dense *g, const float *x, const float *w, float *y, float *ws, int forced, y2h_stream s)
{
    int n;
    size_t bytes;
    if (!x || !w || !y || y2h_train_dense_plan(g, Y2H_DENSE_FORWARD, forced, &n, &bytes, nullptr, 0) != Y2H_OK) return Y2H_EINVAL;
    if (bytes && !ws) return Y2H_EINVAL;
    Dense p = { x, nullptr, w, y, ws, g->batch, g->inputs, g->outputs, n, (g->outputs + ROWS - 1) / ROWS, 0 };
    const dim3 grid((unsigned)(((long)p.tiles * n + 3) / 4), (g->batch + ROWS - 1) / ROWS);
    if (g->inputs % 4 == 0 && (((uintptr_t)x | (uintptr_t)w) % 16) == 0) dense_forward<true><<<grid, 256, 0, S(s)>>>(p);
    else dense_forward<false><<<grid, 256, 0, S(s)>>>(p);
    Y2H_LAUNCH_CHECK();
    if (n > 1) {
        const long e = (long)g->batch * g->outputs;
        dense_finish<<<y2h_grid(e, 256), 256, 0, S(s)>>>(ws, y, e, n, 0);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}

int y2h_train_dense_dinput(const y2h_train_dense *g, const float *d, const float *w, float *dx, int add, float *ws, int forced, y2h_stream s)
{
    int n;
    size_t bytes;
    if (!d || !w || !dx || y2h_train_dense_plan(g, Y2H_DENSE_DINPUT, forced, &n, &bytes, nullptr, 0) != Y2H_OK) return Y2H_EINVAL;
    if (bytes && !ws) return Y2H_EINVAL;
    Dense p = { d, nullptr, w, dx, ws, g->batch, g->inputs, g->outputs, n, 0, add != 0 };
    dense_dinput<<<dim3((g->inputs + 4 * ROWS - 1) / (4 * ROWS), (g->batch + ROWS - 1) / ROWS, n), 256, 0, S(s)>>>(p);
    Y2H_LAUNCH_CHECK();
    if (n > 1) {
        const long e = (long)g->batch * g->inputs;
        dense_finish<<<y2h_grid(e, 256), 256, 0, S(s)>>>(ws, dx, e, n, add != 0);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}

int y2h_train_dense_dweight(const y2h_train_dense *g, const float *x, const float *d, float *dw, y2h_stream s)
{
    if (!x || !d || !dw || !shape_ok(g)) return Y2H_EINVAL;
    Dense p = { x, d, nullptr, dw, nullptr, g->batch, g->inputs, g->outputs, 1, 0, 1 };
    dense_dweight<<<dim3((g->inputs + 4 * ROWS - 1) / (4 * ROWS), (g->outputs + ROWS - 1) / ROWS), 256, 0, S(s)>>>(p);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

}  // extern "C"
