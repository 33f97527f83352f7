// fp16 storage mode for the dense heads (engine extension; the reference is fp32 only): [connected] and [crop] with half
// weights and half activations, fp32 accumulation ([local] in half is local_kernel<_Float16, ...> of y2_layers.hip).  At
// the batches these heads run at they are weight streams (vgg-16's first dense layer: 25088 x 4096, yolov1/yolo.cfg's
// [local]: 49 x 256 x 9216), so half storage halves the bytes that bound them.
//
// connected_f16: y[r][n] = act((sum_k x[r][k] * w[n][k]) * alpha[n] + beta[n]) for up to 16 rows per pass on
// v_mfma_f32_16x16x32_f16.  The A fragment is 16 rows of x (rows past the batch are zero), the B fragment 16 weight rows:
// lane l holds A[row l&15][k = 8*(l>>4) + j] and B[k][col l&15], j = 0..7, so a lane's operand is one 16-byte load from
// its own row.  The order of k inside the sum is free as long as A and B agree, so the main loop takes 64 k per trip and
// lane group g = l>>4 reads halves [16g, 16g + 16) of them -- 32 contiguous bytes per lane, whole 128-byte lines per
// weight row -- and feeds two MFMAs.  No LDS: the operands go straight to registers, x is small and stays in L2.
// A work item is (16-column tile, K range), one wave each; with more than one range the items write raw fp32 partial sums
// to the caller's workspace [range][16][roundup(outputs, 16)] and a second launch adds them in ascending K order.  Both
// ends go through dense_finish, which is the convolution tiles' epilogue_fast: no atomics, the result depends on neither
// timing nor grid.
#include "y2_conv_shared.hpp"
#include <stdint.h>

// K range r of `ranges` over the 32-steps of `inputs`: whole steps, dealt as evenly as integers allow; the last range
// also takes the tail shorter than a step
__host__ __device__ static inline void dense_range(int inputs, int ranges, int r, int *k0, int *k1)
{
    const long steps = (inputs + 31) / 32;
    *k0 = (int)(r * steps / ranges) * 32;
    *k1 = (r + 1 == ranges) ? inputs : (int)((r + 1) * steps / ranges) * 32;
}

// Host arithmetic only (no GPU).  The number of K ranges: one wave streams one (tile, range), and about eight waves per CU
// on 256 CUs keep enough loads in flight to stream from HBM; a range keeps at least eight steps (16 rows x 512 bytes), so
// that the partial sums stay small beside the weights.  forced > 0 sets the count, clamped to the number of steps.
extern "C" int y2h_connected_f16_plan(int rows, int inputs, int outputs, int forced, int *ranges, size_t *ws_bytes, int *bounds,
                                      int max_bounds)
{
    if (rows <= 0 || inputs <= 0 || outputs <= 0) return Y2H_EINVAL;
    const int steps = (inputs + 31) / 32, tiles = (outputs + 15) / 16;
    int n = forced;
    if (n <= 0) {
        n = (2048 + tiles - 1) / tiles;
        if (n > steps / 8) n = steps / 8;
    }
    if (n > steps) n = steps;
    if (n < 1) n = 1;
    if (ranges) *ranges = n;
    if (ws_bytes) *ws_bytes = n > 1 ? (size_t)n * 16 * ((size_t)tiles * 16) * sizeof(float) : 0;
    for (int r = 0; bounds && r < n && r + 1 < max_bounds; ++r) dense_range(inputs, n, r, &bounds[r], &bounds[r + 1]);
    return Y2H_OK;
}

struct DenseK {
    const _Float16 *x; long ldx;    // [rows][ldx]
    const _Float16 *w;              // [outputs][inputs]
    const float *alpha, *beta;
    void *y; int ldy, y_f16;
    int rows, inputs, outputs, act;
    int ranges, tiles, npad;
    float *ws;                      // [ranges][16][npad] raw sums when ranges > 1
};

// the one epilogue of a dense value, whichever launch finishes it
__device__ __forceinline__ void dense_finish(const DenseK &a, int row, int n, float sum)
{
    const float v = epilogue_fast(sum, a.alpha[n], a.beta[n], a.act);
    if (a.y_f16) ((_Float16 *)a.y)[(size_t)row * a.ldy + n] = (_Float16)v;
    else ((float *)a.y)[(size_t)row * a.ldy + n] = v;
}

// VEC: inputs % 8 == 0 and 16-byte aligned views, 16-byte loads; otherwise the same walk with scalar loads
template <bool VEC>
__global__ __launch_bounds__(256) void connected_f16_kernel(DenseK a)
{
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)a.tiles * a.ranges) return;
    const int tile = (int)(item % a.tiles), r = (int)(item / a.tiles);
    const int n = tile * 16 + i;
    int k0, k1;
    dense_range(a.inputs, a.ranges, r, &k0, &k1);
    // a column past the last output reads the last row (in bounds) and is never stored
    const _Float16 *wr = a.w + (size_t)(n < a.outputs ? n : a.outputs - 1) * a.inputs;
    const bool rowok = i < a.rows;
    const _Float16 *xr = a.x + (size_t)(rowok ? i : 0) * a.ldx;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = k0;
    if constexpr (VEC) {
        // 256 k per trip: all sixteen loads are issued before the first MFMA waits for one (a row past the batch reads row 0
        // and is zeroed by a select, so that no load sits behind a branch)
        for (; k + 256 <= k1; k += 256) {
            f16x8 bf[8], af[8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f16x8 *wp = (const f16x8 *)(wr + k + 64 * u + 16 * g), *xp = (const f16x8 *)(xr + k + 64 * u + 16 * g);
                bf[2 * u] = wp[0]; bf[2 * u + 1] = wp[1];
                af[2 * u] = xp[0]; af[2 * u + 1] = xp[1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(rowok ? af[u] : zero, bf[u], acc, 0, 0, 0);
        }
        for (; k + 64 <= k1; k += 64) {
            const f16x8 *wp = (const f16x8 *)(wr + k + 16 * g), *xp = (const f16x8 *)(xr + k + 16 * g);
            const f16x8 b0 = wp[0], b1 = wp[1], a0 = xp[0], a1 = xp[1];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(rowok ? a0 : zero, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(rowok ? a1 : zero, b1, acc, 0, 0, 0);
        }
    }
    // what is left of the range, a step at a time: fragments past k1 are zero
    for (; k < k1; k += 32) {
        const int kk = k + 8 * g;
        f16x8 av = zero, bv = zero;
        if constexpr (VEC) {                      // k1 is a multiple of 8: a fragment is inside or outside as a whole
            if (kk + 8 <= k1) {
                bv = *(const f16x8 *)(wr + kk);
                av = *(const f16x8 *)(xr + kk);
                av = rowok ? av : zero;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (kk + j < k1) { bv[j] = wr[kk + j]; if (rowok) av[j] = xr[kk + j]; }
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc, 0, 0, 0);
    }
    if (n >= a.outputs) return;
    // the lane holds C[row 4g + j][col i]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * g + j;
        if (row >= a.rows) continue;
        if (a.ranges == 1) dense_finish(a, row, n, acc[j]);
        else a.ws[((size_t)r * 16 + row) * a.npad + n] = acc[j];
    }
}

__global__ __launch_bounds__(256) void connected_f16_sum_kernel(DenseK a)
{
    const long total = (long)a.rows * a.outputs;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int n = (int)(idx % a.outputs), row = (int)(idx / a.outputs);
        float sum = a.ws[(size_t)row * a.npad + n];
        for (int r = 1; r < a.ranges; ++r) sum = sum + a.ws[((size_t)r * 16 + row) * a.npad + n];
        dense_finish(a, row, n, sum);
    }
}

// x: half [rows][ldx]; w: half [outputs][inputs]; y: [rows][ldy] fp32 or half (y_f16).  `ranges` as y2h_connected_f16_plan
// gives it (ws: that many bytes when > 1).  More than 16 rows run in passes of 16 that share ws in stream order.
extern "C" int y2h_connected_f16(const void *x, long ldx, const void *w, const float *alpha, const float *beta, void *y, int ldy,
                                 int y_f16, int rows, int inputs, int outputs, int activation, int ranges, float *ws,
                                 size_t ws_bytes, y2h_stream s)
{
    if (!x || !w || !alpha || !beta || !y || rows <= 0 || inputs <= 0 || outputs <= 0 || ldx < inputs || ldy < outputs) return Y2H_EINVAL;
    if (activation < Y2H_ACT_LINEAR || activation > Y2H_ACT_RELU) return Y2H_EINVAL;
    if (ranges < 1 || ranges > (inputs + 31) / 32) return Y2H_EINVAL;
    DenseK a;
    memset(&a, 0, sizeof a);
    a.w = (const _Float16 *)w; a.alpha = alpha; a.beta = beta; a.ldx = ldx; a.ldy = ldy; a.y_f16 = y_f16;
    a.inputs = inputs; a.outputs = outputs; a.act = activation; a.ranges = ranges;
    a.tiles = (outputs + 15) / 16; a.npad = a.tiles * 16; a.ws = ws;
    if (ranges > 1 && (!ws || ws_bytes < (size_t)ranges * 16 * a.npad * sizeof(float))) return Y2H_EINVAL;
    const bool vec = inputs % 8 == 0 && ldx % 8 == 0 && (((uintptr_t)x | (uintptr_t)w) % 16) == 0;
    const long items = (long)a.tiles * ranges;
    for (int r0 = 0; r0 < rows; r0 += 16) {
        a.rows = rows - r0 < 16 ? rows - r0 : 16;
        a.x = (const _Float16 *)x + (size_t)r0 * ldx;
        a.y = y_f16 ? (void *)((_Float16 *)y + (size_t)r0 * ldy) : (void *)((float *)y + (size_t)r0 * ldy);
        if (vec) hipLaunchKernelGGL(connected_f16_kernel<true>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, S(s), a);
        else hipLaunchKernelGGL(connected_f16_kernel<false>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, S(s), a);
        Y2H_LAUNCH_CHECK();
        if (ranges > 1) {
            hipLaunchKernelGGL(connected_f16_sum_kernel, dim3(y2h_grid((long)a.rows * outputs, 256)), dim3(256), 0, S(s), a);
            Y2H_LAUNCH_CHECK();
        }
    }
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// crop_f16: crop_kernel (y2_layers.hip) writing half.  x*scale + trans is evaluated in fp32 as there and rounded to half
// once.  One thread per output pixel writes its channels to the plain NHWC output and, with y4 set (c <= 4), the pixel
// {v0, v1, v2, v3 or 0} to the interior of the [batch][oh+2][ow+2][4] form the fp16 first-layer kernel reads (the caller
// zeroes that buffer once: the halo and the unused channels stay zero).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crop_f16_kernel(const float *__restrict__ x, int ldx, _Float16 *__restrict__ y, int ldy,
                                                       _Float16 *__restrict__ y4, int h, int w, int c, int oh, int ow, int dh, int dw,
                                                       float scale, float trans, long total)
{
    for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < total; pix += (long)gridDim.x * 256) {
        const int ox = (int)(pix % ow);
        const int oy = (int)((pix / ow) % oh);
        const long b = pix / ((long)ow * oh);
        const float *src = x + ((b * h + oy + dh) * w + ox + dw) * ldx;
        f16x4 px = {0, 0, 0, 0};
        for (int k = 0; k < c; ++k) {
            const _Float16 v = (_Float16)(src[k] * scale + trans);
            y[pix * ldy + k] = v;
            if (k < 4) px[k] = v;
        }
        if (y4) *(f16x4 *)&y4[((b * (oh + 2) + oy + 1) * (long)(ow + 2) + ox + 1) * 4] = px;
    }
}

extern "C" int y2h_crop_f16(const float *x, int ldx, void *y, int ldy, void *y4, int batch, int h, int w, int c, int out_h, int out_w,
                            int noadjust, y2h_stream s)
{
    if (!x || !y || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || out_h <= 0 || out_w <= 0 || out_h > h || out_w > w) return Y2H_EINVAL;
    if (ldx < c || ldy < c || (y4 && (c > 4 || ((uintptr_t)y4 % 8) != 0))) return Y2H_EINVAL;
    const long total = (long)batch * out_h * out_w;
    hipLaunchKernelGGL(crop_f16_kernel, dim3(y2h_grid(total, 256)), dim3(256), 0, S(s), x, ldx, (_Float16 *)y, ldy, (_Float16 *)y4,
                       h, w, c, out_h, out_w, (h - out_h) / 2, (w - out_w) / 2, noadjust ? 1.f : 2.f, noadjust ? 0.f : -1.f, total);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
