// [normalization] (cross-channel local response normalization, normalization_layer.c:65-94) and the stand-alone
// [activation] layer (activation_layer.c:39-43), NHWC.  Compiled with -ffp-contract=off.
//
// The reference builds norms[k] channel by channel: norms[0] = kappa + alpha*sq[0..size/2-1], then norms[k] = norms[k-1]
// - alpha*sq[k-(size-1)/2-1] + alpha*sq[k+size/2].  Channel size/2 is therefore never added, but it is subtracted once it
// leaves the window, so for every k
//     norms[k] = kappa + alpha * (sum_{j in W_k} sq[j] - sq[size/2]),   W_k = [k-(size-1)/2, k+size/2] within [0, c-1]
// (sq[j] = 0 for j >= c).  out = norms^-beta * x; a norm <= 0 gives NaN there and here.
//
//   lrn_ref_kernel   strict mode: one lane per pixel walks the channels in the reference's order, product and sum rounded
//                    separately, pow in double -- bit-identical to the reference.
//   lrn_kernel       the closed form in one pass.  A workgroup takes a tile of pixels; a lane owns four consecutive
//                    channels of one pixel: it loads them once (16 bytes where the layout allows), keeps them in registers,
//                    puts their squares into the pixel's LDS row, and after the barrier sums each of its four windows in
//                    ascending channel order from LDS.  The row has a zero border on both sides, so no window tests its
//                    bounds.  A value depends on its own pixel only: the same at any batch size, tile and run.
//                    norm^-beta is v_exp_f32(-beta * v_log_f32(norm)).  Those instructions flush denormals, so a positive
//                    denormal norm gives inf where the reference is finite, and with beta == 0 a norm of exactly 0 gives
//                    NaN (-0 * -inf) where pow gives 1; no norm is denormal or zero with kappa near its default of 1, and
//                    strict mode (pow in double) covers a network that needs those cases.
#include "y2_common.hpp"
#include <stdint.h>

#define LRN_NT 256          // lanes per workgroup

// Lanes of one pixel read LDS words 4 apart: on the 32 banks of ds_read_b32 that would be a 4-way conflict.  One pad word per
// 32 moves each run of 8 lanes to the next bank, so the 32 lanes of a half wave hit 32 banks.
__device__ __forceinline__ int lrn_pos(int i) { return i + (i >> 5); }
static inline int lrn_pos_host(int i) { return i + (i >> 5); }

template <typename T> struct lrn_vec;
template <> struct lrn_vec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct lrn_vec<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(4))); };

// halo: zero words in front of channel 0 (a multiple of 4, >= size); rowlen: padded words per pixel row, odd.
// tile_px * ceil(c/4) <= LRN_NT: every lane owns at most one group of four channels of one pixel of the tile.
template <typename T, bool VEC>
__global__ __launch_bounds__(LRN_NT) void lrn_kernel(const T *__restrict__ x, int ldx, T *__restrict__ y, int ldy, long pixels, int c,
                                                     int size, float alpha, float beta, float kappa, int tile_px, int halo, int rowlen)
{
    extern __shared__ float sq[];
    typedef typename lrn_vec<T>::type vec4;
    const int t = threadIdx.x;
    const int cg = (c + 3) >> 2;                    // four-channel groups per pixel
    const int lo = (size - 1) / 2, q = size / 2;
    const int px = t / cg, k = (t - px * cg) * 4;   // this lane's pixel of the tile and first channel
    float *row = sq + px * rowlen;
    for (int i = t; i < tile_px * rowlen; i += LRN_NT) sq[i] = 0.f;
    __syncthreads();
    const long tiles = (pixels + tile_px - 1) / tile_px;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long p = tile * tile_px + px;
        const bool live = px < tile_px && p < pixels;
        float xv[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const T *src = x + p * ldx + k;
            if (VEC) {
                const vec4 v = *(const vec4 *)src;
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = (float)v[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < c) xv[j] = (float)src[j];
            }
        }
        if (px < tile_px) {
#pragma unroll
            for (int j = 0; j < 4; ++j) row[lrn_pos(halo + k + j)] = xv[j] * xv[j];
        }
        __syncthreads();
        if (live) {
            const float gone = row[lrn_pos(halo + q)];
            // window words k-lo .. k+3+size/2 once, each added to the sums whose window holds it: ascending order per sum
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            const int first = halo + k - lo;
            for (int i = 0; i < size + 3; ++i) {
                const float v = row[lrn_pos(first + i)];
                if (i < size) s0 += v;
                if (i >= 1 && i < size + 1) s1 += v;
                if (i >= 2 && i < size + 2) s2 += v;
                if (i >= 3) s3 += v;
            }
            const float s[4] = {s0, s1, s2, s3};
            float r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = s[j] - gone;
                const float norm = kappa + alpha * d;
                // v_exp_f32(-beta * v_log_f32(norm)), about 1 ulp each: NaN for norm < 0, inf * x for norm = 0
                r[j] = __builtin_amdgcn_exp2f(-beta * __builtin_amdgcn_logf(norm)) * xv[j];
            }
            T *dst = y + p * ldy + k;
            if (VEC) {
                vec4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (T)r[j];
                *(vec4 *)dst = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (k + j < c) dst[j] = (T)r[j];
            }
        }
        __syncthreads();                            // the next tile overwrites the rows
    }
}

__global__ __launch_bounds__(256) void lrn_ref_kernel(const float *__restrict__ x, int ldx, float *__restrict__ y, int ldy, long pixels,
                                                      int c, int size, float alpha, float beta, float kappa)
{
    const float nalpha = -alpha;
    const double nbeta = (double)(-beta);
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long)gridDim.x * 256) {
        const float *in = x + p * ldx;
        float *out = y + p * ldy;
        float norm = kappa;
        for (int k = 0; k < size / 2; ++k) { const float v = in[k], t = alpha * (v * v); norm = norm + t; }
        out[0] = (float)pow((double)norm, nbeta) * in[0];
        for (int k = 1; k < c; ++k) {
            const int prev = k - (size - 1) / 2 - 1, next = k + size / 2;
            if (prev >= 0) { const float v = in[prev], t = nalpha * (v * v); norm = norm + t; }
            if (next < c) { const float v = in[next], t = alpha * (v * v); norm = norm + t; }
            out[k] = (float)pow((double)norm, nbeta) * in[k];
        }
    }
}

// pixels per tile and the row geometry of the one-pass form; 0 when one pixel's row does not fit a workgroup (more than
// 4 * LRN_NT = 1024 channels, or a window that pushes the row past 48 KB): the reference-order kernel runs then
static int lrn_tile(int c, int size, int *halo, int *rowlen)
{
    const int cg = (c + 3) / 4;
    if (cg > LRN_NT) return 0;
    *halo = (size + 3) / 4 * 4;
    *rowlen = lrn_pos_host(*halo + cg * 4 + size - 1) + 1;
    *rowlen |= 1;                                   // rows of neighbouring pixels start on different banks
    if ((size_t)*rowlen * sizeof(float) > 48 * 1024) return 0;
    return LRN_NT / cg;
}

template <typename T>
static int lrn_launch(const T *x, int ldx, T *y, int ldy, long pixels, int c, int size, float alpha, float beta, float kappa,
                      int align, y2h_stream s)
{
    int halo = 0, rowlen = 0;
    const int tile_px = lrn_tile(c, size, &halo, &rowlen);
    if (tile_px <= 0) return Y2H_EINVAL;
    const bool vec = (c % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) % align == 0);
    const long tiles = (pixels + tile_px - 1) / tile_px;
    const size_t lds = (size_t)tile_px * rowlen * sizeof(float);
    const dim3 grid(y2h_grid(tiles, 1, 256 * 8));
    void (*fn)(const T *, int, T *, int, long, int, int, float, float, float, int, int, int) = vec ? lrn_kernel<T, true> : lrn_kernel<T, false>;
    hipLaunchKernelGGL(fn, grid, dim3(LRN_NT), lds, S(s), x, ldx, y, ldy, pixels, c, size, alpha, beta, kappa, tile_px, halo, rowlen);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

static bool lrn_args_ok(const void *x, int ldx, const void *y, int ldy, long pixels, int c, int size)
{
    return x && y && pixels > 0 && c > 0 && size >= 1 && size / 2 <= c && ldx >= c && ldy >= c;
}

extern "C" int y2h_lrn_fast_ok(int c, int size)
{
    int halo, rowlen;
    return c > 0 && size >= 1 && lrn_tile(c, size, &halo, &rowlen) > 0;
}

extern "C" int y2h_lrn(const float *x, int ldx, float *y, int ldy, long pixels, int c, int size, float alpha, float beta, float kappa,
                       int strict, y2h_stream s)
{
    if (!lrn_args_ok(x, ldx, y, ldy, pixels, c, size)) return Y2H_EINVAL;
    if (!strict && y2h_lrn_fast_ok(c, size)) return lrn_launch<float>(x, ldx, y, ldy, pixels, c, size, alpha, beta, kappa, 16, s);
    hipLaunchKernelGGL(lrn_ref_kernel, dim3(y2h_grid(pixels, 256)), dim3(256), 0, S(s), x, ldx, y, ldy, pixels, c, size, alpha, beta, kappa);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_lrn_f16(const void *x, int ldx, void *y, int ldy, long pixels, int c, int size, float alpha, float beta, float kappa,
                           y2h_stream s)
{
    if (!lrn_args_ok(x, ldx, y, ldy, pixels, c, size) || !y2h_lrn_fast_ok(c, size)) return Y2H_EINVAL;
    return lrn_launch<_Float16>((const _Float16 *)x, ldx, (_Float16 *)y, ldy, pixels, c, size, alpha, beta, kappa, 8, s);
}

// ---------------------------------------------------------------------------
// [activation]: y[row][k] = act(x[row][k]), out of place, the formulas of y2h_activate_array (activate_any)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void activate_copy_kernel(const T *__restrict__ x, int ldx, T *__restrict__ y, int ldy, int c, int act,
                                                            long total)
{
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long row = idx / c;
        const int k = (int)(idx - row * c);
        y[row * ldy + k] = (T)activate_any((float)x[row * ldx + k], act);
    }
}

extern "C" int y2h_activate_copy(const float *x, int ldx, float *y, int ldy, long rows, int c, int activation, y2h_stream s)
{
    if (!x || !y || rows <= 0 || c <= 0 || ldx < c || ldy < c || activation < 0 || activation > Y2H_ACT_LHTAN) return Y2H_EINVAL;
    const long total = rows * c;
    hipLaunchKernelGGL(activate_copy_kernel<float>, dim3(y2h_grid(total, 256)), dim3(256), 0, S(s), x, ldx, y, ldy, c, activation, total);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// half in, half out, the function in fp32; the four activations the half convolutions apply (Y2H_ACT_LINEAR .. _RELU)
extern "C" int y2h_activate_copy_f16(const void *x, int ldx, void *y, int ldy, long rows, int c, int activation, y2h_stream s)
{
    if (!x || !y || rows <= 0 || c <= 0 || ldx < c || ldy < c || activation < 0 || activation > Y2H_ACT_RELU) return Y2H_EINVAL;
    const long total = rows * c;
    hipLaunchKernelGGL(activate_copy_kernel<_Float16>, dim3(y2h_grid(total, 256)), dim3(256), 0, S(s), (const _Float16 *)x, ldx,
                       (_Float16 *)y, ldy, c, activation, total);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
