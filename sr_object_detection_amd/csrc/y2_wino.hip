// Winograd F(2x2,3x3) for the fp32 stride-1 3x3 convolutions: the two memory-bound passes around the batched GEMM
// (y2_conv.hip: y2h_conv_wino_forward; the rule: include/y2_wino_rule.h).
//
//     Y = A^T [ U .* V ] A,    U = G g G^T (at weight upload, y2_arena.c),    V = B^T d B
//
//         | 1  0 -1  0 |            | 1  1  1  0 |
//   B^T = | 0  1  1  0 |      A^T = | 0  1 -1 -1 |
//         | 0 -1  1  0 |
//         | 0  1  0 -1 |
//
// A tile t = (image, ty, tx) is the 2x2 output patch at (2 ty, 2 tx) and reads the 4x4 input patch at (2 ty - 1, 2 tx - 1);
// with the fused 2x2/2 maxpool it is exactly one pooling window.  B^T and A^T only add and subtract: on integer data both
// passes are exact.
//
//  * wino_input_kernel  -- V[g][t][c] from the NHWC input: a thread owns four channels of one tile (sixteen 16-byte loads,
//    consecutive threads consecutive channels; padding taps and the row / column behind an odd edge read as zero), transforms
//    them in registers and writes its sixteen components.  The four tiles that share a pixel are neighbours in t, so the
//    pixel comes from HBM once and from the caches otherwise.  Tiles tiles .. tiles_pad - 1 (the GEMM's row padding) are zero.
//
//  * wino_output_kernel -- a thread owns four filters of one tile: sixteen 16-byte loads of M[g][t][n], A^T M A, then the
//    shared epilogue() on each of the four outputs -- or, with the fused pool, pool_pick over the four and ONE epilogue, the
//    direct kernel's rule (negative batch-norm scales pick the minimum).  Honours ldy (route targets) and odd H / W.
//
// Compiled with -ffp-contract=off like y2_conv.hip: the epilogue mirrors the reference step by step.
#include "y2_conv_shared.hpp"
#include "y2_split_rule.h"

struct WinoK {
    const float *x;
    float *V;
    const float *M;
    float *y;
    const float *mean;
    const double *rinv;
    const float *scale;
    const float *bias;
    int H, W, C, ldx, N, ldy;
    int th, tw;                // tiles per image column / row: ceil(H/2), ceil(W/2)
    long tiles, tiles_pad;
    int pool, bn, act;
    int vec;                   // 16-byte output stores are possible (ldy and y aligned)
};

__global__ __launch_bounds__(256) void wino_input_kernel(WinoK a)
{
    const int c4n = a.C >> 2;
    const long total = a.tiles_pad * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long t = idx / c4n;
        const int c = (int)(idx - t * c4n) * 4;
        f32x4 d[4][4];
        if (t < a.tiles) {
            const int tx = (int)(t % a.tw);
            const long q = t / a.tw;
            const int ty = (int)(q % a.th), n = (int)(q / a.th);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = 2 * ty - 1 + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = 2 * tx - 1 + j;
                    const bool ok = y >= 0 && y < a.H && x >= 0 && x < a.W;
                    d[i][j] = ok ? *(const f32x4 *)&a.x[((size_t)(n * a.H + y) * a.W + x) * a.ldx + c] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        f32x4 r[4][4];          // B^T d
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[0][j] = d[0][j] - d[2][j];
            r[1][j] = d[1][j] + d[2][j];
            r[2][j] = d[2][j] - d[1][j];
            r[3][j] = d[1][j] - d[3][j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v0 = r[i][0] - r[i][2], v1 = r[i][1] + r[i][2], v2 = r[i][2] - r[i][1], v3 = r[i][1] - r[i][3];
            float *dst = a.V + ((size_t)(i * 4) * a.tiles_pad + t) * a.C + c;
            const size_t comp = (size_t)a.tiles_pad * a.C;
            *(f32x4 *)&dst[0] = v0;
            *(f32x4 *)&dst[comp] = v1;
            *(f32x4 *)&dst[2 * comp] = v2;
            *(f32x4 *)&dst[3 * comp] = v3;
        }
    }
}

// The same pass for the split GEMM (y2_wino_split.hip): every component leaves as three bf16 planes h, m, l with
// h + m + l == v (y2_split3 of include/y2_split_rule.h restated: v_cvt_pk_bf16_f32 and two exact subtractions), in the
// operand layout of y2_split_index.  A thread still owns four channels of one tile; a wave takes the 16 channels of one
// K-tile for 16 consecutive tiles, so that per component, plane and k-half it writes one run of 256 bytes and the four waves
// of a block read 64 consecutive channels of each pixel.  Rows tiles .. tiles_pad - 1 are zero in all three planes.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 bf16x4_f32(u16x4 b)
{
    const u32x4 u = __builtin_convertvector(b, u32x4) << 16;
    return __builtin_bit_cast(f32x4, u);
}

__device__ __forceinline__ void split3_x4(const f32x4 v, u16x4 &h, u16x4 &m, u16x4 &l)
{
    const u32x4 bits = __builtin_bit_cast(u32x4, v);
    h = __builtin_bit_cast(u16x4, __builtin_convertvector(v, bf16x4));
    bool fin[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned mag = bits[k] & 0x7fffffffu;
        fin[k] = mag < 0x7f800000u;
        if (fin[k] && mag >= 0x7f7f8000u) h[k] = (unsigned short)(((bits[k] >> 16) & 0x8000u) | 0x7f7fu);      // never round a finite value to an infinity
    }
    f32x4 r = v - bf16x4_f32(h);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (!fin[k]) r[k] = 0.f;
    m = __builtin_bit_cast(u16x4, __builtin_convertvector(r, bf16x4));
    r = r - bf16x4_f32(m);
    l = __builtin_bit_cast(u16x4, __builtin_convertvector(r, bf16x4));    // exact: the low 16 bits are zero (but for bits below 2^-133)
}

__global__ __launch_bounds__(256) void wino_input_split_kernel(WinoK a, unsigned short *Vs)
{
    const int nk = a.C / Y2_SPLIT_BK;
    const long total = a.tiles_pad * (a.C >> 2);
    const size_t rb = (size_t)(a.tiles_pad / Y2_SPLIT_ROWS);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int cq = (int)(idx & 3), tl = (int)((idx >> 2) & 15);
        const long rest = idx >> 6;
        const int kt = (int)(rest % nk);
        const long t = (rest / nk) * 16 + tl;
        const int c = kt * Y2_SPLIT_BK + cq * 4;
        f32x4 d[4][4];
        if (t < a.tiles) {
            const int tx = (int)(t % a.tw);
            const long q = t / a.tw;
            const int ty = (int)(q % a.th), n = (int)(q / a.th);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = 2 * ty - 1 + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = 2 * tx - 1 + j;
                    const bool ok = y >= 0 && y < a.H && x >= 0 && x < a.W;
                    d[i][j] = ok ? *(const f32x4 *)&a.x[((size_t)(n * a.H + y) * a.W + x) * a.ldx + c] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        f32x4 r[4][4];          // B^T d
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[0][j] = d[0][j] - d[2][j];
            r[1][j] = d[1][j] + d[2][j];
            r[2][j] = d[2][j] - d[1][j];
            r[3][j] = d[1][j] - d[3][j];
        }
        // y2_split_index(tiles_pad, C, g, t, c, p) = first + g * comp + p * plane
        const size_t first = ((size_t)(t / Y2_SPLIT_ROWS) * nk + kt) * Y2_SPLIT_BLOCK_ELEMS + ((size_t)(cq >> 1) * Y2_SPLIT_ROWS + (size_t)(t % Y2_SPLIT_ROWS)) * 8 + (size_t)(cq & 1) * 4;
        const size_t comp = rb * nk * Y2_SPLIT_BLOCK_ELEMS, plane = (size_t)2 * Y2_SPLIT_ROWS * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v[4] = {r[i][0] - r[i][2], r[i][1] + r[i][2], r[i][2] - r[i][1], r[i][1] - r[i][3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u16x4 h, m, l;
                split3_x4(v[j], h, m, l);
                unsigned short *dst = Vs + first + (size_t)(i * 4 + j) * comp;
                *(u16x4 *)&dst[0] = h;
                *(u16x4 *)&dst[plane] = m;
                *(u16x4 *)&dst[2 * plane] = l;
            }
        }
    }
}

__global__ __launch_bounds__(256) void wino_output_kernel(WinoK a)
{
    const int n4n = a.N >> 2;
    const long total = a.tiles * n4n;
    const size_t comp = (size_t)a.tiles_pad * a.N;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long t = idx / n4n;
        const int co = (int)(idx - t * n4n) * 4;
        const float *src = a.M + (size_t)t * a.N + co;
        f32x4 m[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) m[i][j] = *(const f32x4 *)&src[(size_t)(i * 4 + j) * comp];
        f32x4 s[2][4];          // A^T M
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[0][j] = (m[0][j] + m[1][j]) + m[2][j];
            s[1][j] = (m[1][j] - m[2][j]) - m[3][j];
        }
        f32x4 o[2][2];          // (A^T M) A: the patch's outputs (row, column)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            o[i][0] = (s[i][0] + s[i][1]) + s[i][2];
            o[i][1] = (s[i][1] - s[i][2]) - s[i][3];
        }
        float mean[4] = {0.f, 0.f, 0.f, 0.f}, scale[4] = {1.f, 1.f, 1.f, 1.f}, bias[4];
        double rinv[4] = {1.0, 1.0, 1.0, 1.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bias[k] = a.bias[co + k];
            if (a.bn) { mean[k] = a.mean[co + k]; rinv[k] = a.rinv[co + k]; scale[k] = a.scale[co + k]; }
        }
        if (a.pool) {
            // the tile is the pooling window: output pixel t of the [batch][H/2][W/2] map
            f32x4 out;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                out[k] = epilogue(pool_pick(o[0][0][k], o[0][1][k], o[1][0][k], o[1][1][k], !a.bn || scale[k] >= 0.f), a.bn, mean[k], rinv[k],
                                  scale[k], bias[k], a.act);
            float *dst = a.y + (size_t)t * a.ldy + co;
            if (a.vec) *(f32x4 *)dst = out;
            else { dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3]; }
            continue;
        }
        const int tx = (int)(t % a.tw);
        const long q = t / a.tw;
        const int ty = (int)(q % a.th), n = (int)(q / a.th);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = 2 * ty + i, x = 2 * tx + j;
                if (y >= a.H || x >= a.W) continue;            // the row / column behind an odd edge
                f32x4 out;
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = epilogue(o[i][j][k], a.bn, mean[k], rinv[k], scale[k], bias[k], a.act);
                float *dst = a.y + ((size_t)(n * a.H + y) * a.W + x) * a.ldy + co;
                if (a.vec) *(f32x4 *)dst = out;
                else { dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3]; }
            }
    }
}

static void wino_args(const y2h_conv *d, long tiles, long tiles_pad, WinoK &a)
{
    memset(&a, 0, sizeof a);
    a.x = d->x; a.y = d->y;
    a.mean = d->mean; a.rinv = d->rinv; a.scale = d->scale; a.bias = d->bias;
    a.H = d->h; a.W = d->w; a.C = d->c; a.ldx = d->ldx; a.N = d->n; a.ldy = d->ldy;
    a.th = (d->h + 1) / 2; a.tw = (d->w + 1) / 2;
    a.tiles = tiles; a.tiles_pad = tiles_pad;
    a.pool = d->fuse_maxpool2 ? 1 : 0;
    a.bn = d->batch_normalize; a.act = d->activation;
    a.vec = d->ldy % 4 == 0 && ((uintptr_t)d->y % 16) == 0;
}

int y2_wino_input_launch(const y2h_conv *d, float *V, long tiles, long tiles_pad, y2h_stream s)
{
    if (!V || d->c % 4 != 0 || d->ldx % 4 != 0 || ((uintptr_t)d->x | (uintptr_t)V) % 16 != 0) return Y2H_EINVAL;
    if (tiles != y2_wino_tiles(d->batch, d->h, d->w) || tiles_pad < tiles) return Y2H_EINVAL;
    WinoK a;
    wino_args(d, tiles, tiles_pad, a);
    a.V = V;
    hipLaunchKernelGGL(wino_input_kernel, dim3(y2h_grid(tiles_pad * (d->c / 4), 256, 256 * 32)), dim3(256), 0, S(s), a);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2_wino_input_split_launch(const y2h_conv *d, unsigned short *V, long tiles, long tiles_pad, y2h_stream s)
{
    if (!V || d->c % Y2_SPLIT_BK != 0 || d->ldx % 4 != 0 || ((uintptr_t)d->x | (uintptr_t)V) % 16 != 0) return Y2H_EINVAL;
    if (tiles != y2_wino_tiles(d->batch, d->h, d->w) || tiles_pad < tiles || tiles_pad % Y2_SPLIT_ROWS != 0) return Y2H_EINVAL;
    WinoK a;
    wino_args(d, tiles, tiles_pad, a);
    hipLaunchKernelGGL(wino_input_split_kernel, dim3(y2h_grid(tiles_pad * (d->c / 4), 256, 256 * 32)), dim3(256), 0, S(s), a, V);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

int y2_wino_output_launch(const y2h_conv *d, const float *M, long tiles, long tiles_pad, y2h_stream s)
{
    if (!M || d->n % 4 != 0 || ((uintptr_t)M % 16) != 0) return Y2H_EINVAL;
    if (tiles != y2_wino_tiles(d->batch, d->h, d->w) || tiles_pad < tiles) return Y2H_EINVAL;
    if (d->fuse_maxpool2 && ((d->h | d->w) & 1)) return Y2H_EINVAL;
    WinoK a;
    wino_args(d, tiles, tiles_pad, a);
    a.M = M;
    hipLaunchKernelGGL(wino_output_kernel, dim3(y2h_grid(tiles * (d->n / 4), 256, 256 * 32)), dim3(256), 0, S(s), a);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
