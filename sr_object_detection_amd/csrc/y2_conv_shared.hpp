// Shared between the fp32 (y2_conv.hip) and fp16 (y2_conv_f16.hip) convolution kernels.
#pragma once
#include "y2_common.hpp"
#include "y2_streamk_rule.h"
#include "y2_wino_rule.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct ConvK {
    const float *x;    // fp16 kernels: const _Float16 *
    const float *w;
    float *y;          // y_f16: _Float16 *
    const float *mean;
    const double *rinv;
    const float *scale;
    const float *bias;
    const float *alpha, *beta;   // fp16 path: y = act(acc * alpha[co] + beta[co])
    int y_f16;         // 1: the output is stored as IEEE half
    int vec_store;     // fp16 kernels: half outputs leave as 16-byte stores (ldy, y and Cout aligned to 8 halves)
    int nchw;          // first-layer kernel: x is the fp32 NCHW network input (no halo, no NHWC copy)
    int dbg;           // ablation switches for tuning runs (env Y2_DBG; 0 in normal use): see y2_conv_f16.hip
    int H, W, Cin, ldx, Cout, ldy, K;
    int npix;          // GEMM rows = output pixels: batch * out_h * out_w (== batch * H * W at stride 1)
    int pool;          // 1: a 2x2 stride-2 maxpool is fused behind the activation (see pool_pixel)
    int bn, act;
    unsigned xbytes, wbytes;
    unsigned ybytes;   // fp32 8-wave tiles with vec_store: byte size of the output buffer from a.y on (buffer stores)
    int tiles_n;
    int ntiles;        // tiles_m * tiles_n * ksplit work items; workgroups walk them with stride gridDim.x
    int ksplit;        // >= 1: number of K ranges each output tile is cut into (split-K)
    float *ws;         // split-K partial sums [ksplit][npix][Cout]; stream-K: piece slots (see sk_tiles)
    // Stream-K (persistent kernels): the LAST sk_tiles output tiles are not walked whole.  Their sk_tiles * nk K-tile
    // iterations are dealt in equal contiguous shares to workgroups 0 .. sk_wgs-1 by the rule of y2_streamk_rule.h (share <=
    // one tile: sk_tiles <= sk_wgs), each share is one or two pieces (tile, K range) whose raw fp32 sums go to slot 2*wg + piece
    // of `ws`, and a fix-up launch adds a tile's pieces in ascending K order and applies the epilogue.  0 = every tile is walked whole.
    int sk_tiles, sk_wgs;
    // fp32 matrix-core kernel, wide heads (yolo9000's 28 269-filter 1x1: 116 MB of weights against 9.5 MB of input): tiles are
    // dealt per XCD -- workgroups b with the same b % 8 share an L2 -- so that XCD x owns filter tiles x, x + 8, ... (every
    // weight byte enters ONE L2) and walks them in blocks of `pblk` pixel tiles whose input rows stay L2-resident meanwhile.
    // 0 = plain order (filter tile fastest).  Needs gridDim.x % 8 == 0 and ksplit == 1; placement is speed only.
    int xcd_order, tiles_m, pblk;
    int row0;          // fp16 matrix-core kernels: first GEMM row of this launch (tail launch behind the 256x256 kernel); tile t starts at row0 + (t / tiles_n) * BM
    unsigned long long *stamps;   // diagnostic builds (-DY2_F32_STAMPS): per-wave cycle counters
    // stride / out_h / out_w: fp32 matrix-core and direct kernels; size / pad / batch: direct kernel only
    int size, stride, pad, out_h, out_w, batch;
};

// The reference's epilogue, step by step (blas.c:122, convolutional_layer.c:407-419, activations.h:35-41)
__device__ __forceinline__ float epilogue(float v, bool bn, float mean, double rinv, float scale, float bias, int act)
{
    if (bn) {
        float d = v - mean;                 // blas.c:122 numerator, fp32
        v = (float)((double)d * rinv);      // divide by (sqrt(var)+1e-6f) evaluated in double
        v = v * scale;                      // convolutional_layer.c:419
    }
    v = v + bias;                           // convolutional_layer.c:407
    if (act == Y2H_ACT_LEAKY) v = (v > 0) ? v : (float)(.1 * (double)v);              // activations.h:41
    else if (act == Y2H_ACT_LOGISTIC) v = (float)(1. / (1. + exp(-(double)v)));       // activations.h:35
    else if (act == Y2H_ACT_RELU) v = v * (float)(v > 0);                             // activations.h:37
    return v;
}

// Fused conv + maxpool: the epilogue is a MONOTONE function of the accumulator -- every step (x - mean, * rinv > 0 in
// double, * scale, + bias, leaky / linear / logistic / relu) is monotone and every rounding is monotone; the whole is
// non-decreasing when scale >= 0 (or without batch-norm) and non-increasing otherwise.  So
//     max_t epilogue(acc_t) == epilogue(max_t acc_t)      (scale >= 0),      == epilogue(min_t acc_t)     (scale < 0)
// EXACTLY, and a pooling window costs one epilogue evaluation instead of four (the first layer was bound by this
// arithmetic: 378 M double-precision evaluations per 32 frames of 608x608).
__device__ __forceinline__ float pool_pick(float a0, float a1, float a2, float a3, bool increasing)
{
    const float mx = __builtin_fmaxf(__builtin_fmaxf(a0, a1), __builtin_fmaxf(a2, a3));
    const float mn = __builtin_fminf(__builtin_fminf(a0, a1), __builtin_fminf(a2, a3));
    return increasing ? mx : mn;
}

// fp16 path: BN folded into one fma on the fp32 accumulator (alpha = scale/(sqrt(var)+1e-6), beta = bias - mean*alpha),
// fp32 activation.  There is no reference arithmetic to mirror here: the reference has no half path.
__device__ __forceinline__ float epilogue_fast(float v, float alpha, float beta, int act)
{
    v = __builtin_fmaf(v, alpha, beta);
    if (act == Y2H_ACT_LEAKY) v = __builtin_fmaxf(v, 0.1f * v);       // slope < 1: max(v, .1v) is the leaky select
    else if (act == Y2H_ACT_LOGISTIC) v = 1.f / (1.f + __expf(-v));
    else if (act == Y2H_ACT_RELU) v = (v > 0.f) ? v : 0.f;
    return v;
}

// Fused conv + 2x2/2 maxpool (maxpool_layer.c:79-114 with size 2, stride 2, pad 0).
// The GEMM rows are enumerated in POOL-MAJOR order: row r = 4*q + t is pixel
// (2*yo + t/2, 2*xo + t%2) of pooling window q = (n, yo, xo).  An MFMA accumulator lane holds
// rows (reg&3) + 8*(reg>>2) + 4*half, i.e. registers 4g..4g+3 are the four pixels of ONE window,
// so the pool is a max over four registers of the same lane -- no cross-lane traffic -- and the
// full-resolution activation is never written.  Values are identical to conv followed by maxpool.
__device__ __forceinline__ int pool_pixel(int r, int H, int W)
{
    const int q = r >> 2, t = r & 3;
    const int Wp = W >> 1, HWp = (H >> 1) * Wp;
    const int n = q / HWp, rem = q - n * HWp;
    const int yo = rem / Wp, xo = rem - yo * Wp;
    return (n * H + 2 * yo + (t >> 1)) * W + 2 * xo + (t & 1);
}

// ---------------------------------------------------------------------------
// The staging side of the implicit-GEMM kernels.  conv_mfma_f16_kernel uses all of it; conv_mfma_kernel the tap mask and the
// slice address, conv_p8_f16_kernel neither: those two carry their own copy of the rest, with a comment that says why.
// A thread stages one 16-byte chunk, at byte offset `chunk` of a row's BK channels, of the GEMM rows sr + q * RP of the
// pixel tile and of the filter tile.  T = element type, KS = filter size; what callers differ in is a template argument.
// ---------------------------------------------------------------------------
// bit kh*KS+kw = tap (kh, kw) of the pixel (px, py) lies inside the W x H image (pad = KS/2): a column pattern times a row
// pattern spread KS bits apart, no carries.  Any odd size with KS*KS <= 32 taps (5x5: alexnet.cfg).
template <int KS>
__device__ __forceinline__ unsigned conv_tap_mask(int px, int py, int W, int H)
{
    static_assert(KS * KS <= 32, "one mask bit per tap");
    if (KS == 1) return 1u;
    if (KS == 3) {
        const unsigned xm = (px > 0 ? 1u : 0u) | 2u | (px < W - 1 ? 4u : 0u);
        const unsigned ym = (py > 0 ? 1u : 0u) | 8u | (py < H - 1 ? 64u : 0u);
        return xm * ym;
    }
    unsigned xm = 0, ym = 0;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        if (px + k - KS / 2 >= 0 && px + k - KS / 2 < W) xm |= 1u << k;
        if (py + k - KS / 2 >= 0 && py + k - KS / 2 < H) ym |= 1u << (k * KS);
    }
    return xm * ym;
}

// K-slice (tap, c0) = channels c0 .. c0 + BK - 1 of one filter tap.  K order: channel chunk outermost, the KS*KS taps
// innermost -- the taps of one chunk touch the same (neighbouring) pixel lines, so all but one of the A-slice reads hit L1/L2.
// Byte offset of the slice from the centre pixel's channel 0 ...
template <int KS, int ESZ>
__device__ __forceinline__ unsigned conv_slice_a(int tap, int c0, int W, int ldx)
{
    int delta = 0;        // element offset of the tap relative to the centre pixel
    if (KS > 1) {
        const int kh = tap / KS, kw = tap - kh * KS;
        delta = ((kh - KS / 2) * W + (kw - KS / 2)) * ldx;
    }
    return (unsigned)((delta + c0) * ESZ);
}
// ... and from the start of a packed weight row
template <int ESZ>
__device__ __forceinline__ unsigned conv_slice_b(int tap, int c0, int Cin) { return (unsigned)((tap * Cin + c0) * ESZ); }
template <int KS, int BK>
__device__ __forceinline__ void conv_slice_next(int &tap, int &c0) { if (++tap == KS * KS) { tap = 0; c0 += BK; } }

// Row metadata of the pixel tile at GEMM row p0 (`live` false: a tile past the end, everything masked): a_off = byte
// offset of the row's centre pixel (+ chunk), a_msk = its tap mask.  ONE coordinate decode per thread and tile: this
// thread's rows are RP apart, so the image coordinates of the following rows come from a carry update (unit grid = pooling
// windows, row r = 4*window + corner, with the fused pool; pixels without).  Stride 1: the GEMM rows enumerate a.H x a.W.
template <typename T, int KS, int BM, int RP, int PA>
__device__ __forceinline__ void conv_stage_rows(const ConvK a, bool live, int p0, int sr, unsigned chunk, unsigned (&a_off)[PA], unsigned (&a_msk)[PA])
{
    static_assert(RP % 4 == 0, "rows of one thread must keep their pooling-window corner");
    const int Wu = a.pool ? a.W >> 1 : a.W, Hu = a.pool ? a.H >> 1 : a.H;
    const int r0 = p0 + sr;
    const int u0 = a.pool ? r0 >> 2 : r0, tc = r0 & 3;
    int cn = u0 / (Hu * Wu);
    int cy = (u0 - cn * Hu * Wu) / Wu, cx = u0 - cn * Hu * Wu - cy * Wu;
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const int r = r0 + q * RP;                            // GEMM row
        const int py = a.pool ? 2 * cy + (tc >> 1) : cy, px = a.pool ? 2 * cx + (tc & 1) : cx;
        a_off[q] = (unsigned)((cn * a.H + py) * a.W + px) * (unsigned)a.ldx * (unsigned)sizeof(T) + chunk;
        a_msk[q] = (live && r < a.npix && (BM % RP == 0 || sr + q * RP < BM)) ? conv_tap_mask<KS>(px, py, a.W, a.H) : 0u;
        cx += a.pool ? RP / 4 : RP;
        while (cx >= Wu) { cx -= Wu; if (++cy >= Hu) { cy = 0; ++cn; } }
    }
}

// b_off = byte offset of the filter tile's weight rows (+ chunk); rows past Cout or the tile: a.wbytes, which reads as zero
template <typename T, int BN, int RP, int PB>
__device__ __forceinline__ void conv_stage_filters(const ConvK &a, bool live, int n0, int sr, unsigned chunk, unsigned (&b_off)[PB])
{
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const unsigned co = (unsigned)(n0 + sr + q * RP);
        b_off[q] = (live && co < (unsigned)a.Cout && (BN % RP == 0 || sr + q * RP < BN)) ? co * (unsigned)a.K * (unsigned)sizeof(T) + chunk : a.wbytes;
    }
}

// Register-staged kernels: fetch slice (tap, c0) into ra / rb and move on to the next slice; padding taps and rows past
// the end are out-of-range buffer loads (zeros, no memory traffic) -- cheaper than a branch, which would split the
// scheduling region.
template <typename T, int KS, int BK, int PA, int PB>
__device__ __forceinline__ void conv_load_slice(const ConvK &a, __amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t wr, int &tap, int &c0,
                                                const unsigned (&a_off)[PA], const unsigned (&a_msk)[PA], const unsigned (&b_off)[PB],
                                                f32x4 (&ra)[PA], f32x4 (&rb)[PB])
{
    const unsigned add = conv_slice_a<KS, (int)sizeof(T)>(tap, c0, a.W, a.ldx);
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const bool ok = (a_msk[q] >> tap) & 1u;
        const unsigned off = ok ? a_off[q] + add : a.xbytes;
        ra[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
    const unsigned kadd = conv_slice_b<(int)sizeof(T)>(tap, c0, a.Cin);
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const unsigned off = (b_off[q] == a.wbytes) ? a.wbytes : b_off[q] + kadd;
        rb[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }
    conv_slice_next<KS, BK>(tap, c0);
}

// ... and write it to the LDS buffer at As: [BM + BN rows][LS elements], this thread's chunk sc of rows sr + q * RP
template <typename T, int BM, int BN, int LS, int RP, int PA, int PB>
__device__ __forceinline__ void conv_store_slice(T *As, int sr, int sc, const f32x4 (&ra)[PA], const f32x4 (&rb)[PB])
{
    constexpr int CW = 16 / (int)sizeof(T);       // elements per 16-byte chunk
    T *Bs = As + BM * LS;
#pragma unroll
    for (int q = 0; q < PA; ++q)
        if (BM % RP == 0 || sr + q * RP < BM) *(f32x4 *)&As[(sr + q * RP) * LS + sc * CW] = ra[q];
#pragma unroll
    for (int q = 0; q < PB; ++q)
        if (BN % RP == 0 || sr + q * RP < BN) *(f32x4 *)&Bs[(sr + q * RP) * LS + sc * CW] = rb[q];
}

// Which kernel runs a convolution and how it is launched: decided once per descriptor by conv_plan (y2_conv.hip), whose
// fp16 half is y2_f16_plan; every entry point (kernel name, weight layout, workspace size, the launch) reads the plan.
enum ConvKind {
    CK_NONE,                                  // no kernel takes the descriptor (an NCHW input nothing reads)
    CK_FIRST_NCHW_F16, CK_FIRST_NCHW_F32,     // first layer reading the fp32 NCHW network input
    CK_FIRST_F16, CK_FIRST_F32,               // first layer reading a one-pixel haloed copy (half NHWC4 / fp32 NHWC)
    CK_C32_F16, CK_C64_F16, CK_MFMA_F16,      // fp16 matrix-core kernels
    CK_C32_F32, CK_MFMA_F32, CK_STEM,         // fp32 matrix-core kernels
    CK_DIRECT,                                // reference accumulation order, reference-layout weights
};

struct Variant;
struct VariantH;
struct P8Plan {
    int sk_tiles, sk_wgs;          // stream-K (0: none)
    int tail_tiles;                // 256x256 tiles handed to the tail launch (0: none)
    VariantH *tail;
};

struct ConvPlan {
    ConvKind kind;
    const char *name;              // y2h_conv_variant
    size_t ws;                     // y2h_conv_workspace_bytes
    // fp32 matrix-core kernel.  v / ksplit: the cost model's choice among whole-tile launches with an integer K-split -- the
    // name and the first autotune candidate.  Set whenever that kernel takes the descriptor, also when conv_c32_f32 runs it.
    Variant *v;
    int ksplit;
    // What its launch runs: the stream-K form of sk_v on sk_wgs workgroups (0: none), or whole tiles of `tile`.  `tile` is v
    // unless a stream-K candidate shifted a near-tie of the cost model, and v when stream-K is chosen: then it is the launch
    // if y2h_conv.ws has no room for the pieces.  Its shape: the grid and the XCD-grouped tile order.
    Variant *sk_v;
    int sk_wgs;
    Variant *tile;
    int tile_ksplit;
    long grid;
    int xcd_order, tiles_m, pblk;
    double cost;                   // modelled CU cycles of the choice (pick_variant): the Winograd rule's "direct" side
    // fp16 matrix-core kernel (nullptr: no tile fits the descriptor -- the launch fails)
    VariantH *vh;
    long h_ntiles, h_grid;
    int h_tiles_n;
    P8Plan p8;
};

// fp16 side (y2_conv_f16.hip): fills p for an fp16-input descriptor (x_f16) and returns true when an fp16 kernel takes it
bool y2_f16_plan(const y2h_conv *d, ConvPlan &p);
int y2_f16_launch(const ConvPlan &p, const y2h_conv *d, ConvK &a, y2h_stream s);
bool y2_f16_first_ok(const y2h_conv *d);
bool y2_f16_first_nchw_ok(const y2h_conv *d);

// What every forward entry point (y2h_conv_forward and the three Winograd forms) asks of a descriptor before it plans: the
// pointers every kernel reads, sane dimensions and strides, the batch-norm constants where the layer normalizes.  Each adds
// its own conditions (w_packed, the output size, workspace size and alignment).
static inline bool conv_args_ok(const y2h_conv *d)
{
    if (!d || !d->x || !d->y || !d->bias) return false;
    if (d->batch <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->n <= 0 || d->ldx < d->c || d->ldy < d->n) return false;
    return !d->batch_normalize || (d->mean && d->rinv && d->scale);
}

// Winograd F(2x2,3x3) transforms (y2_wino.hip), the passes in front of and behind the batched GEMM of y2h_conv_wino_forward:
// V[16][tiles_pad][c] from the NHWC input of d; the layer's output from M[16][tiles_pad][n] through the shared epilogue.
int y2_wino_input_launch(const y2h_conv *d, float *V, long tiles, long tiles_pad, y2h_stream s);
int y2_wino_output_launch(const y2h_conv *d, const float *M, long tiles, long tiles_pad, y2h_stream s);
// The split form (include/y2_split_rule.h): V as three bf16 planes in the layout of y2_split_index (y2_wino.hip), and the
// batched GEMM on the bf16 matrix cores, raw fp32 sums to M[16][tiles_pad][n] (y2_wino_split.hip).
int y2_wino_input_split_launch(const y2h_conv *d, unsigned short *V, long tiles, long tiles_pad, y2h_stream s);
int y2_wino_split_gemm_launch(const unsigned short *V, const unsigned short *U, float *M, long tiles_pad, int c, int n, y2h_stream s);

// Grid of a kernel that walks its tiles with a grid stride: exactly what is co-resident (256 CUs x the runtime's answer for
// this kernel), no more -- a surplus block only starts when a resident one has finished ALL its tiles, i.e. runs a second,
// nearly empty round (the first-layer kernel asked for four blocks per CU with registers for three: 1024 blocks, 768
// resident).  Cached per kernel and device.
static inline long resident_blocks(const void *fn, int threads, size_t lds, long fallback_per_cu)
{
    struct Entry { const void *fn; int dev; size_t lds; int per_cu; };
    static Entry cache[32];
    static int n = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256L * fallback_per_cu;
    for (int i = 0; i < n; ++i) if (cache[i].fn == fn && cache[i].dev == dev && cache[i].lds == lds) return 256L * cache[i].per_cu;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu < 1) per_cu = (int)fallback_per_cu;
    if (getenv("Y2_FIRST_GRID_PER_CU")) per_cu = atoi(getenv("Y2_FIRST_GRID_PER_CU")) > 0 ? atoi(getenv("Y2_FIRST_GRID_PER_CU")) : per_cu;
    if (n < 32) { cache[n].fn = fn; cache[n].dev = dev; cache[n].lds = lds; cache[n].per_cu = per_cu; ++n; }
    return 256L * per_cu;
}

