// What the two implicit-GEMM templates of the trainer share (y2_train.hip: fp32 operands; y2_train_bf16.hip: bf16 operands,
// split or rounded): the three forms, the 64 x 64 output tile, the (pixel, tap) addressing of the gathered operand, the
// shapes both accept and the second pass of the weight gradient.
#pragma once
#include "y2_common.hpp"

namespace {

enum { FWD = 0, DX = 1, DW = 2 };
constexpr int TB = 64;            // output tile: TB x TB per workgroup of four waves, 32 x 32 per wave

struct Geo { int B, H, W, C, N, K, P, OH, OW; int I, J, R; };
struct Pix { int b, y, x; bool ok; };
struct Tap { int ky, kx, ch; bool ok; };

__device__ __forceinline__ Pix pix_of(int m, int lim, int h, int w)
{
    Pix p;
    p.ok = m < lim;
    const int mm = p.ok ? m : 0, hw = h * w;
    p.b = mm / hw;
    const int r = mm - p.b * hw;
    p.y = r / w;
    p.x = r - p.y * w;
    return p;
}

__device__ __forceinline__ Tap tap_of(int k, int lim, int ksize, int chans)
{
    Tap t;
    t.ok = k < lim;
    const int kk = t.ok ? k : 0, q = kk / chans;
    t.ch = kk - q * chans;
    t.ky = q / ksize;
    t.kx = q - t.ky * ksize;
    return t;
}

template <int MODE>
__device__ __forceinline__ float a_val(const float *__restrict__ src, const Geo &g, const Pix &p, const Tap &t)
{
    if (!p.ok || !t.ok) return 0.f;
    if (MODE == DX) {
        const int oy = p.y + g.P - t.ky, ox = p.x + g.P - t.kx;
        if ((unsigned)oy >= (unsigned)g.OH || (unsigned)ox >= (unsigned)g.OW) return 0.f;
        return src[((size_t)(p.b * g.OH + oy) * g.OW + ox) * g.N + t.ch];
    }
    const int iy = p.y - g.P + t.ky, ix = p.x - g.P + t.kx;
    if ((unsigned)iy >= (unsigned)g.H || (unsigned)ix >= (unsigned)g.W) return 0.f;
    return src[((size_t)(p.b * g.H + iy) * g.W + ix) * g.C + t.ch];
}

inline int geo_of(const y2h_train_conv *c, int mode, Geo *g)
{
    if (!c || c->batch <= 0 || c->h <= 0 || c->w <= 0 || c->c <= 0 || c->n <= 0 || c->size <= 0 || c->pad < 0) return Y2H_EINVAL;
    if (c->out_h != c->h + 2 * c->pad - c->size + 1 || c->out_w != c->w + 2 * c->pad - c->size + 1 || c->out_h <= 0 || c->out_w <= 0)
        return Y2H_EINVAL;
    const long mo = (long)c->batch * c->out_h * c->out_w, mi = (long)c->batch * c->h * c->w;
    const long kc = (long)c->size * c->size * c->c, kn = (long)c->size * c->size * c->n;
    if (mo * c->n >= 2147483647L || mi * c->c >= 2147483647L || kc * c->n >= 2147483647L) return Y2H_EINVAL;   // int indices
    g->B = c->batch; g->H = c->h; g->W = c->w; g->C = c->c; g->N = c->n; g->K = c->size; g->P = c->pad;
    g->OH = c->out_h; g->OW = c->out_w;
    if (mode == FWD) { g->I = (int)mo; g->J = c->n; g->R = (int)kc; }
    else if (mode == DX) { g->I = (int)mi; g->J = c->c; g->R = (int)kn; }
    else { g->I = (int)kc; g->J = c->n; g->R = (int)mo; }
    return Y2H_OK;
}

inline dim3 tiles_of(const Geo &g, int z) { return dim3((g.I + TB - 1) / TB, (g.J + TB - 1) / TB, z); }

// the weight gradient's reduction ranges: y2h_train_dweight_splits of them, each a multiple of 16 long (the fp32 template's
// staging depth; the partition is part of what makes a step reproducible, so both templates take it from here)
inline int dweight_range(const Geo &g, int splits) { return ((g.R + splits - 1) / splits + 15) / 16 * 16; }

}  // namespace

// dw[e] += the `splits` partial tiles of ws in range order (y2_train.hip)
int y2_train_dweight_finish(const float *ws, float *dw, long n, int splits, y2h_stream s);
