// The three products of a trainable convolution on the bf16 matrix cores (gfx950, v_mfma_f32_32x32x16_bf16): the implicit
// GEMM of y2_train.hip -- the same three forms FWD / DX / DW, the same (pixel, tap) gathers with the same guarded edges, no
// im2col buffer, no floating-point atomic -- with the fp32 operands turned into bf16 where they are staged into LDS:
//   PLANES = 3  every value is split a = h + m + l (y2_split3 of include/y2_split_rule.h, restated below as in y2_wino.hip)
//               and the six products of order <= 2 are issued smallest first, l h', h l', m m', m h', h m', h h', as
//               y2_wino_split.hip issues them: fp32 results, terms below 2^-25 |a b| dropped;
//   PLANES = 1  every value is rounded once to nearest even (y2_bf16_rn): one MFMA per 16 reduction values.
// Accumulators are fp32 either way.
//
// A workgroup of four waves owns a 64 x 64 output tile, 32 x 32 per wave, and walks the reduction 32 values at a time.
// LDS holds per operand and plane four slabs, one per group of 8 consecutive reduction values; a slab is
// [64 rows][8 values] bf16, so the fragment a lane feeds the MFMA -- 8 consecutive reduction values of one row -- is one
// 16-byte read, and the 32 rows a half-wave reads are 512 contiguous bytes: every 16-lane group of ds_read_b128 covers the
// 64 banks once.  Slabs are 32 bytes apart beyond their 1024, which spreads the 16-byte stores of the row-contiguous staging
// (lane = 4 rows' worth of k-groups: rows 16 bytes apart, k-groups one slab apart) over distinct bank slots.
//
// Staging, per thread 8 consecutive reduction values of one row per operand:
//   row-contiguous operands (A of FWD and DX, B of DX: the reduction index runs along NHWC channels): thread = (row t / 4,
//     k-group t % 4); with a channel count that is a multiple of 8 and 16-byte aligned tensors the 8 values are one tap's
//     and come as two 16-byte loads (VEC), otherwise the tap is walked value by value through the guarded scalar gather;
//   the others (B of FWD and DW: [r][j] rows; A of DW: one tap per row, pixels along r): thread = (row t % 64, k-group
//     t / 64 = its wave), eight scalar loads that are contiguous across the wave's lanes; the pixels are wave-uniform.
// The weight gradient keeps y2h_train_dweight_splits, its ranges, workspace and second pass, so a step stays reproducible.
// Compiled with -ffp-contract=off like the other conv units.
#include "y2_train_geo.hpp"
#include "y2_split_rule.h"
#include "y2_split_dev.hpp"      // bf16_rn_x4, split3_x4, put_planes

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int KB = 32;                        // reduction depth of one staging step: two MFMA steps
constexpr int KG = KB / 8;                    // k-groups of a staging step
constexpr int SLAB = TB * 16 + 32;            // bytes from one (plane, k-group) slab to the next

__device__ __forceinline__ void tap_step(Tap &t, int k, int lim, int ksize, int chans)      // tap_of(k - 1) -> tap_of(k)
{
    t.ok = k < lim;
    if (++t.ch == chans) {
        t.ch = 0;
        if (++t.kx == ksize) { t.kx = 0; ++t.ky; }
    }
}

// where the 8 values of tap t (t.ch a multiple of 8, 8 | channels) of pixel p start, or NULL for padding / past an edge
template <int MODE>
__device__ __forceinline__ const float *a_run(const float *__restrict__ src, const Geo &g, const Pix &p, const Tap &t)
{
    if (!p.ok || !t.ok) return nullptr;
    if (MODE == DX) {
        const int oy = p.y + g.P - t.ky, ox = p.x + g.P - t.kx;
        if ((unsigned)oy >= (unsigned)g.OH || (unsigned)ox >= (unsigned)g.OW) return nullptr;
        return src + ((size_t)(p.b * g.OH + oy) * g.OW + ox) * g.N + t.ch;
    }
    const int iy = p.y - g.P + t.ky, ix = p.x - g.P + t.kx;
    if ((unsigned)iy >= (unsigned)g.H || (unsigned)ix >= (unsigned)g.W) return nullptr;
    return src + ((size_t)(p.b * g.H + iy) * g.W + ix) * g.C + t.ch;
}

__device__ __forceinline__ void load8(const float *p, float (&v)[8])
{
    if (p) {
        const f32x4 a = *(const f32x4 *)p, b = *(const f32x4 *)(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
}

// blockIdx.z = the reduction range; a launch with ranges writes range z's tile to dst + z * I * J
template <int MODE, int PLANES, bool VEC>
__global__ __launch_bounds__(256) void train_gemm_bf16(const float *__restrict__ asrc, const float *__restrict__ bsrc,
                                                       float *__restrict__ dst, Geo g, int range)
{
    constexpr bool A_RC = MODE != DW, B_RC = MODE == DX;
    static_assert(!VEC || A_RC, "16-byte loads need the reduction index along channels");
    __shared__ __attribute__((aligned(16))) unsigned char As[PLANES * KG * SLAB], Bs[PLANES * KG * SLAB];
    const int t = threadIdx.x, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);          // uniform: the pixels a wave stages are scalar work
    const int wi = wave & 1, wj = wave >> 1;
    const int i0 = blockIdx.x * TB, j0 = blockIdx.y * TB;
    const int rbeg = blockIdx.z * range;
    const int rend = (rbeg + range < g.R) ? rbeg + range : g.R;
    const int ph = MODE == DX ? g.H : g.OH, pw = MODE == DX ? g.W : g.OW;      // what a pixel index counts
    const int tch = MODE == DX ? g.N : g.C;                                   // what a tap's channel counts
    dst += (size_t)blockIdx.z * g.I * g.J;

    // which 8 values of which row each thread stages, and the part of their address that does not move with r
    const int a_row = A_RC ? t >> 2 : t & 63, a_kg = A_RC ? t & 3 : wave;
    const int b_row = B_RC ? t >> 2 : t & 63, b_kg = B_RC ? t & 3 : wave;
    Pix pa_fixed;
    Tap ta_fixed;
    if (A_RC) pa_fixed = pix_of(i0 + a_row, g.I, ph, pw);
    else ta_fixed = tap_of(i0 + a_row, g.I, g.K, tch);

    float ra[8], rb[8];
    auto fetch = [&](int r0) {
        if (A_RC) {
            const int k0 = r0 + a_kg * 8;                 // == r0 + b_kg * 8 where B_RC: DX's B reads the same taps
            Tap ta = tap_of(k0, rend, g.K, tch);
            const int j = j0 + b_row;
            if (VEC) {
                load8(a_run<MODE>(asrc, g, pa_fixed, ta), ra);
                if (B_RC) load8((ta.ok && j < g.J) ? bsrc + ((size_t)(ta.ky * g.K + ta.kx) * g.C + j) * g.N + ta.ch : nullptr, rb);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (e) tap_step(ta, k0 + e, rend, g.K, tch);
                    ra[e] = a_val<MODE>(asrc, g, pa_fixed, ta);
                    if (B_RC) rb[e] = (ta.ok && j < g.J) ? bsrc[((size_t)(ta.ky * g.K + ta.kx) * g.C + j) * g.N + ta.ch] : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ra[e] = a_val<MODE>(asrc, g, pix_of(r0 + a_kg * 8 + e, rend, ph, pw), ta_fixed);
        }
        if (!B_RC) {
            const int j = j0 + b_row;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int r = r0 + b_kg * 8 + e;
                rb[e] = (r < rend && j < g.J) ? bsrc[(size_t)r * g.J + j] : 0.f;
            }
        }
    };

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    unsigned char *const a_put = As + a_kg * SLAB + a_row * 16, *const b_put = Bs + b_kg * SLAB + b_row * 16;
    const unsigned char *const a_get = As + lh * SLAB + (wi * 32 + li) * 16, *const b_get = Bs + lh * SLAB + (wj * 32 + li) * 16;

    if (rbeg < rend) fetch(rbeg);
    for (int r0 = rbeg; r0 < rend; r0 += KB) {
        __syncthreads();                                  // the previous step's fragments have been read
        put_planes<PLANES, KG * SLAB>(a_put, ra);
        put_planes<PLANES, KG * SLAB>(b_put, rb);
        __syncthreads();
        if (r0 + KB < rend) fetch(r0 + KB);               // the next step's loads fly under this step's MFMAs
#pragma unroll
        for (int ks = 0; ks < KB / 16; ++ks) {
            bf16x8 af[PLANES], bf[PLANES];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) {
                af[p] = *(const bf16x8 *)(a_get + (p * KG + 2 * ks) * SLAB);
                bf[p] = *(const bf16x8 *)(b_get + (p * KG + 2 * ks) * SLAB);
            }
            if constexpr (PLANES == 1) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bf[0], acc, 0, 0, 0);
            } else {
                // (plane of A, plane of B), smallest product first
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[q]], bf[PB[q]], acc, 0, 0, 0);
            }
        }
    }
    const int col = j0 + wj * 32 + li;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = i0 + wi * 32 + (v >> 2) * 8 + lh * 4 + (v & 3);
        if (row < g.I && col < g.J) dst[(size_t)row * g.J + col] = acc[v];
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <int MODE, int PLANES>
int launch(const Geo &g, const float *a, const float *b, float *dst, int z, int range, y2h_stream s)
{
    if (MODE != DW && (MODE == DX ? g.N : g.C) % 8 == 0 && aligned16(a) && aligned16(b))
        train_gemm_bf16<MODE, PLANES, MODE != DW><<<tiles_of(g, z), 256, 0, S(s)>>>(a, b, dst, g, range);
    else
        train_gemm_bf16<MODE, PLANES, false><<<tiles_of(g, z), 256, 0, S(s)>>>(a, b, dst, g, range);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

template <int MODE>
int launch_planes(int planes, const Geo &g, const float *a, const float *b, float *dst, int z, int range, y2h_stream s)
{
    return planes == 3 ? launch<MODE, 3>(g, a, b, dst, z, range, s) : launch<MODE, 1>(g, a, b, dst, z, range, s);
}

}  // namespace

extern "C" {

int y2h_train_conv_forward_bf16(const y2h_train_conv *c, const float *x, const float *w, float *y, int planes, y2h_stream s)
{
    Geo g;
    if (!x || !w || !y || (planes != 1 && planes != 3) || geo_of(c, FWD, &g) != Y2H_OK) return Y2H_EINVAL;
    return launch_planes<FWD>(planes, g, x, w, y, 1, g.R, s);
}

int y2h_train_conv_dinput_bf16(const y2h_train_conv *c, const float *dy, const float *w, float *dx, int planes, y2h_stream s)
{
    Geo g;
    if (!dy || !w || !dx || (planes != 1 && planes != 3) || geo_of(c, DX, &g) != Y2H_OK) return Y2H_EINVAL;
    return launch_planes<DX>(planes, g, dy, w, dx, 1, g.R, s);
}

int y2h_train_conv_dweight_bf16(const y2h_train_conv *c, const float *x, const float *dy, float *dw, float *ws, int planes, y2h_stream s)
{
    Geo g;
    if (!x || !dy || !dw || !ws || (planes != 1 && planes != 3) || geo_of(c, DW, &g) != Y2H_OK) return Y2H_EINVAL;
    const int splits = y2h_train_dweight_splits(c);
    const int rc = launch_planes<DW>(planes, g, x, dy, ws, splits, dweight_range(g, splits), s);
    if (rc != Y2H_OK) return rc;
    return y2_train_dweight_finish(ws, dw, (long)g.I * g.J, splits, s);
}

}  // extern "C"
