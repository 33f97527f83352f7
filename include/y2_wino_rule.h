/*
 * The Winograd rule: which fp32 3x3 convolutions run as F(2x2,3x3) -- input transform, sixteen batched 1x1 GEMMs on the
 * matrix cores, output transform + epilogue -- instead of the direct implicit GEMM.  Host arithmetic only; the tile table
 * and the direct plan's cost are the dispatch's (y2_conv.hip: y2h_wino_plan puts the two together).
 *
 * F(2x2,3x3) computes a 2x2 output patch from a 4x4 input patch with 16 multiplies per (channel, filter) instead of 36:
 *     Y = A^T [ (G g G^T) .* (B^T d B) ] A
 * The sum over channels of the element-wise products is, per component g = 4 i + j of the 4x4 patch, one GEMM
 *     M[g][tile][n] = sum_c V[g][tile][c] * U[g][n][c]
 * with T = batch * ceil(H/2) * ceil(W/2) tiles per component.  V holds T padded to a multiple of the GEMM's BM rows per
 * component (padding rows zero), so that no GEMM tile straddles two components.
 *
 * Cost, in CU cycles like pick_variant's: the batched GEMM by the direct kernel's own formula on its 1x1 tiles, plus the
 * bytes the two transform passes move at 5.75e-4 cycles per byte (4 TB/s at 2.4 GHz), plus two launch boundaries.
 * Winograd is taken when that is below the direct plan's cost by Y2_WINO_MARGIN.
 */
#ifndef Y2_WINO_RULE_H
#define Y2_WINO_RULE_H

#include <stddef.h>

#define Y2_WINO_BYTE_CYCLES 5.75e-4       /* one byte of a transform pass (the cost model's workspace round-trip rate) */
#define Y2_WINO_LAUNCH_CYCLES 5000.0      /* one more launch boundary (as a split-K reduction is charged) */
/* The margin: 10 %.  Set against the measured per-layer table of yolo.cfg 608x608 batch 32 (profiles/wino_608b32.txt,
 * section 3): every layer the rule takes with it measured 34-44 % faster than its direct form, the two 152x152 layers that
 * measured slower with Winograd are 80-90 % away from being taken, and the model over-charges Winograd by 20-30 % on every
 * row (the 76x76 layers it leaves direct would be 14 % faster) -- its error is on the side of leaving a layer alone, so no
 * layer measured slower is taken and the margin needs no widening. */
#define Y2_WINO_MARGIN 0.10

/* the shapes the three kernels take (the caller also asks that the direct plan is the fp32 matrix-core kernel) */
static inline int y2_wino_shape_ok(int size, int stride, int pad, int c, int n, int h, int w, int out_h, int out_w, int pool,
                                   int x_f16, int y_f16, int x_halo, int x_nchw, int ldx)
{
    if (x_f16 || y_f16 || x_halo || x_nchw) return 0;
    if (size != 3 || stride != 1 || pad != 1 || out_h != h || out_w != w) return 0;
    if (c % 32 != 0 || n % 4 != 0 || ldx % 4 != 0) return 0;
    if (pool && ((h | w) & 1)) return 0;
    return 1;
}

static inline long y2_wino_tiles(int batch, int h, int w) { return (long)batch * ((h + 1) / 2) * ((w + 1) / 2); }
static inline long y2_wino_tiles_pad(long tiles, int bm) { return (tiles + bm - 1) / bm * bm; }

/* bytes of the two transform passes: the input read once and V written; M read and the output written */
static inline double y2_wino_transform_bytes(int batch, int h, int w, int c, int n, int pool, long tiles_pad)
{
    const double in = (double)batch * h * w * c * 4.0, out = (double)batch * h * w * n * 4.0 * (pool ? 0.25 : 1.0);
    return in + 16.0 * (double)tiles_pad * c * 4.0 + 16.0 * (double)tiles_pad * n * 4.0 + out;
}

static inline double y2_wino_cost(double gemm_cost, double transform_bytes)
{
    return gemm_cost + transform_bytes * Y2_WINO_BYTE_CYCLES + 2.0 * Y2_WINO_LAUNCH_CYCLES;
}

static inline int y2_wino_wins(double direct_cost, double wino_cost) { return wino_cost < direct_cost * (1.0 - Y2_WINO_MARGIN); }

/* G g G^T of one 3x3 filter (row-major g[9]) -> u[16], evaluated in double and rounded once to fp32.
 * G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1].  Small integer filters give exact multiples of 1/4. */
static inline void y2_wino_filter(const float *g, float *u)
{
    static const double G[4][3] = { {1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0} };
    double t[4][3];
    int i, j, k;
    for (i = 0; i < 4; ++i)
        for (j = 0; j < 3; ++j) {
            t[i][j] = 0.0;
            for (k = 0; k < 3; ++k) t[i][j] += G[i][k] * (double)g[k * 3 + j];
        }
    for (i = 0; i < 4; ++i)
        for (j = 0; j < 4; ++j) {
            double s = 0.0;
            for (k = 0; k < 3; ++k) s += t[i][k] * G[j][k];
            u[i * 4 + j] = (float)s;
        }
}

#endif
