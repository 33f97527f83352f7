/*
 * The 3-way bf16 split of the fp32 Winograd GEMMs: the split itself, the operand layout of the split GEMM
 * (y2_wino_split.hip) and the rule that decides which Winograd layers take the form.  Host arithmetic only, C; the device
 * side restates y2_split3 with v_cvt_pk_bf16_f32 (y2_wino.hip) and the index below.
 *
 * The split.  An fp32 number is exactly the sum of three bf16 numbers, a = h + m + l:
 *     h = bf16_rn(a),  m = bf16_rn(a - h),  l = (a - h) - m
 * Both subtractions are exact in fp32 (each remainder is below half an ulp of the part before it and a multiple of a's own
 * ulp), every part has fp32's exponent range and at most 8 significant bits, and a value with at most 16 significant bits
 * has l == 0.  Conversions round to nearest even.  Three cases need a word:
 *   - bf16 has fp32's exponents but its smallest subnormal is 2^-133, not 2^-149: the sum is exact for every a that is a
 *     multiple of 2^-133 (all normal values from 2^-110 up among them); a tinier bit is rounded away, the sum is then within
 *     2^-134 of a;
 *   - a non-finite a gives h = a, m = l = 0 (inf - inf would be a NaN);
 *   - a finite a that bf16_rn would round to an infinity (|a| >= 0x7f7f8000 as bits) takes the largest finite bf16 of its
 *     sign as h; the remainder then has at most 16 bits and the sum is still exact.
 *
 * The product.  With b = h' + m' + l', the GEMM keeps the six products of order <= 2
 *     h h' + (h m' + m h') + (h l' + l h' + m m')
 * each exact in fp32 (8 x 8 bits); the three dropped ones are below 2^-25 |a b|, under the half ulp the fp32 product
 * rounding costs.  On operands of at most 16 significant bits (l == l' == 0, e.g. integers below 2^16 and multiples of 1/4)
 * the dropped terms are zero and the six are the whole product.
 *
 * The layout.  A split operand X[g][row][c] (g: the sixteen Winograd components; rows: tiles for V, filters for U, padded
 * with zero rows to a multiple of Y2_SPLIT_ROWS; c: input channels, a multiple of Y2_SPLIT_BK) is stored as bf16 in blocks
 * of one (component, row block of 256, K-tile of 16 channels):
 *     [g][row / 256][c / 16][plane h, m, l][c % 16 / 8][row % 256][c % 8]
 *   - a plane's k-fragment -- 8 consecutive channels of one row, the 16 bytes one lane feeds a 32x32x16 bf16 MFMA -- is
 *     contiguous;
 *   - one K-tile of one row BLOCK (256 rows x 16 channels x 3 planes = 24 KB) is one contiguous run, in exactly the order
 *     the kernel keeps it in LDS: LDS-DMA moves it with lane-linear 16-byte pieces on both sides, and a wave's fragment
 *     read (32 rows of one plane and k-half) is 512 contiguous bytes -- no bank conflict, no swizzle;
 *   - all K-tiles of one row block are contiguous (c / 16 inside row / 256), so a GEMM tile streams one run per operand.
 * (A run per single ROW would be 96 bytes: it straddles cache lines, and its LDS image has 2-way conflicts on the reads.)
 *
 * The rule.  The split form applies to layers the Winograd rule takes; it is chosen when its modelled cost is below the
 * fp32 Winograd form's by Y2_WINO_MARGIN.  Cost, in the Winograd
 * rule's units: the GEMM's matrix cycles -- six bf16 MFMAs per product, 6/16 of the fp32 instruction's, counted on the
 * split tile's own rounds -- over the share of the matrix rate the kernel holds, or its operand bytes (V, U, M once) at the
 * model's byte rate, whichever is larger; plus the two transform passes with V at
 * 6 bytes per element; plus two launch boundaries.
 */
#ifndef Y2_SPLIT_RULE_H
#define Y2_SPLIT_RULE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "y2_wino_rule.h"

#define Y2_SPLIT_ROWS 256          /* rows of a block = BM = BN of the main tile */
#define Y2_SPLIT_BK 16             /* channels of a K-tile = the K of one 32x32x16 MFMA */
#define Y2_SPLIT_BLOCK_ELEMS (3 * Y2_SPLIT_BK * Y2_SPLIT_ROWS)      /* bf16 values of one (row block, K-tile): 24 KB */
/* matrix cycles of one K-tile of one output tile: 48 MFMAs of 32 cycles on each of a SIMD's two waves -- per product the
 * 6/16 of the sixteen rate units v_mfma_f32_32x32x2_f32 takes */
#define Y2_SPLIT_KTILE_CYCLES 3072.0
/* Share of the bf16 matrix rate the split GEMM holds.  Set against the measured per-layer table of yolo.cfg 608x608 batch 32
 * (profiles/wino_split_608b32.txt, section 3) with the transform passes charged at the model's own rate: 0.52 on the
 * 256-channel 38x38 layers, 0.58-0.59 on the 19x19 ones.  With 0.52 the model is within 3 % on the 76x76 (byte-bound, forced) and
 * 38x38 layers and over-charges the 19x19 ones by 8-10 %. */
#define Y2_SPLIT_GEMM_EFF 0.52

static inline uint32_t y2_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float y2_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline float y2_bf16_f32(uint16_t b) { return y2_bits_f32((uint32_t)b << 16); }

/* round to nearest even; NaNs stay NaNs (quiet bit set); a finite value never becomes an infinity (see above) */
static inline uint16_t y2_bf16_rn(float f)
{
    const uint32_t u = y2_f32_bits(f), mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    if (mag == 0x7f800000u) return (uint16_t)(u >> 16);
    if (mag >= 0x7f7f8000u) return (uint16_t)((u >> 16 & 0x8000u) | 0x7f7fu);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static inline void y2_split3(float a, uint16_t *h, uint16_t *m, uint16_t *l)
{
    const uint32_t mag = y2_f32_bits(a) & 0x7fffffffu;
    float r;
    *h = y2_bf16_rn(a);
    if (mag >= 0x7f800000u) { *m = 0; *l = 0; return; }
    r = a - y2_bf16_f32(*h);
    *m = y2_bf16_rn(r);
    r = r - y2_bf16_f32(*m);
    *l = y2_bf16_rn(r);                             /* exact (the low 16 bits are zero) unless a has bits below 2^-133 */
}

static inline long y2_split_rows_pad(long rows) { return (rows + Y2_SPLIT_ROWS - 1) / Y2_SPLIT_ROWS * Y2_SPLIT_ROWS; }

/* index (in bf16 values) of plane p of X[g][row][c]; rows_pad a multiple of Y2_SPLIT_ROWS, c_total of Y2_SPLIT_BK */
static inline size_t y2_split_index(long rows_pad, int c_total, int g, long row, int c, int p)
{
    const size_t rb = (size_t)(rows_pad / Y2_SPLIT_ROWS), kt = (size_t)(c_total / Y2_SPLIT_BK);
    const size_t block = ((size_t)g * rb + (size_t)(row / Y2_SPLIT_ROWS)) * kt + (size_t)(c / Y2_SPLIT_BK);
    return block * Y2_SPLIT_BLOCK_ELEMS + ((size_t)(p * 2 + (c % Y2_SPLIT_BK) / 8) * Y2_SPLIT_ROWS + (size_t)(row % Y2_SPLIT_ROWS)) * 8 + (size_t)(c % 8);
}

/* bytes of a split operand: three bf16 planes */
static inline size_t y2_split_bytes(long rows_pad, int c) { return (size_t)16 * (size_t)rows_pad * (size_t)c * 6; }

/* the filters of a split layer: U = G g G^T (y2_wino_filter) of reference-layout weights [n][c][3][3], split, in the
 * layout above with filters as rows; rows n .. rows_pad - 1 are zero */
static inline void y2_split_pack_u(uint16_t *up, const float *weights, int n, int c)
{
    const long rows_pad = y2_split_rows_pad(n);
    int co, ci, g;
    memset(up, 0, y2_split_bytes(rows_pad, c));
    for (co = 0; co < n; ++co)
        for (ci = 0; ci < c; ++ci) {
            float u[16];
            y2_wino_filter(weights + ((size_t)co * c + ci) * 9, u);
            for (g = 0; g < 16; ++g) {
                uint16_t h, m, l;
                y2_split3(u[g], &h, &m, &l);
                up[y2_split_index(rows_pad, c, g, co, ci, 0)] = h;
                up[y2_split_index(rows_pad, c, g, co, ci, 1)] = m;
                up[y2_split_index(rows_pad, c, g, co, ci, 2)] = l;
            }
        }
}

/* the shapes the split form takes: the Winograd gate; the layout needs whole K-tiles, which c % 32 == 0 already gives */
static inline int y2_split_shape_ok(int size, int stride, int pad, int c, int n, int h, int w, int out_h, int out_w, int pool,
                                    int x_f16, int y_f16, int x_halo, int x_nchw, int ldx)
{
    return y2_wino_shape_ok(size, stride, pad, c, n, h, w, out_h, out_w, pool, x_f16, y_f16, x_halo, x_nchw, ldx) && c % Y2_SPLIT_BK == 0;
}

/* bytes of the two transform passes with V at 6 bytes per element */
static inline double y2_split_transform_bytes(int batch, int h, int w, int c, int n, int pool, long tiles_pad)
{
    const double in = (double)batch * h * w * c * 4.0, out = (double)batch * h * w * n * 4.0 * (pool ? 0.25 : 1.0);
    return in + 16.0 * (double)tiles_pad * c * 6.0 + 16.0 * (double)tiles_pad * n * 4.0 + out;
}

/* the GEMM: whole rounds of 256 workgroups over `blocks` output tiles of nk K-tiles each, or the operand bytes */
static inline double y2_split_gemm_cost(long blocks, int nk, double v_bytes, double u_bytes, double m_bytes)
{
    const double matrix = (double)((blocks + 255) / 256) * nk * Y2_SPLIT_KTILE_CYCLES / Y2_SPLIT_GEMM_EFF;
    const double bytes = (v_bytes + u_bytes + m_bytes) * Y2_WINO_BYTE_CYCLES;
    return matrix > bytes ? matrix : bytes;
}

static inline double y2_split_cost(double gemm_cost, double transform_bytes)
{
    return gemm_cost + transform_bytes * Y2_WINO_BYTE_CYCLES + 2.0 * Y2_WINO_LAUNCH_CYCLES;
}

#endif
