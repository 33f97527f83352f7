/*
 * The direct split rule: which fp32 3x3 convolutions run as ONE direct kernel on the bf16 matrix cores (y2_conv_split.hip),
 * both operands split three ways into bf16 planes (the split and the six products kept: y2_split_rule.h) -- no transform
 * pass and no V or M array in memory; the input crosses memory once, the output once.  Host arithmetic only, C.
 *
 * The tile.  256 positions x BN filters (BN = 128 for n <= 128, else 256), K-tile = 16 channels, eight waves of 128
 * positions x BN / 4 filters.  Without a fused pool the positions are linear over image rows padded to W + 2 -- the pad sits
 * at the end of a row and is the left halo of the next one -- with one zero row between images:
 *     position = (image * (H + 1) + y) * (W + 2) + x
 * so tap (ky, kx) of any position is the position ((ky - 1) (W + 2) + (kx - 1)) further on, and a tile of 256 positions reads
 * a patch of 256 + 2 (W + 3) of them.  The outputs at pad positions (x >= W or y == H) are computed and dropped.
 * With the fused 2x2 maxpool the tile is four units of 32 columns x 2 image rows (an even row and the odd row below it: two
 * streams of 32 positions); a unit keeps its own patch of 4 rows x 34 columns, and a pooling window is the same lane and
 * register of the two streams' accumulators and the neighbouring lane.
 *
 * The filters.  Reference layout [n][c][3][3], split once at weight upload into three bf16 planes, one contiguous run per
 * (filter tile, K-tile, tap) in the order the kernel streams them; inside a run [plane][k-half][filter % BN][8 channels] as in
 * y2_split_index.  Filters past n in the last tile are zero rows.
 *
 * The shapes.  3x3, stride 1, pad 1, fp32 in and out, NHWC without halo, c % 16 == 0, n % 4 == 0, ldx % 4 == 0; with the
 * fused pool H and W even.  The pooled form has the 128-wide filter tile only; more filters are further filter tiles, each
 * of which stages and splits its patch again.
 *
 * The cost, in the Winograd rule's units (CU cycles): matrix cycles on whole rounds of the tile over 256 CUs over the share
 * of the bf16 rate the kernel holds, or the bytes (input times the patch's halo factor, filters, output) at
 * Y2_WINO_BYTE_CYCLES, whichever is larger.  The form is taken when that is below the direct plan's cost by Y2_WINO_MARGIN,
 * the tiles fill at least one round, and ONE 128-wide filter tile covers all filters (n <= 128).
 *
 * Layers with more than 128 filters stay on the direct fp32 kernel.  This is deliberate: tests/test_gpu_configs.py asserts
 * that conv_mfma_f32_192x256x32_k3 runs in yolo.cfg at 608 batch 32 under exactly that name, which only the unpooled layer 8
 * carries (layer 10 is ...+maxpool2), so layer 8 has to keep it -- it measured 0.96 -> 0.53 ms in this form, about 0.4 ms per
 * step that stays there.  The pooled layer 10 measured 0.92 -> 0.79 ms as two filter tiles; with the measured efficiency the
 * model does not put it below the margin (profiles/conv_split_608b32.txt, section 2).
 */
#ifndef Y2_SPLITD_RULE_H
#define Y2_SPLITD_RULE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "y2_split_rule.h"

#define Y2_SPLITD_BM 256                 /* positions of a tile */
#define Y2_SPLITD_UNIT_W 32              /* pooled: columns of a unit */
#define Y2_SPLITD_UNIT_PITCH 34          /* pooled: columns of a unit's patch */
#define Y2_SPLITD_UNIT_POS (4 * Y2_SPLITD_UNIT_PITCH)
#define Y2_SPLITD_LDS_BYTES 163840       /* LDS of a CU */
/* matrix cycles of one (K-tile, tap) of a 256 x 128 tile: 24 MFMAs of 32 cycles on each of a SIMD's two waves */
#define Y2_SPLITD_STEP_CYCLES 1536.0
/* Share of the bf16 matrix rate the kernel holds, in the model's cycles (2.4 GHz; the kernel runs at about 2.1).  Set against the
 * measured per-layer table of yolo.cfg 608x608 batch 32 (profiles/conv_split_608b32.txt, section 2): 0.47 and 0.49 on the two
 * 152x152 layers the rule takes, 0.52 on the 256-wide tile (76x76, forced), 0.47 on the pooled two-tile form (76x76, forced). */
#define Y2_SPLITD_EFF 0.47

/* the filter tile: one tile for all filters up to 128, else 256 wide; forced (tests) by Y2_SPLITD_TILE=256x128 / 256x256.
 * The pooled form has the 128-wide tile only (its patch leaves no room for 256-wide filter buffers). */
static inline int y2_splitd_bn(int n, int pool)
{
    const char *f = getenv("Y2_SPLITD_TILE");
    int bm = 0, bn = 0;
    if (pool) return 128;
    if (f && sscanf(f, "%dx%d", &bm, &bn) == 2 && bm == Y2_SPLITD_BM && (bn == 128 || bn == 256)) return bn;
    return n <= 128 ? 128 : 256;
}

static inline int y2_splitd_shape_ok(int size, int stride, int pad, int c, int n, int h, int w, int out_h, int out_w, int pool,
                                     int x_f16, int y_f16, int x_halo, int x_nchw, int ldx)
{
    if (x_f16 || y_f16 || x_halo || x_nchw) return 0;
    if (size != 3 || stride != 1 || pad != 1 || out_h != h || out_w != w) return 0;
    if (c <= 0 || c % Y2_SPLIT_BK != 0 || n <= 0 || n % 4 != 0 || ldx % 4 != 0) return 0;
    if (pool && ((h | w) & 1)) return 0;
    return 1;
}

/* positions the persistent grid walks, and the patch positions of one tile */
static inline long y2_splitd_positions(int batch, int h, int w, int pool)
{
    if (pool) return (long)batch * (h / 2) * ((w + Y2_SPLITD_UNIT_W - 1) / Y2_SPLITD_UNIT_W) * (2 * Y2_SPLITD_UNIT_W);
    return (long)batch * (h + 1) * (w + 2);
}
static inline int y2_splitd_patch_positions(int w, int pool) { return pool ? 4 * Y2_SPLITD_UNIT_POS : Y2_SPLITD_BM + 2 * (w + 3); }
static inline long y2_splitd_tiles_m(int batch, int h, int w, int pool)
{
    return (y2_splitd_positions(batch, h, w, pool) + Y2_SPLITD_BM - 1) / Y2_SPLITD_BM;
}

/* LDS: two patch buffers (three planes of 16 channels), three filter buffers, the epilogue constants of a filter tile */
static inline size_t y2_splitd_lds_bytes(int w, int pool, int bn)
{
    return (size_t)2 * y2_splitd_patch_positions(w, pool) * 96 + (size_t)3 * 96 * bn + (size_t)bn * 20;
}

/* bf16 values of the filter slot, and the index of plane p of filter co, channel ci, tap (= 3 ky + kx) */
static inline size_t y2_splitd_u_elems(int n, int c, int bn) { return (size_t)((n + bn - 1) / bn) * (size_t)(c / Y2_SPLIT_BK) * 9 * 48 * (size_t)bn; }
static inline size_t y2_splitd_u_index(int c, int bn, int co, int ci, int tap, int p)
{
    const size_t run = ((size_t)(co / bn) * (size_t)(c / Y2_SPLIT_BK) + (size_t)(ci / Y2_SPLIT_BK)) * 9 + (size_t)tap;
    return run * 48 * (size_t)bn + ((size_t)(p * 2 + (ci % Y2_SPLIT_BK) / 8) * (size_t)bn + (size_t)(co % bn)) * 8 + (size_t)(ci % 8);
}

/* the filters of a direct split layer from the reference layout [n][c][3][3] */
static inline void y2_splitd_pack_u(uint16_t *up, const float *weights, int n, int c, int bn)
{
    int co, ci, tap;
    memset(up, 0, y2_splitd_u_elems(n, c, bn) * 2);
    for (co = 0; co < n; ++co)
        for (ci = 0; ci < c; ++ci)
            for (tap = 0; tap < 9; ++tap) {
                uint16_t h, m, l;
                y2_split3(weights[((size_t)co * c + ci) * 9 + tap], &h, &m, &l);
                up[y2_splitd_u_index(c, bn, co, ci, tap, 0)] = h;
                up[y2_splitd_u_index(c, bn, co, ci, tap, 1)] = m;
                up[y2_splitd_u_index(c, bn, co, ci, tap, 2)] = l;
            }
}

/* the two costs of `tiles` tiles of nk K-tiles (nine taps each) on 256 CUs; the larger is the layer's */
static inline double y2_splitd_matrix_cost(long tiles, int nk, int bn)
{
    return (double)((tiles + 255) / 256) * nk * 9.0 * Y2_SPLITD_STEP_CYCLES * (bn / 128) / Y2_SPLITD_EFF;
}
static inline double y2_splitd_byte_cost(double x_bytes, double halo, double u_bytes, double y_bytes)
{
    return (x_bytes * halo + u_bytes + y_bytes) * Y2_WINO_BYTE_CYCLES;
}

/* patch positions fetched per position computed */
static inline double y2_splitd_halo(int w, int pool) { return (double)y2_splitd_patch_positions(w, pool) / Y2_SPLITD_BM; }

#endif
