/*
 * The stationary-Winograd rule: which shallow fp32 3x3 convolutions run as ONE fused F(2x2,3x3) kernel (y2_winos.hip) whose
 * transformed filters U = G g G^T stay in registers for the whole launch -- no V or M array in memory, unlike the three-pass
 * path of y2_wino_rule.h, whose transform passes cost the shallow layers more than its GEMM saves.  Host arithmetic only.
 *
 * The form with 32 input channels: U of 32 channels x 64 filters is 16 x 32 x 64 floats = 128 KiB, the registers of the
 * eight waves of one workgroup per CU.  A workgroup walks output patches of 8 x 16 pixels (32 Winograd tiles, one MFMA row
 * tile); the rule asks for at least Y2_WINOS_MIN_PATCHES of them, the work of conv_c32_f32's 512 tiles of 16 x 16, so that
 * every CU walks four patches or more and the filter load and the last partial round are a small share.
 *
 * The margin is the project's 10 %: the form is taken because yolo.cfg layer 2 at 608x608 batch 32 measured more than that
 * below conv_c32_f32 (profiles/winos_608b32.txt, section 2).
 */
#ifndef Y2_WINOS_RULE_H
#define Y2_WINOS_RULE_H

#include <stddef.h>

#define Y2_WINOS_MIN_PATCHES 1024L
#define Y2_WINOS_PATCH_H 8
#define Y2_WINOS_PATCH_W 16

/* the shapes the 32-channel form takes */
static inline int y2_winos_shape_ok(int size, int stride, int pad, int c, int n, int h, int w, int out_h, int out_w, int pool,
                                    int x_f16, int y_f16, int x_halo, int x_nchw, int ldx)
{
    (void)pool;                 /* H and W are even: a Winograd tile is a pooling window */
    if (x_f16 || y_f16 || x_halo || x_nchw) return 0;
    if (size != 3 || stride != 1 || pad != 1 || out_h != h || out_w != w) return 0;
    if (c != 32 || n < 4 || n > 64 || n % 4 != 0 || ldx % 4 != 0) return 0;
    if (h <= 0 || w <= 0 || h % Y2_WINOS_PATCH_H != 0 || w % Y2_WINOS_PATCH_W != 0) return 0;
    return 1;
}

static inline long y2_winos_patches(int batch, int h, int w) { return (long)batch * (h / Y2_WINOS_PATCH_H) * (w / Y2_WINOS_PATCH_W); }

static inline int y2_winos_wins(long patches) { return patches >= Y2_WINOS_MIN_PATCHES; }

/* U in the kernel's register order.  Wave (filter tile fq = co / 32, component row i) keeps, per lane (li = co % 32,
 * lh = (ci % 8) / 4), sixteen 16-byte registers kk = 4 j + ci / 8 holding channels ci % 4 = 0..3:
 *     [fq][i][kk][lane = 32 lh + li][ci % 4]
 * so a register is one coalesced 16-byte load.  Filters past n inside the last tile are zero. */
static inline size_t y2_winos_u_floats(int n) { return (size_t)((n + 31) / 32) * 4 * 16 * 64 * 4; }
static inline size_t y2_winos_u_index(int co, int ci, int i, int j)
{
    const size_t fq = (size_t)(co / 32), lane = (size_t)(32 * ((ci % 8) / 4) + co % 32), kk = (size_t)(4 * j + ci / 8);
    return (((fq * 4 + (size_t)i) * 16 + kk) * 64 + lane) * 4 + (size_t)(ci % 4);
}

#endif
