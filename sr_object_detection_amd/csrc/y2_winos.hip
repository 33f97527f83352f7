// "Winograd, stationary": F(2x2,3x3) for the shallow fp32 stride-1 3x3 convolutions as ONE fused kernel whose transformed
// filters U = G g G^T stay in registers for the whole launch (the rule: include/y2_winos_rule.h).  No V or M array exists in
// memory: the input crosses memory once (plus the patch halo), the output once.
//
//     Y = A^T [ sum_c U .* V ] A,    U = G g G^T (at weight upload, y2_arena.c),    V = B^T d B
//
//         | 1  0 -1  0 |            | 1  1  1  0 |
//   B^T = | 0  1  1  0 |      A^T = | 0  1 -1 -1 |
//         | 0 -1  1  0 |
//         | 0  1  0 -1 |
//
// The 32-channel form (c == 32, n <= 64: yolo.cfg layer 2, 304x304 32 -> 64 + pool at 608x608), one 512-thread workgroup per
// CU on a persistent grid over 8 x 16-pixel output patches (32 tiles of 2x2 = one MFMA row tile, in the order of ws_tile):
//   * wave (filter tile fq, component row i) keeps U[i][j = 0..3][filter li][channel 8 g + 4 lh + s] as sixteen 16-byte
//     registers, loaded once per kernel (layout: y2_winos_u_index);
//   * the raw NHWC patch of the NEXT block (10 x 18 pixels at a 144-byte pitch, bank-skewed: ws_tile) is fetched into registers during the current
//     block's MFMAs and written to the other LDS buffer afterwards, as in conv_c32_f32_kernel;
//   * per group g of 8 channels a lane reads the two patch rows that row i of B^T combines at its tile's four columns
//     (eight ds_read_b128), forms (B^T d)[i][0..3] and from it V[i][0..3], and issues 16 v_mfma_f32_32x32x2_f32 into the four
//     independent accumulators M[i][0..3]: 64 MFMAs per block and wave where the direct kernel issues 144;
//   * after the channel loop S[i][b] = (M A)[i][b] in registers, the four row-waves of a filter tile exchange S through LDS,
//     and wave i finishes tile row ty = i: Y[a][b] = sum_i A^T[a][i] S[i][b], a lane owning four filters of one tile;
//   * the epilogue is the shared epilogue() / pool_pick() arithmetic (a tile is a pooling window; negative batch-norm scales
//     pick the window minimum); outputs leave as 16-byte stores, or dword by dword when ldy or y is not 16-byte aligned.
// B^T and A^T only add and subtract and U of a small-integer filter is a multiple of 1/4: exact on integer data like every
// tile here.  Compiled with -ffp-contract=off like y2_conv.hip: the epilogue mirrors the reference step by step.
#include "y2_conv_shared.hpp"
#include "y2_winos_rule.h"
#include <string.h>

namespace {

constexpr int WS_PW = 18, WS_PH = 10, WS_PIX_B = 144, WS_ROW_B = WS_PW * WS_PIX_B, WS_BUF_B = WS_PH * WS_ROW_B;
constexpr int WS_NCH = WS_PH * WS_PW * 8;            // 16-byte chunks of one patch
constexpr int WS_NP = (WS_NCH + 511) / 512;          // staging passes
constexpr int WS_EX_P = 36;                          // exchange: floats per tile row (32 filters + 4: 16-byte aligned rows)
constexpr int WS_EX_COMP = 32 * WS_EX_P;             // one S[i][b] of a filter tile: [32 tiles][WS_EX_P]
constexpr int WS_EX_FQ = 8 * WS_EX_COMP;             // the eight (i, b) of a filter tile
constexpr int WS_CONST_B = 64 * (3 * 4 + 8);         // mean, scale, bias, rinv of up to 64 filters
constexpr size_t WS_LDS = (size_t)2 * WS_BUF_B + (size_t)2 * WS_EX_FQ * 4 + WS_CONST_B;

// Which tile of the block MFMA row li carries.  A ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27} and
// {4-11, 16-19, 28-31} of each half wave -- and a tile's patch address is 16 ty + 8 tx banks (mod 64) from the block's: with
// tile rows 0, 1 in the first group and 2, 3 in the second, and every other pair of patch columns 16 bytes further on
// (s_lds below), the sixteen lanes of a group read sixteen distinct 16-byte slots.  Row-major tiles would conflict four ways.
__device__ __forceinline__ int ws_tile(int li)
{
    const int q = li >> 2;
    return 16 * (__builtin_popcount(q) & 1) + ((q >> 1) << 2) + (li & 3);
}

__device__ __forceinline__ f32x4 flip(f32x4 v, unsigned neg)
{
    u32x4 b = __builtin_bit_cast(u32x4, v);
    b ^= neg;
    return __builtin_bit_cast(f32x4, b);
}

template <bool POOL, bool FAST>
__global__ __launch_bounds__(512, 2) void conv_winos_c32_kernel(ConvK a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
    const int t = threadIdx.x, lane = t & 63, li = lane & 31, lh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int fq = wv & 1, wi = wv >> 1;
    const bool BN_ = FAST ? true : (bool)a.bn;
    const int ACT_ = FAST ? (int)Y2H_ACT_LEAKY : a.act;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void *)a.w, 0, a.wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void *)a.y, 0, a.ybytes, 0x00020000);

    float *ex = (float *)(ws_smem + 2 * WS_BUF_B);
    float *c_mean = ex + 2 * WS_EX_FQ, *c_scale = c_mean + 64, *c_bias = c_scale + 64;
    double *c_rinv = (double *)(c_bias + 64);
    if (t < 64) {
        float mean = 0.f, scale = 1.f, bias = 0.f;
        double rinv = 1.0;
        if (t < a.Cout) {
            bias = a.bias[t];
            if (BN_) { mean = a.mean[t]; rinv = a.rinv[t]; scale = a.scale[t]; }
        }
        c_mean[t] = mean; c_scale[t] = scale; c_bias[t] = bias; c_rinv[t] = rinv;
    }

    f32x4 bu[16];                                    // [4 j + g]: U[wi][j][32 fq + li][8 g + 4 lh .. + 3]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const unsigned off = 32 * fq < a.Cout ? (unsigned)((((fq * 4 + wi) * 16 + kk) * 64 + lane) * 16) : a.wbytes;
        bu[kk] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }

    const int ldxB = a.ldx * 4;
    int s_lds[WS_NP], s_rel[WS_NP], s_yx[WS_NP];
#pragma unroll
    for (int p = 0; p < WS_NP; ++p) {
        const int q = t + 512 * p;
        const int pixel = q >> 3, part = q & 7;
        const int py = pixel / WS_PW, px = pixel - py * WS_PW;
        s_lds[p] = py * WS_ROW_B + px * WS_PIX_B + ((px >> 2) & 1) * 16 + part * 16;
        s_rel[p] = ((py - 1) * a.W + (px - 1)) * ldxB + part * 16;
        s_yx[p] = q < WS_NCH ? (py << 8) | px : -1;
    }
    const int blocks_x = a.W >> 4, bpi = (a.H >> 3) * blocks_x;
    const int nblocks = a.batch * bpi;
    u32x4 sreg[WS_NP];
    auto load_patch = [&](int blk) {
        const int n = blk / bpi, rem = blk - n * bpi;
        const int oy0 = (rem / blocks_x) << 3, ox0 = (rem - (rem / blocks_x) * blocks_x) << 4;
        const unsigned base = (unsigned)((n * a.H + oy0) * a.W + ox0) * (unsigned)ldxB;
#pragma unroll
        for (int p = 0; p < WS_NP; ++p) {
            const int iy = oy0 - 1 + (s_yx[p] >> 8), ix = ox0 - 1 + (s_yx[p] & 255);
            const bool ok = s_yx[p] >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            sreg[p] = __builtin_amdgcn_raw_buffer_load_b128(xr, ok ? base + (unsigned)s_rel[p] : a.xbytes, 0, 0);
        }
    };
    auto store_patch = [&](int buf) {
#pragma unroll
        for (int p = 0; p < WS_NP; ++p)
            if (s_yx[p] >= 0) *(u32x4 *)(ws_smem + buf * WS_BUF_B + s_lds[p]) = sreg[p];
    };

    // row i of B^T: (B^T d)[i] = d[ra] + d[rb], the second term negated unless i == 1
    const int ra = wi == 0 ? 0 : wi == 2 ? 2 : 1;
    const int rb = wi == 0 ? 2 : wi == 1 ? 2 : wi == 2 ? 1 : 3;
    const unsigned neg = wi == 1 ? 0u : 0x80000000u;
    // MFMA row li = tile ws_tile(li) = (ty = T >> 3, tx = T & 7): its 4x4 input patch starts at patch pixel (2 ty, 2 tx).
    // a_off[0]: patch columns 2 tx, + 1; a_off[1]: columns 2 tx + 2, + 3 (the column skew differs)
    const int aty = ws_tile(li) >> 3, atx = ws_tile(li) & 7;
    const int a_off0 = 2 * aty * WS_ROW_B + 2 * atx * WS_PIX_B + ((atx >> 1) & 1) * 16 + lh * 16;
    const int a_off1 = 2 * aty * WS_ROW_B + (2 * atx + 2) * WS_PIX_B + (((atx + 1) >> 1) & 1) * 16 + lh * 16;
    // the finishing side: tile (ty = wi, tx = lane >> 3), filters cbase .. cbase + 3
    const int otx = lane >> 3, cq = 32 * fq + (lane & 7) * 4;
    const bool fok = cq < a.Cout;
    const float *exr = ex + fq * WS_EX_FQ + (wi * 8 + otx) * WS_EX_P + (lane & 7) * 4;
    float *exw = ex + fq * WS_EX_FQ + (wi * 2) * WS_EX_COMP + li;
    float *exw_even = exw + 16 * lh * WS_EX_P, *exw_odd = exw + 16 * (1 - lh) * WS_EX_P;
    const int Hp = a.H >> 1, Wp = a.W >> 1;

    int blk = blockIdx.x, cur = 0;
    if (blk < nblocks) { load_patch(blk); store_patch(0); }
    __syncthreads();
    for (; blk < nblocks; blk += gridDim.x, cur ^= 1) {
        const int next = blk + gridDim.x;
        if (next < nblocks) load_patch(next);
        const unsigned char *ap0 = ws_smem + cur * WS_BUF_B + a_off0, *ap1 = ws_smem + cur * WS_BUF_B + a_off1;
        f32x16 M[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) M[j][r] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 tc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned char *ap = c < 2 ? ap0 + c * WS_PIX_B : ap1 + (c - 2) * WS_PIX_B;
                const f32x4 da = *(const f32x4 *)(ap + ra * WS_ROW_B + g * 32);
                const f32x4 db = *(const f32x4 *)(ap + rb * WS_ROW_B + g * 32);
                tc[c] = da + flip(db, neg);
            }
            f32x4 v[4];
            v[0] = tc[0] - tc[2]; v[1] = tc[1] + tc[2]; v[2] = tc[2] - tc[1]; v[3] = tc[1] - tc[3];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    M[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][s4], bu[4 * j + g][s4], M[j], 0, 0, 0);
        }
        // S = M A per row: S[i][0] = (M0 + M1) + M2, S[i][1] = (M1 - M2) - M3
        const f32x16 S0 = (M[0] + M[1]) + M[2], S1 = (M[1] - M[2]) - M[3];
        __syncthreads();                                       // every wave has read the previous block's exchange
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // MFMA row (r & 3) + 8 (r >> 2) + 4 lh = tile ws_tile(row): 16 (parity(r >> 2) ^ lh) + 4 (r >> 2) + (r & 3)
            float *e = ((__builtin_popcount(r >> 2) & 1) ? exw_odd : exw_even) + (4 * (r >> 2) + (r & 3)) * WS_EX_P;
            e[0] = S0[r];
            e[WS_EX_COMP] = S1[r];
        }
        if (next < nblocks) store_patch(cur ^ 1);
        __syncthreads();

        // Y = A^T S: Y[0][b] = (S[0][b] + S[1][b]) + S[2][b], Y[1][b] = (S[1][b] - S[2][b]) - S[3][b]
        f32x4 Y[2][2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const f32x4 s0 = *(const f32x4 *)(exr + (0 + b) * WS_EX_COMP), s1 = *(const f32x4 *)(exr + (2 + b) * WS_EX_COMP);
            const f32x4 s2 = *(const f32x4 *)(exr + (4 + b) * WS_EX_COMP), s3 = *(const f32x4 *)(exr + (6 + b) * WS_EX_COMP);
            Y[0][b] = (s0 + s1) + s2;
            Y[1][b] = (s1 - s2) - s3;
        }
        const f32x4 mean = *(const f32x4 *)(c_mean + cq), scale = *(const f32x4 *)(c_scale + cq), bias = *(const f32x4 *)(c_bias + cq);
        double rinv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) rinv[q] = c_rinv[cq + q];
        const int n = blk / bpi, rem = blk - n * bpi;
        const int oy0 = (rem / blocks_x) << 3, ox0 = (rem - (rem / blocks_x) * blocks_x) << 4;
        if (POOL) {
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                o[q] = epilogue(pool_pick(Y[0][0][q], Y[0][1][q], Y[1][0][q], Y[1][1][q], !BN_ || scale[q] >= 0.f),
                                BN_, mean[q], rinv[q], scale[q], bias[q], ACT_);
            const unsigned prow = (unsigned)((n * Hp + (oy0 >> 1) + wi) * Wp + (ox0 >> 1) + otx);
            const unsigned idx = prow * (unsigned)a.ldy + (unsigned)cq;
            if (a.vec_store) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, fok ? idx * 4u : 0xffffffffu, 0, 0);
            else if (fok) {
#pragma unroll
                for (int q = 0; q < 4; ++q) a.y[(size_t)idx + q] = o[q];
            }
        } else {
#pragma unroll
            for (int ya = 0; ya < 2; ++ya)
#pragma unroll
                for (int xb = 0; xb < 2; ++xb) {
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = epilogue(Y[ya][xb][q], BN_, mean[q], rinv[q], scale[q], bias[q], ACT_);
                    const unsigned prow = (unsigned)((n * a.H + oy0 + 2 * wi + ya) * a.W + ox0 + 2 * otx + xb);
                    const unsigned idx = prow * (unsigned)a.ldy + (unsigned)cq;
                    if (a.vec_store) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, fok ? idx * 4u : 0xffffffffu, 0, 0);
                    else if (fok) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) a.y[(size_t)idx + q] = o[q];
                    }
                }
        }
    }
}

}  // namespace

// Host arithmetic only.  Y2_WINOS=0: never; Y2_WINOS=1: every eligible descriptor (tests); otherwise the rule's min-work
// threshold, which no other switch lowers.  A measured or forced tile choice keeps the layer on the tile it names.
extern "C" int y2h_winos_plan(const y2h_conv *d, y2h_winos *out)
{
    if (!d || !out) return Y2H_EINVAL;
    memset(out, 0, sizeof *out);
    int mode = -1;
    if (const char *f = getenv("Y2_WINOS")) mode = atoi(f) != 0 ? 1 : 0;
    if (!y2_winos_shape_ok(d->size, d->stride, d->pad, d->c, d->n, d->h, d->w, d->out_h, d->out_w, d->fuse_maxpool2, d->x_f16, d->y_f16,
                           d->x_halo, d->x_nchw, d->ldx)) return Y2H_OK;
    if (d->ldy < d->n || d->tile_bm || d->ksplit > 1 || getenv("Y2_CONV_TILE")) return Y2H_OK;
    if (((uintptr_t)d->x | (uintptr_t)d->w_packed) % 16 != 0 || !d->w_packed) return Y2H_OK;
    const double xbytes = (double)d->batch * d->h * d->w * d->ldx * 4.0;
    const double ybytes = (double)d->batch * d->h * d->w * (d->fuse_maxpool2 ? 0.25 : 1.0) * d->ldy * 4.0;
    if (xbytes >= 4294967000.0 || ybytes >= 4294967000.0) return Y2H_OK;               // 32-bit buffer offsets
    out->eligible = 1;
    out->form = 32;
    out->patches = y2_winos_patches(d->batch, d->h, d->w);
    out->u_bytes = y2_winos_u_floats(d->n) * sizeof(float);
    out->take = mode >= 0 ? mode : y2_winos_wins(out->patches);
    return Y2H_OK;
}

static unsigned long g_winos_launches = 0;
extern "C" unsigned long y2h_winos_launches(void) { return g_winos_launches; }

extern "C" int y2h_conv_winos_forward(const y2h_conv *d, y2h_stream s)
{
    if (!conv_args_ok(d) || !d->w_packed) return Y2H_EINVAL;
    y2h_winos w;
    if (y2h_winos_plan(d, &w) != Y2H_OK || !w.take || w.form != 32) return Y2H_EINVAL;
    ConvK a;
    memset(&a, 0, sizeof a);
    a.x = d->x; a.y = d->y; a.w = d->w_packed;
    a.mean = d->mean; a.rinv = d->rinv; a.scale = d->scale; a.bias = d->bias;
    a.H = d->h; a.W = d->w; a.Cin = d->c; a.ldx = d->ldx; a.Cout = d->n; a.ldy = d->ldy;
    a.K = 9 * d->c;
    a.bn = d->batch_normalize; a.act = d->activation;
    a.size = 3; a.stride = 1; a.pad = 1; a.out_h = d->out_h; a.out_w = d->out_w; a.batch = d->batch;
    a.pool = d->fuse_maxpool2 ? 1 : 0;
    a.npix = d->batch * d->h * d->w;
    a.xbytes = (unsigned)((size_t)d->batch * d->h * d->w * d->ldx * 4);
    a.wbytes = (unsigned)w.u_bytes;
    a.ybytes = (unsigned)((size_t)(a.pool ? a.npix / 4 : a.npix) * d->ldy * 4);
    a.vec_store = d->ldy % 4 == 0 && (uintptr_t)d->y % 16 == 0;
    const bool fast = d->batch_normalize && d->activation == Y2H_ACT_LEAKY;
    void (*fn)(ConvK) = a.pool ? (fast ? conv_winos_c32_kernel<true, true> : conv_winos_c32_kernel<true, false>)
                               : (fast ? conv_winos_c32_kernel<false, true> : conv_winos_c32_kernel<false, false>);
    Y2H_CHECK(y2h_lds_limit((const void *)fn, WS_LDS));
    long grid = w.patches < 256 ? w.patches : 256;
    if (const char *g = getenv("Y2_CONV_GRID")) { if (atol(g) > 0 && atol(g) < grid) grid = atol(g); }
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(512), WS_LDS, S(s), a);
    Y2H_LAUNCH_CHECK();
    ++g_winos_launches;
    return Y2H_OK;
}
