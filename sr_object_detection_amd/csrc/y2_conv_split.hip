// "Direct, split": the fp32 stride-1 3x3 convolution as ONE implicit-GEMM kernel on the bf16 matrix cores, both operands
// split three ways into bf16 planes a = h + m + l (include/y2_split_rule.h: the split and the six products kept; the rule,
// the position order and the filter layout: include/y2_splitd_rule.h).  No V or M array, no transform pass: the input
// crosses memory once (plus the patch halo, which L2 serves), the output once.
//
//  * A persistent walk, one workgroup of eight waves per CU, over tiles of 256 positions x BN filters (BN = 128 or 256,
//    filter tile fastest); waves 2 (positions) x 4 (filters), each 128 positions x BN / 4 filters = 4 x BN / 128 accumulator
//    tiles of 32x32.  K-tile = 16 channels = one v_mfma_f32_32x32x16_bf16 step; the filters are the MFMA's row operand, so a
//    lane holds four consecutive filters of one position in four consecutive registers.
//  * Every input value is fetched and split ONCE per tile and K-tile: a thread stages 8 channels of one patch position (two
//    16-byte buffer loads, split3_x4 twice, three 16-byte LDS stores) into the patch [plane][k-half][position][8 channels].
//    Padding, the zero row between images and everything outside the image are out-of-range buffer loads (zeros).  All nine
//    taps read that patch by an address shift: without the pool positions are linear over rows padded to W + 2, so tap
//    (ky, kx) of a row tile of 32 positions is the same 512 contiguous bytes (ky (W + 2) + kx) * 16 bytes further on; with the
//    fused pool a unit of 32 columns x 2 rows has its own patch of 4 rows x 34 columns and the shift is (34 ky + kx) * 16.
//    Either way a fragment read is 512 contiguous bytes: no bank conflict, no swizzle.
//  * The patch of K-tile k + 1 is loaded into registers during the first taps of K-tile k (one pass of 512 (position,
//    k-half) items per tap: three passes, two beside the 256-wide filter buffers), split behind that tap's MFMAs and written
//    to the other patch buffer.
//  * The filters stream: one contiguous run per (filter tile, K-tile, tap), 96 BN bytes already in LDS order, by lane-linear
//    16-byte LDS-DMA pieces from L2 into three buffers, two taps ahead.  A step = one tap: wait for the own pieces of this
//    step (counted vmcnt: the next step's stay in flight) and the own LDS traffic, barrier, issue the pieces of the step
//    after next into the buffer every wave has just left, read the fragments, 24 or 48 MFMAs.
//  * The six products are issued smallest first -- l h', h l', m m', m h', h m', h h' -- term by term across the
//    accumulator tiles, as y2_wino_split.hip does.
//  * Epilogue: the shared epilogue() step by step, constants of the filter tile in LDS; 16-byte buffer stores where ldy and
//    y allow, dword stores otherwise; positions that are padding are dropped.  Fused pool: the window is registers of the
//    even-row and the odd-row accumulator tile of this lane and of lane ^ 1; pool_pick, then ONE epilogue per window.
//
// Compiled with -ffp-contract=off like the other conv units.
#include "y2_conv_shared.hpp"
#include "y2_splitd_rule.h"
#include "y2_split_dev.hpp"
#include <string.h>

typedef __attribute__((address_space(3))) void lds_void_d;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

struct SplitDK {
    const float *x;
    const unsigned short *u;
    float *y;
    const float *mean, *scale, *bias;
    const double *rinv;
    unsigned xbytes, ubytes, ybytes;
    int H, W, Wp, batch, ldx, ldy, N, nk;
    int np;                    // positions (pooled: units)
    int pp;                    // patch positions of a tile
    int ux;                    // pooled: units per row pair
    int tiles_n, ntiles;
    int bn, act, vec_store;
};

constexpr unsigned SD_NONE = 0xffffffffu;

template <int BN, bool POOL, bool FAST>
__global__ __launch_bounds__(512, 1) void conv_splitd_kernel(SplitDK a)
{
    static_assert(BN == 128 || (BN == 256 && !POOL), "the pooled form has one filter tile of 128");
    constexpr int NJ = BN / 128;                     // 32-filter accumulator tiles per wave
    constexpr int RUN_B = 96 * BN;                   // one (filter tile, K-tile, tap) of filters
    constexpr int FPL_B = 32 * BN, FHALF_B = 16 * BN;
    constexpr int PIECES = BN == 256 ? 3 : 2;        // LDS-DMA pieces per wave and step
    constexpr int NPASS = BN == 256 ? 2 : 3;         // staging passes of 512 items: 2 x patch positions fit (y2h_conv_splitd_plan)
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];

    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, lh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wv >> 2, wn = wv & 3;
    const bool BN_ = FAST ? true : (bool)a.bn;
    const int ACT_ = FAST ? (int)Y2H_ACT_LEAKY : a.act;
    const int HALF_B = a.pp * 16, PLANE_B = 2 * HALF_B, PATCH_B = 3 * PLANE_B;
    const int pitch = POOL ? Y2_SPLITD_UNIT_PITCH : a.Wp;
    unsigned char *fbuf = sd_smem + 2 * PATCH_B;
    float *c_mean = (float *)(fbuf + 3 * RUN_B), *c_scale = c_mean + BN, *c_bias = c_scale + BN;
    double *c_rinv = (double *)(c_bias + BN);

    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, a.xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ur = __builtin_amdgcn_make_buffer_rsrc((void *)a.u, 0, a.ubytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void *)a.y, 0, a.ybytes, 0x00020000);

    auto load_consts = [&](int tn) {
        if (t < BN) {
            const int f = tn * BN + t;
            float mean = 0.f, scale = 1.f, bias = 0.f;
            double rinv = 1.0;
            if (f < a.N) {
                bias = a.bias[f];
                if (BN_) { mean = a.mean[f]; rinv = a.rinv[f]; scale = a.scale[f]; }
            }
            c_mean[t] = mean; c_scale[t] = scale; c_bias[t] = bias; c_rinv[t] = rinv;
        }
    };

    // ---- patch staging: pass p of this thread is item t + 512 p = (patch position q, k-half) ----
    unsigned s_off[NPASS];                           // byte offset of the item's 8 channels of K-tile 0 in x, or SD_NONE
    auto patch_addr = [&](int tm) {                  // tm < 0: nothing follows, every item reads zero
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int item = t + 512 * p, q = item >> 1;
            bool ok = tm >= 0 && q < a.pp;
            int n, y, x;
            if (POOL) {
                const int u = q / Y2_SPLITD_UNIT_POS, rem = q - u * Y2_SPLITD_UNIT_POS;
                const int r = rem / Y2_SPLITD_UNIT_PITCH, ci = rem - r * Y2_SPLITD_UNIT_PITCH;
                const int U = (tm < 0 ? 0 : tm) * 4 + u;
                ok = ok && U < a.np;
                const int pr = U / a.ux, xs = U - pr * a.ux;          // row pair (over all images), unit column
                const int Hp = a.H >> 1;
                n = pr / Hp;
                y = 2 * (pr - n * Hp) - 1 + r;
                x = 32 * xs - 1 + ci;
                ok = ok && y >= 0 && y < a.H && x >= 0 && x < a.W;
            } else {
                const int P = (tm < 0 ? 0 : tm) * Y2_SPLITD_BM - a.Wp - 1 + q;
                ok = ok && P >= 0 && P < a.np;
                const int Pc = P < 0 ? 0 : P;
                const int r = Pc / a.Wp;
                x = Pc - r * a.Wp;
                n = r / (a.H + 1);
                y = r - n * (a.H + 1);
                ok = ok && x < a.W && y < a.H;
            }
            s_off[p] = ok ? (unsigned)((n * a.H + y) * a.W + x) * (unsigned)(a.ldx * 4) + (unsigned)(item & 1) * 32u : SD_NONE;
        }
    };
    auto patch_load = [&](int p, unsigned kadd, u32x4 &r0, u32x4 &r1) {
        const unsigned o = s_off[p] == SD_NONE ? a.xbytes : s_off[p] + kadd;       // a.xbytes (+ 16): out of range, reads zero
        r0 = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
        r1 = __builtin_amdgcn_raw_buffer_load_b128(xr, o + 16u, 0, 0);
    };
    auto patch_store = [&](int p, unsigned char *buf, const u32x4 r0, const u32x4 r1) {
        const int item = t + 512 * p, q = item >> 1;
        if (q >= a.pp) return;
        u16x4 h0, m0, l0, h1, m1, l1;
        split3_x4(__builtin_bit_cast(f32x4, r0), h0, m0, l0);
        split3_x4(__builtin_bit_cast(f32x4, r1), h1, m1, l1);
        unsigned char *at = buf + (item & 1) * HALF_B + q * 16;
        *(u16x8 *)at = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        *(u16x8 *)(at + PLANE_B) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
        *(u16x8 *)(at + 2 * PLANE_B) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    // ---- filter streaming: the run at byte offset `off` of u into filter buffer b ----
    auto filter_dma = [&](unsigned off, int b) {
        unsigned char *dst = fbuf + b * RUN_B;
        if (BN == 256) {
#pragma unroll
            for (int p = 0; p < 3; ++p)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, (lds_void_d *)(dst + p * 8192 + wv * 1024), 16, off + p * 8192u + (unsigned)t * 16u, 0, 0, 0);
        } else {
            // 12 KB: piece 0 of every wave covers the first 8 KB; the last 4 KB come from waves 0-3, and once more -- the same
            // bytes to the same place -- from waves 4-7, so that every wave has the same count on its vmcnt
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, (lds_void_d *)(dst + wv * 1024), 16, off + (unsigned)t * 16u, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, (lds_void_d *)(dst + 8192 + (wv & 3) * 1024), 16,
                                                     off + 8192u + (unsigned)((wv & 3) * 1024 + lane * 16), 0, 0, 0);
        }
    };

    // fragment of a 32x32x16 operand: lane (r = lane & 31, h = lane >> 5) holds channels 8 h .. 8 h + 7 of row r
    const unsigned u_base = (unsigned)lh * FHALF_B + (unsigned)(wn * (BN / 4) + l31) * 16u;
    // row tile i of this wave starts v_row(i) positions behind the wave's first: a compile-time step either way
    const unsigned v_base = (unsigned)lh * (unsigned)HALF_B + (unsigned)((POOL ? wm * 2 * Y2_SPLITD_UNIT_POS : wm * 128) + l31) * 16u;
    auto v_row = [](int i) { return POOL ? (i >> 1) * Y2_SPLITD_UNIT_POS + (i & 1) * Y2_SPLITD_UNIT_PITCH : i * 32; };

    const unsigned KT_B = 9u * RUN_B;                // the nine runs of one K-tile
    long tile = blockIdx.x;
    int tm = (int)(tile / a.tiles_n), tn = (int)(tile - (long)tm * a.tiles_n);
    unsigned f_cur = (unsigned)(tn * a.nk) * KT_B;

    load_consts(tn);
    patch_addr(tm);
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        u32x4 r0, r1;
        patch_load(p, 0u, r0, r1);
        patch_store(p, sd_smem, r0, r1);
    }
    __builtin_amdgcn_sched_barrier(0);
    filter_dma(f_cur, 0);
    filter_dma(f_cur + RUN_B, 1);
    __builtin_amdgcn_sched_barrier(0);

    int pb = 0;
    for (;;) {
        const long ntile = tile + gridDim.x;
        const bool nlive = ntile < a.ntiles;
        const int ntm = nlive ? (int)(ntile / a.tiles_n) : -1, ntn = nlive ? (int)(ntile - (long)ntm * a.tiles_n) : 0;
        f32x16 acc[4][NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        for (int kt = 0; kt < a.nk; ++kt) {
            const bool last = kt + 1 == a.nk;
            if (last) patch_addr(ntm);
            const unsigned kadd = last ? 0u : (unsigned)(kt + 1) * 64u;
            // past the last tile the pieces still come (from run 0, into a buffer nobody reads): the counted waits stay right
            const unsigned f_next = last ? (unsigned)(ntn * a.nk) * KT_B : f_cur + KT_B;
            unsigned char *nbuf = sd_smem + (pb ^ 1) * PATCH_B;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                // this wave's pieces of this step are in (the next step's may be in flight), its LDS stores are done
                if (PIECES == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();        // every wave's are; nobody still reads the buffers written next
                __builtin_amdgcn_sched_barrier(0);
                u32x4 r0, r1;
                if (tap < NPASS) patch_load(tap, kadd, r0, r1);
                filter_dma(tap + 2 < 9 ? f_cur + (unsigned)(tap + 2) * RUN_B : f_next + (unsigned)(tap - 7) * RUN_B, (tap + 2) % 3);
                __builtin_amdgcn_sched_barrier(0);
                const unsigned char *fb = fbuf + (tap % 3) * RUN_B;
                // the tap's shift is added here, per tap: hoisted out of the K loop the 27 (tap, plane) addresses cost registers
                unsigned pa = v_base + (unsigned)(pb * PATCH_B);
                asm volatile("" : "+v"(pa));
                const unsigned char *pl = sd_smem + pa + (unsigned)((tap / 3) * pitch + tap % 3) * 16u;
                // (plane of the input, plane of the filters), smallest product first: l h', h l', m m', m h', h m', h h'.  The m
                // planes are read behind the first product, when the input's l plane is dead: 56 fragment registers, not 72
                bf16x8 pf[4][3], uf[NJ][3];
                auto read_u = [&](int p) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) uf[j][p] = *(const bf16x8 *)(fb + u_base + p * FPL_B + j * 512);
                };
                auto read_p = [&](int p) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) pf[i][p] = *(const bf16x8 *)(pl + p * PLANE_B + v_row(i) * 16);
                };
                auto product = [&](int pv, int pu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uf[j][pu], pf[i][pv], acc[i][j], 0, 0, 0);
                };
                read_u(0); read_p(2); read_p(0); read_u(2);
                product(2, 0);
                __builtin_amdgcn_sched_barrier(0);
                read_p(1); read_u(1);
                product(0, 2);
                product(1, 1);
                product(1, 0);
                product(0, 1);
                product(0, 0);
                if (tap < NPASS) patch_store(tap, nbuf, r0, r1);
            }
            f_cur = f_next;
            pb ^= 1;
        }

        // ---- epilogue: register 4 rg + e of a lane is filter 8 rg + 4 (lane >> 5) + e of the tile, position lane & 31 ----
        int pix[4];                                  // output pixel of accumulator row tile i (pooled: of unit i), or -1
        if (POOL) {
            const int Hp = a.H >> 1, Wq = a.W >> 1;
#pragma unroll
            for (int ul = 0; ul < 2; ++ul) {
                const int U = tm * 4 + 2 * wm + ul;
                const int pr = U / a.ux, xs = U - pr * a.ux;
                const int x = 32 * xs + l31;
                pix[ul] = (U < a.np && x < a.W && !(l31 & 1)) ? pr * Wq + (x >> 1) : -1;          // pr = image * Hp + yo
                (void)Hp;
            }
            pix[2] = pix[3] = -1;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int P = tm * Y2_SPLITD_BM + wm * 128 + i * 32 + l31;
                const int r = P / a.Wp, x = P - r * a.Wp;
                const int n = r / (a.H + 1), y = r - n * (a.H + 1);
                pix[i] = (P < a.np && x < a.W && y < a.H) ? (n * a.H + y) * a.W + x : -1;
            }
        }
        int fl0 = wn * (BN / 4) + lh * 4;            // computed here, per tile: the constants' addresses stay out of the K loop's registers
        asm volatile("" : "+v"(fl0));
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int fl = fl0 + j * 32 + rg * 8, f = tn * BN + fl;
                const bool fok = f < a.N;            // N % 4 == 0: the four filters are in or out together
                const f32x4 mean = *(const f32x4 *)(c_mean + fl), scale = *(const f32x4 *)(c_scale + fl), bias = *(const f32x4 *)(c_bias + fl);
                double rinv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) rinv[e] = c_rinv[fl + e];
#pragma unroll
                for (int i = 0; i < (POOL ? 2 : 4); ++i) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v;
                        if (POOL) {
                            const float e0 = acc[2 * i][j][4 * rg + e], o0 = acc[2 * i + 1][j][4 * rg + e];
                            v = pool_pick(e0, __shfl_xor(e0, 1), o0, __shfl_xor(o0, 1), !BN_ || scale[e] >= 0.f);
                        } else v = acc[i][j][4 * rg + e];
                        o[e] = epilogue(v, BN_, mean[e], rinv[e], scale[e], bias[e], ACT_);
                    }
                    const bool ok = pix[i] >= 0 && fok;
                    const unsigned idx = (unsigned)pix[i] * (unsigned)a.ldy + (unsigned)f;
                    if (a.vec_store) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), yr, ok ? idx * 4u : SD_NONE, 0, 0);
                    else if (ok) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) a.y[(size_t)idx + e] = o[e];
                    }
                    if (!FAST) __builtin_amdgcn_sched_barrier(0);      // one group's double arithmetic at a time: no scratch
                }
            }
        if (!nlive) break;
        if (a.tiles_n > 1) {                         // the next tile may be another filter tile: its constants
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            load_consts(ntn);
        }
        tile = ntile; tm = ntm; tn = ntn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

static unsigned long g_splitd_launches = 0;
extern "C" unsigned long y2h_conv_splitd_launches(void) { return g_splitd_launches; }

extern "C" int y2h_conv_splitd_forward(const y2h_conv *d, y2h_stream s)
{
    if (!conv_args_ok(d) || !d->w_packed) return Y2H_EINVAL;
    y2h_splitd w;
    if (y2h_conv_splitd_plan(d, &w) != Y2H_OK || !w.take) return Y2H_EINVAL;
    const int pool = d->fuse_maxpool2 ? 1 : 0;
    SplitDK a;
    memset(&a, 0, sizeof a);
    a.x = d->x; a.u = (const unsigned short *)d->w_packed; a.y = d->y;
    a.mean = d->mean; a.rinv = d->rinv; a.scale = d->scale; a.bias = d->bias;
    a.H = d->h; a.W = d->w; a.Wp = d->w + 2; a.batch = d->batch; a.ldx = d->ldx; a.ldy = d->ldy; a.N = d->n; a.nk = d->c / Y2_SPLIT_BK;
    a.bn = d->batch_normalize; a.act = d->activation;
    a.ux = (d->w + Y2_SPLITD_UNIT_W - 1) / Y2_SPLITD_UNIT_W;
    a.np = pool ? d->batch * (d->h / 2) * a.ux : (int)y2_splitd_positions(d->batch, d->h, d->w, 0);
    a.pp = y2_splitd_patch_positions(d->w, pool);
    a.tiles_n = (d->n + w.bn - 1) / w.bn;
    a.ntiles = (int)w.tiles;
    a.xbytes = (unsigned)((size_t)d->batch * d->h * d->w * d->ldx * 4);
    a.ubytes = (unsigned)w.u_bytes;
    a.ybytes = (unsigned)((size_t)d->batch * d->h * d->w / (pool ? 4 : 1) * d->ldy * 4);
    a.vec_store = d->ldy % 4 == 0 && (uintptr_t)d->y % 16 == 0;
    const bool fast = d->batch_normalize && d->activation == Y2H_ACT_LEAKY;
    void (*fn)(SplitDK);
    if (w.bn == 256) fn = fast ? conv_splitd_kernel<256, false, true> : conv_splitd_kernel<256, false, false>;
    else if (pool) fn = fast ? conv_splitd_kernel<128, true, true> : conv_splitd_kernel<128, true, false>;
    else fn = fast ? conv_splitd_kernel<128, false, true> : conv_splitd_kernel<128, false, false>;
    Y2H_CHECK(y2h_lds_limit((const void *)fn, w.lds_bytes));
    long grid = w.tiles < 256 ? w.tiles : 256;
    if (const char *g = getenv("Y2_CONV_GRID")) { if (atol(g) > 0 && atol(g) < grid) grid = atol(g); }
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(512), w.lds_bytes, S(s), a);
    Y2H_LAUNCH_CHECK();
    ++g_splitd_launches;
    return Y2H_OK;
}
