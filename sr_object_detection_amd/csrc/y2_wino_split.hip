// The batched GEMM of the Winograd F(2x2,3x3) path at the bf16 matrix rate: M[g][t][n] = sum_c V[g][t][c] U[g][n][c] with
// both fp32 operands split three ways into bf16 planes, a = h + m + l (include/y2_split_rule.h: the split, the six products
// kept, the operand layout).  V is split where it is produced (wino_input_split_kernel, y2_wino.hip), U once at weight upload
// (y2_arena.c); the raw fp32 sums go to M and wino_output_kernel finishes the layer as it does behind the fp32 GEMM.
//
//  * A persistent walk over 16 x tiles_m x tiles_n output tiles of 256 rows x 256 filters, component slowest, filter tile
//    fastest; eight waves, 2 (rows) x 4 (filters), each 128 rows x 64 filters = 4 x 2 accumulator tiles of 32x32 (128
//    registers).  No workgroup talks to another.
//  * K-tile = 16 channels = one v_mfma_f32_32x32x16_bf16 step.  One (row block, K-tile) of an operand is one contiguous
//    24 KB run that already has the LDS image's order -- [plane][k-half][row][8 channels] -- so staging is three lane-linear
//    16-byte LDS-DMA pieces per thread and operand, and a fragment read (32 rows of one plane and k-half) is 512
//    contiguous bytes: no conflicts, no swizzle.  (A 256x256 tile of six planes at 32 channels would need 2 x 96 KB.)
//  * Two LDS buffers of 48 KB, one barrier per K-tile: wait for the own DMA pieces of K-tile k, barrier (now every wave's
//    pieces are in, and every wave has finished reading the other buffer), issue the DMA of K-tile k + 1 -- of the next
//    output tile after the last one -- into the other buffer, then 18 fragment reads and 48 MFMAs.  A wave's 48 MFMAs are
//    ~1500 matrix cycles between two barriers, so the barrier round trip and the DMA latency hide under the other wave
//    of the SIMD.
//  * Per output tile and K step the six products are issued smallest first -- l h', h l', m m', m h', h m', h h' -- term
//    by term across the eight accumulator tiles, so consecutive MFMAs never wait for each other.
//  * The MFMA takes U as its row operand: a lane then holds four consecutive FILTERS of one GEMM row in four consecutive
//    registers and M is written with 16-byte stores.
//
// Compiled with -ffp-contract=off like the other conv units.
#include "y2_conv_shared.hpp"
#include "y2_split_rule.h"

typedef __attribute__((address_space(3))) void lds_void_x;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct WinoXK {
    const unsigned short *V, *U;
    float *M;
    unsigned vbytes, ubytes;
    int N;                     // filters
    int nk;                    // K-tiles: C / 16
    int tiles_m, tiles_n;      // row blocks per component, filter blocks
    int ntiles;                // 16 * tiles_m * tiles_n
    long tiles_pad;            // rows per component: 256 * tiles_m
};

__global__ __launch_bounds__(512, 1) void wino_split_gemm_kernel(WinoXK a)
{
    constexpr int OPER_B = Y2_SPLIT_BLOCK_ELEMS * 2;      // one (row block, K-tile) of one operand: 24 KB
    constexpr int PLANE_B = OPER_B / 3, HALF_B = PLANE_B / 2;
    constexpr int BUF_B = 2 * OPER_B;                     // V block | U block
    extern __shared__ __attribute__((aligned(16))) unsigned char wx_smem[];      // [2][BUF_B]

    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wv >> 2, wn = wv & 3;

    const __amdgpu_buffer_rsrc_t vr = __builtin_amdgcn_make_buffer_rsrc((void *)a.V, 0, a.vbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ur = __builtin_amdgcn_make_buffer_rsrc((void *)a.U, 0, a.ubytes, 0x00020000);

    // ---- staging cursor: K-tile s_k of this workgroup's s_i-th output tile goes to LDS buffer s_buf ----
    int s_i = 0, s_k = 0, s_buf = 0;
    bool s_live = false;
    unsigned s_voff = 0, s_uoff = 0;
    auto begin_tile = [&](int i) {
        const long tile = (long)blockIdx.x + (long)i * gridDim.x;
        s_live = tile < a.ntiles;
        if (!s_live) return;
        const int per = a.tiles_m * a.tiles_n;
        const int g = (int)(tile / per), r = (int)(tile - (long)g * per);
        const int tm = r / a.tiles_n, tn = r - tm * a.tiles_n;
        s_voff = (unsigned)((g * a.tiles_m + tm) * a.nk) * (unsigned)OPER_B + (unsigned)t * 16u;
        s_uoff = (unsigned)((g * a.tiles_n + tn) * a.nk) * (unsigned)OPER_B + (unsigned)t * 16u;
    };
    auto stage = [&]() {
        if (!s_live) return;                              // past the last tile: nothing is fetched
        unsigned char *dst = wx_smem + s_buf * BUF_B + wv * 1024;          // + lane * 16 by the DMA
        const unsigned kadd = (unsigned)s_k * (unsigned)OPER_B;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(vr, (lds_void_x *)(dst + p * 8192), 16, s_voff + kadd + p * 8192u, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, (lds_void_x *)(dst + OPER_B + p * 8192), 16, s_uoff + kadd + p * 8192u, 0, 0, 0);
        }
        s_buf ^= 1;
        if (++s_k == a.nk) { s_k = 0; begin_tile(++s_i); }
    };

    // fragment of a 32x32x16 operand: lane (r = lane & 31, h = lane >> 5) holds channels 8 h .. 8 h + 7 of row r
    const unsigned fr = (unsigned)(lane >> 5) * (unsigned)HALF_B + (unsigned)(lane & 31) * 16u;
    const unsigned v_base = fr + (unsigned)wm * (128u * 16u), u_base = (unsigned)OPER_B + fr + (unsigned)wn * (64u * 16u);

    begin_tile(0);
    stage();
    int cbuf = 0;
    for (int ci = 0;; ++ci) {
        const long tile = (long)blockIdx.x + (long)ci * gridDim.x;
        if (tile >= a.ntiles) break;
        f32x16 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        for (int k = 0; k < a.nk; ++k) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of K-tile k (and its M stores) are done
            __builtin_amdgcn_s_barrier();                         // every wave's are; nobody still reads the other buffer
            __builtin_amdgcn_sched_barrier(0);
            stage();
            __builtin_amdgcn_sched_barrier(0);
            const unsigned char *buf = wx_smem + cbuf * BUF_B;
            bf16x8 vf[4][3], uf[2][3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int j = 0; j < 2; ++j) uf[j][p] = *(const bf16x8 *)(buf + u_base + p * PLANE_B + j * 512);
#pragma unroll
                for (int i = 0; i < 4; ++i) vf[i][p] = *(const bf16x8 *)(buf + v_base + p * PLANE_B + i * 512);
            }
            // (plane of V, plane of U), smallest product first
            constexpr int PV[6] = {2, 0, 1, 1, 0, 0}, PU[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uf[j][PU[q]], vf[i][PV[q]], acc[i][j], 0, 0, 0);
            cbuf ^= 1;
        }
        // ---- raw sums to M[g][row][filter]: register 4 rg + e of a lane is filter 8 rg + 4 (lane >> 5) + e, GEMM row lane & 31 ----
        const int per = a.tiles_m * a.tiles_n;
        const int g = (int)(tile / per), r = (int)(tile - (long)g * per);
        const int tm = r / a.tiles_n, tn = r - tm * a.tiles_n;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)g * a.tiles_pad + tm * 256 + wm * 128 + i * 32 + (lane & 31);      // < 16 * tiles_pad: whole row blocks
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int n = tn * 256 + wn * 64 + j * 32 + rg * 8 + (lane >> 5) * 4;
                    if (n < a.N)                                   // N % 4 == 0: the four filters are in or out together
                        *(f32x4 *)&a.M[(size_t)row * a.N + n] = f32x4{acc[i][j][4 * rg], acc[i][j][4 * rg + 1], acc[i][j][4 * rg + 2], acc[i][j][4 * rg + 3]};
                }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

static unsigned long g_wino_split_launches = 0;
extern "C" unsigned long y2h_wino_split_launches(void) { return g_wino_split_launches; }

// M[16][tiles_pad][n] (fp32) from the split V[16][tiles_pad][c] and U[16][rows_pad(n)][c]
int y2_wino_split_gemm_launch(const unsigned short *V, const unsigned short *U, float *M, long tiles_pad, int c, int n, y2h_stream s)
{
    if (!V || !U || !M || tiles_pad <= 0 || tiles_pad % Y2_SPLIT_ROWS != 0 || c <= 0 || c % Y2_SPLIT_BK != 0 || n <= 0 || n % 4 != 0) return Y2H_EINVAL;
    if ((((uintptr_t)V | (uintptr_t)U | (uintptr_t)M) % 16) != 0) return Y2H_EINVAL;
    const size_t vb = y2_split_bytes(tiles_pad, c), ub = y2_split_bytes(y2_split_rows_pad(n), c);
    if (vb >= 4294967000ull || ub >= 4294967000ull || (size_t)16 * tiles_pad * n * 4 >= 4294967000ull) return Y2H_EINVAL;      // 32-bit buffer offsets
    WinoXK a;
    memset(&a, 0, sizeof a);
    a.V = V; a.U = U; a.M = M;
    a.vbytes = (unsigned)vb; a.ubytes = (unsigned)ub;
    a.N = n; a.nk = c / Y2_SPLIT_BK;
    a.tiles_m = (int)(tiles_pad / Y2_SPLIT_ROWS); a.tiles_n = (int)(y2_split_rows_pad(n) / Y2_SPLIT_ROWS);
    a.tiles_pad = tiles_pad;
    const long ntiles = 16L * a.tiles_m * a.tiles_n;
    if (ntiles >= 0x7fffffffL / 64) return Y2H_EINVAL;
    a.ntiles = (int)ntiles;
    long grid = 256;
    if (const char *g = getenv("Y2_CONV_GRID")) { if (atol(g) > 0 && atol(g) < grid) grid = atol(g); }
    if (grid > ntiles) grid = ntiles;
    const size_t lds = 2 * 2 * (size_t)Y2_SPLIT_BLOCK_ELEMS * 2;
    Y2H_CHECK(y2h_lds_limit((const void *)wino_split_gemm_kernel, lds));
    hipLaunchKernelGGL(wino_split_gemm_kernel, dim3((unsigned)grid), dim3(512), lds, S(s), a);
    Y2H_LAUNCH_CHECK();
    ++g_wino_split_launches;
    return Y2H_OK;
}
