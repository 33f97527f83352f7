// y2_kcf.hip -- the KCF tracker of the Kinect loop on the device, batched over trackers: what KCF_Tracker::init / ::track
// (kcf.cpp:5-45, :75-128) do per object on the host, over complexmat.hpp and piotr_fhog/.  One launch of each kernel
// serves every tracker of a call through the descriptor table (grid.y = tracker); a tracker's buffers are offsets into
// one arena.  Stages, in the order a call enqueues them:
//   patch    grey rule, the on-the-fly halving, get_subwindow (:277-325) -> the float patch
//   fhog     FHoG::extract(patch, 2, 4, 9): gradient + hard orientation bin, the cell histograms as a gather, the norm
//            sums, the 31 channels with the clip; the Hann window is multiplied in where the channel is written for the DFT
//   dft      X^ = F_R * X * F_C as dense products on v_mfma_f32_32x32x2_f32 with the twiddle matrices built at init; real
//            and imaginary parts are separate accumulations; ragged edges are zero inside the tile
//   cross / gauss / train / apply   the element-wise steps of gaussian_correlation (:327-351) and of the model
//   argmax   minMaxLoc's first maximum in row-major order, the wrap, the pose
// No floating-point atomics anywhere: every sum has one order that depends on the shapes alone, so a call run twice gives
// the same bytes.  Complex tensors are two planes, [re][R][C] then [im][R][C] (per channel).
// Built with -ffp-contract=off: the element-wise arithmetic is the rule's, operation for operation.
#include "y2_common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CH = Y2H_KCF_CHANNELS;
constexpr int CHUNKS = Y2H_KCF_CHUNKS;
constexpr int CELL = 4;
constexpr int NOR = 18;

// ---------------------------------------------------------------------------
// patch
// ---------------------------------------------------------------------------
__device__ __forceinline__ float kcf_grey(const y2h_kcf_frame &f, int y, int x)
{
    // rows outside the uploaded band cannot be asked for when the host sized the band; the clamp keeps a wrong band in bounds
    y = min(max(y, f.row_lo), f.row_hi - 1);
    const unsigned char *p = f.bytes + ((size_t)(y - f.row_lo) * f.w + x) * f.c;
    if (f.c == 1) return (float)p[0];
    return (float)((1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14);
}

// one pixel of the half-resolution image: the cubic taps (-3, 19, 19, -3)/32 at 2d-1 .. 2d+2, clamped, horizontal pass
// first, then vertical, each sum left to right
__device__ __forceinline__ float kcf_half_pixel(const y2h_kcf_frame &f, int r, int c)
{
    const float w[4] = {-3.f / 32, 19.f / 32, 19.f / 32, -3.f / 32};
    float rows[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = min(max(2 * r - 1 + j, 0), f.h - 1);
        float acc = w[0] * kcf_grey(f, y, min(max(2 * c - 1, 0), f.w - 1));
#pragma unroll
        for (int i = 1; i < 4; ++i) acc = acc + w[i] * kcf_grey(f, y, min(max(2 * c - 1 + i, 0), f.w - 1));
        rows[j] = acc;
    }
    float acc = w[0] * rows[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) acc = acc + w[j] * rows[j];
    return acc;
}

__host__ __device__ inline int kcf_half_size(int n) { return n / 2 + ((n & 1) ? ((n / 2) & 1) : 0); }

__global__ __launch_bounds__(256) void kcf_patch_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena,
                                                        y2h_kcf_frame f, const double *__restrict__ centres, int stride)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const int width = d.win_w, height = d.win_h;
    const int cols = d.resized ? kcf_half_size(f.w) : f.w, rows = d.resized ? kcf_half_size(f.h) : f.h;
    const double pcx = centres[(size_t)blockIdx.y * stride], pcy = centres[(size_t)blockIdx.y * stride + 1];
    // the `int` parameters of get_subwindow; a pose outside int range has no defined conversion: it reads as outside
    const bool sane = pcx > -1e9 && pcx < 1e9 && pcy > -1e9 && pcy < 1e9;
    const int cx = sane ? (int)pcx : 0, cy = sane ? (int)pcy : 0;
    int x1 = cx - width / 2, y1 = cy - height / 2, x2 = cx + width / 2, y2 = cy + height / 2;
    bool zero = !sane || x1 >= cols || y1 >= rows || x2 < 0 || y2 < 0;
    int top = 0, left = 0;
    if (x1 < 0) { left = -x1; x1 = 0; }
    if (y1 < 0) { top = -y1; y1 = 0; }
    if (x2 >= cols) x2 = cols; else x2 += width % 2;
    if (y2 >= rows) y2 = rows; else y2 += height % 2;
    if (x2 - x1 <= 0 || y2 - y1 <= 0) zero = true;
    float *patch = arena + d.patch;
    const long n = (long)width * height;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = 0.f;
        if (!zero) {
            const int pr = (int)(i / width), pc = (int)(i - (long)pr * width);
            const int sr = min(max(pr - top, 0), y2 - y1 - 1) + y1, sc = min(max(pc - left, 0), x2 - x1 - 1) + x1;
            v = d.resized ? kcf_half_pixel(f, sr, sc) : kcf_grey(f, sr, sc);
        }
        patch[i] = v;
    }
}

// ---------------------------------------------------------------------------
// fHOG
// ---------------------------------------------------------------------------
// gradMag with full = true on I / 255 (central differences, one-sided at the borders), and the hard bin of gradQuantize.
// The angle is taken in double from the fp32 gradient, so the bin is that of exact arithmetic on these two numbers.
__global__ __launch_bounds__(256) void kcf_grad_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const int w = d.win_w, h = d.win_h;
    const float *I = arena + d.patch;
    float *M = arena + d.mag;
    int *B = (int *)(arena + d.bin);
    const long n = (long)w * h;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        const int xp = x > 0 ? x - 1 : x, xn = x < w - 1 ? x + 1 : x, yp = y > 0 ? y - 1 : y, yn = y < h - 1 ? y + 1 : y;
        const float rx = (x == 0 || x == w - 1) ? 1.f : .5f, ry = (y == 0 || y == h - 1) ? 1.f : .5f;
        const float gx = (I[(size_t)y * w + xn] / 255.f - I[(size_t)y * w + xp] / 255.f) * rx;
        const float gy = (I[(size_t)yn * w + x] / 255.f - I[(size_t)yp * w + x] / 255.f) * ry;
        const float gxx = gx * gx, gyy = gy * gy;
        M[i] = sqrtf(gxx + gyy);
        double o = atan2((double)gy, (double)gx);
        if (o < 0) o += 2 * 3.14159265358979323846;
        int b = (int)floor(o * (NOR / (2 * 3.14159265358979323846)) + 0.5);
        if (b >= NOR || b < 0) b = 0;
        B[i] = b;
    }
}

// gradHist with softBin = -1 as a gather: one thread per (orientation, cell) walks the pixels that reach the cell, column
// by column as the reference does (x outer, y inner), and adds those of its bin; then the 8/7 boundary factors, once per
// side the cell lies on.
__global__ __launch_bounds__(256) void kcf_hist_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const int w = d.win_w, hb = d.cells_h, wb = d.cells_w, h0 = hb * CELL, w0 = wb * CELL;
    const float *M = arena + d.mag;
    const int *B = (const int *)(arena + d.bin);
    float *R1 = arena + d.hist;
    const long n = (long)NOR * hb * wb;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int o = (int)(i / ((long)hb * wb)), cell = (int)(i - (long)o * hb * wb), cy = cell / wb, cx = cell - cy * wb;
        float acc = 0.f;
        for (int x = max(CELL * cx - 2, 0); x <= min(CELL * cx + 5, w0 - 1); ++x) {
            const float xb = (x + .5f) * .25f - .5f;
            const int xb0 = xb >= 0 ? (int)xb : -1;
            const float xd = xb - xb0;
            const int dx = cx - xb0;
            if (dx != 0 && dx != 1) continue;
            for (int y = max(CELL * cy - 2, 0); y <= min(CELL * cy + 5, h0 - 1); ++y) {
                const float yb = (y + .5f) * .25f - .5f;
                const int yb0 = yb >= 0 ? (int)yb : -1;
                const int dy = cy - yb0;
                if ((dy != 0 && dy != 1) || B[(size_t)y * w + x] != o) continue;
                const float yd = yb - yb0, xyd = xd * yd;
                const float ms = dx == 0 ? (dy == 0 ? 1.f - xd - yd + xyd : yd - xyd) : (dy == 0 ? xd - xyd : xyd);
                const float m = M[(size_t)y * w + x] * (1.f / (CELL * CELL));
                acc = acc + ms * m;
            }
        }
        const float f87 = 8.f / 7.f;
        if (cx == 0) acc *= f87;
        if (cy == 0) acc *= f87;
        if (cx == wb - 1) acc *= f87;
        if (cy == hb - 1) acc *= f87;
        R1[i] = acc;
    }
}

// hogNormMatrix's sums: S[cell] = sum over the nine insensitive orientations of (R1[o] + R1[o + 9])^2, in order
__global__ __launch_bounds__(256) void kcf_norm_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const long nb = (long)d.cells_h * d.cells_w;
    const float *R1 = arena + d.hist;
    float *S = arena + d.ssum;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long)gridDim.x * 256) {
        float s = 0.f;
        for (int o = 0; o < NOR / 2; ++o) {
            const float r2 = R1[o * nb + i] + R1[(o + NOR / 2) * nb + i], sq = r2 * r2;
            s = s + sq;
        }
        S[i] = s;
    }
}

// the three hogChannels calls of fhog: 18 sensitive, 9 insensitive, 4 texture channels; channel 32 (all zero) is dropped
__global__ __launch_bounds__(256) void kcf_chan_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const int hb = d.cells_h, wb = d.cells_w;
    const long nb = (long)hb * wb;
    const float *R1 = arena + d.hist, *S = arena + d.ssum, *win = arena + d.win;      // win: [hb] row factors, [wb] column factors
    float *feat = arena + d.feat, *xw = arena + d.x;
    const float eps = 1e-4f / 4 / CELL / CELL / CELL / CELL, clip = 0.2f, r = .2357f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long)gridDim.x * 256) {
        const int y = (int)(i / wb), x = (int)(i - (long)y * wb);
        float N[4];                                          // GETT(0), (1), (hb1), (hb1 + 1): the padded matrix at (x+1, y+1), (x+1, y), (x, y+1), (x, y)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int X = x + 1 - (k >> 1), Y = y + 1 - (k & 1);
            const int vx = min(max(X, 1), wb - 1) - 1, vy = min(max(Y, 1), hb - 1) - 1;
            const float s = S[(size_t)vy * wb + vx] + S[(size_t)(vy + 1) * wb + vx] + S[(size_t)vy * wb + vx + 1] +
                            S[(size_t)(vy + 1) * wb + vx + 1] + eps;
            N[k] = 1.f / sqrtf(s);
        }
        const float wv = win[y] * win[hb + x];
        float tex[4] = {0.f, 0.f, 0.f, 0.f};
        for (int o = 0; o < NOR; ++o) {
            const float v = R1[o * nb + i];
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = v * N[k];
                if (t > clip) t = clip;
                acc = acc + t * .5f;
                tex[k] = tex[k] + t * r;
            }
            feat[o * nb + i] = acc;
            xw[o * nb + i] = acc * wv;
        }
        for (int o = 0; o < NOR / 2; ++o) {
            const float v = R1[o * nb + i] + R1[(o + NOR / 2) * nb + i];
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = v * N[k];
                if (t > clip) t = clip;
                acc = acc + t * .5f;
            }
            feat[(NOR + o) * nb + i] = acc;
            xw[(NOR + o) * nb + i] = acc * wv;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            feat[(NOR + NOR / 2 + k) * nb + i] = tex[k];
            xw[(NOR + NOR / 2 + k) * nb + i] = tex[k] * wv;
        }
    }
}

// ---------------------------------------------------------------------------
// DFT: two passes of dense products.  One wave per 32 x 32 output tile of O1 = A1*B1 + A2*B2 and O2 = A3*B3 + A4*B4
// (a missing term or output is a null pointer).  A lane reads eight consecutive k of its A row and of its B column per
// 16-step; rows, columns and k past the matrix read as zero, so any M, N, K >= 1 takes this kernel.
// ---------------------------------------------------------------------------
struct Prod {
    const float *a[4], *b[4];
    float *o[2];
    int M, N, K, lda, ldb, ldo;
    long sa[4], sb[4], so;         // strides between the matrices of a batch
    float alpha;
};

// COMP: every matrix instruction's pair of products is added to the running sum with its rounding error carried in
// `low` (two-sum), so the sum over k is rounded about once whatever its length.  The single-channel transforms take it:
// their small bins are differences of large partial sums, and kf divides yf.
template <bool COMP>
__device__ __forceinline__ void prod_term(const float *__restrict__ A, const float *__restrict__ Bm, int M, int N, int K, int lda,
                                          int ldb, int row, int col, int lh, f32x16 &acc, f32x16 &low)
{
    const bool rok = row < M, cok = col < N;
    const float *ar = A + (size_t)(rok ? row : 0) * lda;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + 8 * lh + u;
            const bool kok = k < K;
            av[u] = (rok && kok) ? ar[k] : 0.f;
            bv[u] = (cok && kok) ? Bm[(size_t)k * ldb + col] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (!COMP) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            } else {
                f32x16 zero;
#pragma unroll
                for (int v = 0; v < 16; ++v) zero[v] = 0.f;
                const f32x16 pair = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], zero, 0, 0, 0);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float s = acc[v] + pair[v], bb = s - acc[v];
                    const float e1 = acc[v] - (s - bb), e2 = pair[v] - bb;
                    low[v] = low[v] + (e1 + e2);
                    acc[v] = s;
                }
            }
        }
    }
}

// pass 0 multiplies by the column twiddles from the right, pass 1 by the row twiddles from the left
__device__ __forceinline__ bool kcf_dft_stage(const y2h_kcf_desc &d, float *arena, int which, int pass, Prod &p, int &nb)
{
    const int R = d.cells_h, C = d.cells_w;
    const long P = (long)R * C;
    const float *cc = arena + d.cc, *nsc = arena + d.nsc, *cr = arena + d.cr, *sr = arena + d.sr, *nsr = arena + d.nsr;
    for (int k = 0; k < 4; ++k) { p.a[k] = p.b[k] = nullptr; p.sa[k] = p.sb[k] = 0; }
    p.o[0] = p.o[1] = nullptr; p.alpha = 1.f; p.so = 2 * P; nb = 1;
    long src, tmp, dst;
    bool inverse = false;
    switch (which) {
    case Y2H_KCF_DFT_X: src = d.x; tmp = d.y; dst = d.xf; nb = CH; break;
    case Y2H_KCF_DFT_G: src = d.g; tmp = d.gy; dst = d.kf; break;
    case Y2H_KCF_DFT_LAB: src = d.lab; tmp = d.gy; dst = d.yf; break;
    case Y2H_KCF_IDFT_Z: src = d.z; tmp = d.t; dst = d.xy; inverse = true; break;
    case Y2H_KCF_IDFT_P: src = d.p; tmp = d.t; dst = d.resp; inverse = true; break;
    default: return false;
    }
    p.ldo = C;
    if (!inverse && pass == 0) {            // Y = X * (Cc - i Sc), X real
        p.M = R; p.N = C; p.K = C; p.lda = C; p.ldb = C;
        p.a[0] = arena + src; p.b[0] = cc; p.a[2] = arena + src; p.b[2] = nsc;
        p.sa[0] = p.sa[2] = P;
        p.o[0] = arena + tmp; p.o[1] = arena + tmp + P;
    } else if (!inverse) {                  // X^ = (Cr - i Sr) * Y
        p.M = R; p.N = C; p.K = R; p.lda = R; p.ldb = C;
        p.a[0] = cr; p.b[0] = arena + tmp; p.a[1] = sr; p.b[1] = arena + tmp + P;
        p.a[2] = cr; p.b[2] = arena + tmp + P; p.a[3] = nsr; p.b[3] = arena + tmp;
        p.sb[0] = p.sb[1] = p.sb[2] = p.sb[3] = 2 * P;
        p.o[0] = arena + dst; p.o[1] = arena + dst + P;
    } else if (pass == 0) {                 // T = (Cr + i Sr) * Z
        p.M = R; p.N = C; p.K = R; p.lda = R; p.ldb = C;
        p.a[0] = cr; p.b[0] = arena + src; p.a[1] = nsr; p.b[1] = arena + src + P;
        p.a[2] = sr; p.b[2] = arena + src; p.a[3] = cr; p.b[3] = arena + src + P;
        p.o[0] = arena + tmp; p.o[1] = arena + tmp + P;
    } else {                                // Re(T * (Cc + i Sc)) / (R*C)
        p.M = R; p.N = C; p.K = C; p.lda = C; p.ldb = C;
        p.a[0] = arena + tmp; p.b[0] = cc; p.a[1] = arena + tmp + P; p.b[1] = nsc;
        p.o[0] = arena + dst;
        p.alpha = 1.f / (float)(R * C);
    }
    return true;
}

template <bool COMP>
__global__ __launch_bounds__(256) void kcf_dft_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena, int which,
                                                      int pass)
{
    const y2h_kcf_desc d = desc[blockIdx.z];
    Prod p;
    int nb;
    if (!kcf_dft_stage(d, arena, which, pass, p, nb)) return;
    const int batch = blockIdx.y;
    if (batch >= nb) return;
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int tn = (p.N + 31) / 32, tiles = ((p.M + 31) / 32) * tn;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= tiles) return;                               // wave-uniform
    const int m0 = (tile / tn) * 32, n0 = (tile % tn) * 32;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (!p.o[half]) continue;
        f32x16 acc, low;
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc[v] = 0.f; low[v] = 0.f; }
#pragma unroll
        for (int term = 0; term < 2; ++term) {
            const int k = 2 * half + term;
            if (!p.a[k]) continue;
            prod_term<COMP>(p.a[k] + batch * p.sa[k], p.b[k] + batch * p.sb[k], p.M, p.N, p.K, p.lda, p.ldb, m0 + li, n0 + li, lh, acc, low);
        }
        float *out = p.o[half] + batch * p.so;
#pragma unroll
        for (int v = 0; v < 16; ++v) {                       // acc[v] is row (v >> 2) * 8 + lh * 4 + (v & 3), column li
            const int row = m0 + (v >> 2) * 8 + lh * 4 + (v & 3), col = n0 + li;
            if (row < p.M && col < p.N) out[(size_t)row * p.ldo + col] = (acc[v] + low[v]) * p.alpha;
        }
    }
}

// ---------------------------------------------------------------------------
// element-wise steps
// ---------------------------------------------------------------------------
// sum of 256 per-thread values in a fixed tree
__device__ __forceinline__ float block_sum(float v, float *lds)
{
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// the cross-spectrum summed over the channels, z = sum_ch a[ch] * conj(b[ch]) (b = the model; autocorrelation: b = a, so
// z = |a|^2), and this chunk's share of sqr_norm's sums of a and of b: chunk c of CHUNKS owns the elements c*256 + tid,
// (c + CHUNKS)*256 + tid, ...; its 256 threads' sums are added in a tree, the chunks' sums in chunk order by the reader.
__global__ __launch_bounds__(256) void kcf_cross_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena, int autoc)
{
    __shared__ float lds[256];
    const y2h_kcf_desc d = desc[blockIdx.y];
    const long P = (long)d.cells_h * d.cells_w;
    const float *a = arena + d.xf, *b = arena + (autoc ? d.xf : d.model_xf);
    float *z = arena + d.z, *part = arena + d.part;
    float sa = 0.f, sb = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)CHUNKS * 256) {
        float zr = 0.f, zi = 0.f;
        for (int c = 0; c < CH; ++c) {
            const float ar = a[(2 * c) * P + i], ai = a[(2 * c + 1) * P + i], br = b[(2 * c) * P + i], bi = b[(2 * c + 1) * P + i];
            const float arr = ar * ar, aii = ai * ai, brr = br * br, bii = bi * bi;
            sa = sa + (arr + aii);
            sb = sb + (brr + bii);
            const float rr = ar * br, ii = ai * bi, ir = ai * br, ri = ar * bi;
            zr = zr + (rr + ii);
            zi = zi + (ir - ri);
        }
        z[i] = zr; z[P + i] = zi;
    }
    const float ta = block_sum(sa, lds), tb = block_sum(sb, lds);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = ta; part[2 * blockIdx.x + 1] = tb; }
}

// g = exp(-1/sigma^2 * max((xx + yy - 2 * xy) * numel_inv, 0)), sigma = 0.5
__global__ __launch_bounds__(256) void kcf_gauss_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const long P = (long)d.cells_h * d.cells_w;
    const float *part = arena + d.part, *xy = arena + d.xy;
    float *g = arena + d.g;
    float xx = 0.f, yy = 0.f;
    for (int c = 0; c < CHUNKS; ++c) { xx = xx + part[2 * c]; yy = yy + part[2 * c + 1]; }
    xx = xx / (float)P; yy = yy / (float)P;
    const float numel_inv = 1.f / (float)(P * CH), scale = (float)(-1. / (0.5 * 0.5));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float v = (xx + yy - 2.f * xy[i]) * numel_inv;
        g[i] = expf(scale * fmaxf(v, 0.f));
    }
}

// alphaf = yf / (kf + lambda); mode 0 (init): the model is (xf, alphaf); mode 1 (update): both are interpolated with
// factor 0.02 and the stored pose takes the tracked one
__global__ __launch_bounds__(256) void kcf_train_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena, int mode,
                                                        double *__restrict__ pose, const y2h_kcf_rec *__restrict__ rec)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const long P = (long)d.cells_h * d.cells_w;
    const float *yf = arena + d.yf, *kf = arena + d.kf, *xf = arena + d.xf;
    float *ma = arena + d.model_alphaf, *mx = arena + d.model_xf;
    const float keep = (float)(1. - 0.02), take = (float)0.02, lambda = (float)1e-4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float a = yf[i], b = yf[P + i], c = kf[i] + lambda, e = kf[P + i];
        const float cc = c * c, ee = e * e, den = cc + ee;
        const float ac = a * c, be = b * e, bc = b * c, ae = a * e;
        const float re = (ac + be) / den, im = (bc - ae) / den;
        if (mode == 0) { ma[i] = re; ma[P + i] = im; }
        else { ma[i] = ma[i] * keep + re * take; ma[P + i] = ma[P + i] * keep + im * take; }
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < 2 * CH * P; i += (long)gridDim.x * 256)
        mx[i] = mode == 0 ? xf[i] : mx[i] * keep + xf[i] * take;
    if (mode == 1 && blockIdx.x == 0 && threadIdx.x == 0) {
        pose[2 * blockIdx.y] = rec[blockIdx.y].cx;
        pose[2 * blockIdx.y + 1] = rec[blockIdx.y].cy;
    }
}

// p = model_alphaf * kzf
__global__ __launch_bounds__(256) void kcf_apply_kernel(const y2h_kcf_desc *__restrict__ desc, float *__restrict__ arena)
{
    const y2h_kcf_desc d = desc[blockIdx.y];
    const long P = (long)d.cells_h * d.cells_w;
    const float *ma = arena + d.model_alphaf, *kf = arena + d.kf;
    float *p = arena + d.p;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float a = ma[i], b = ma[P + i], c = kf[i], e = kf[P + i];
        const float ac = a * c, be = b * e, ae = a * e, bc = b * c;
        p[i] = ac - be; p[P + i] = ae + bc;
    }
}

// minMaxLoc: the first maximum in row-major order; the wrap (> rows/2, > cols/2, integer halves); pose += 4 * loc
__global__ __launch_bounds__(256) void kcf_argmax_kernel(const y2h_kcf_desc *__restrict__ desc, const float *__restrict__ arena,
                                                         const double *__restrict__ pose, y2h_kcf_rec *__restrict__ rec)
{
    __shared__ float bv[256];
    __shared__ int bi[256];
    const y2h_kcf_desc d = desc[blockIdx.x];
    const int R = d.cells_h, C = d.cells_w, P = R * C, t = threadIdx.x;
    const float *resp = arena + d.resp;
    float best = -FLT_MAX;
    int at = 0x7fffffff;
    for (int i = t; i < P; i += 256) {
        const float v = resp[i];
        if (at == 0x7fffffff || v > best) { best = v; at = i; }
    }
    bv[t] = best; bi[t] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const float v = bv[t + s];
            const int j = bi[t + s];
            if (j != 0x7fffffff && (bi[t] == 0x7fffffff || v > bv[t] || (v == bv[t] && j < bi[t]))) { bv[t] = v; bi[t] = j; }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int idx = bi[0] == 0x7fffffff ? 0 : bi[0];
        int my = idx / C, mx = idx - my * C;
        if (my > R / 2) my -= R;
        if (mx > C / 2) mx -= C;
        y2h_kcf_rec r;
        r.cx = pose[2 * blockIdx.x] + (double)(CELL * mx);
        r.cy = pose[2 * blockIdx.x + 1] + (double)(CELL * my);
        r.peak = bv[0]; r.mx = mx; r.my = my; r.pad_ = 0;
        rec[blockIdx.x] = r;
    }
}

inline unsigned blocks_for(long n, long cap = 1024)
{
    long g = (n + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline bool bad_batch(const void *desc, const void *arena, int n) { return !desc || !arena || n < 1 || n > Y2H_KCF_MAX_TRACKERS; }

} // namespace

extern "C" int y2h_kcf_patch(const y2h_kcf_desc *desc, int n, float *arena, const y2h_kcf_frame *f, const double *centres,
                             int stride, long max_pixels, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || !f || !f->bytes || !centres || stride < 2 || max_pixels < 1) return Y2H_EINVAL;
    if (f->h < 1 || f->w < 1 || (f->c != 1 && f->c != 3 && f->c != 4) || f->row_lo < 0 || f->row_hi > f->h || f->row_lo >= f->row_hi)
        return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_patch_kernel, dim3(blocks_for(max_pixels), n), dim3(256), 0, S(s), desc, arena, *f, centres, stride);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_fhog(const y2h_kcf_desc *desc, int n, float *arena, long max_pixels, long max_cells, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || max_pixels < 1 || max_cells < 1) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_grad_kernel, dim3(blocks_for(max_pixels), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    hipLaunchKernelGGL(kcf_hist_kernel, dim3(blocks_for(max_cells * NOR), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    hipLaunchKernelGGL(kcf_norm_kernel, dim3(blocks_for(max_cells), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    hipLaunchKernelGGL(kcf_chan_kernel, dim3(blocks_for(max_cells), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_dft(const y2h_kcf_desc *desc, int n, float *arena, int which, int max_side, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || which < 0 || which > Y2H_KCF_IDFT_P || max_side < 1 || max_side > Y2H_KCF_MAX_CELLS) return Y2H_EINVAL;
    const int t = (max_side + 31) / 32, tiles = t * t;
    const int nb = which == Y2H_KCF_DFT_X ? CH : 1;
    for (int pass = 0; pass < 2; ++pass) {
        const dim3 grid((unsigned)((tiles + 3) / 4), nb, n);
        if (nb == 1) hipLaunchKernelGGL(kcf_dft_kernel<true>, grid, dim3(256), 0, S(s), desc, arena, which, pass);
        else hipLaunchKernelGGL(kcf_dft_kernel<false>, grid, dim3(256), 0, S(s), desc, arena, which, pass);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}

extern "C" int y2h_kcf_cross(const y2h_kcf_desc *desc, int n, float *arena, int autocorrelation, y2h_stream s)
{
    if (bad_batch(desc, arena, n)) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_cross_kernel, dim3(CHUNKS, n), dim3(256), 0, S(s), desc, arena, autocorrelation != 0);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_gauss(const y2h_kcf_desc *desc, int n, float *arena, long max_cells, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || max_cells < 1) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_gauss_kernel, dim3(blocks_for(max_cells), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_train(const y2h_kcf_desc *desc, int n, float *arena, int update, double *pose, const y2h_kcf_rec *rec,
                             long max_cells, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || max_cells < 1 || (update && (!pose || !rec))) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_train_kernel, dim3(blocks_for(max_cells * 2 * CH, 2048), n), dim3(256), 0, S(s), desc, arena,
                       update ? 1 : 0, pose, rec);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_apply(const y2h_kcf_desc *desc, int n, float *arena, long max_cells, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || max_cells < 1) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_apply_kernel, dim3(blocks_for(max_cells), n), dim3(256), 0, S(s), desc, arena);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_kcf_argmax(const y2h_kcf_desc *desc, int n, const float *arena, const double *pose, y2h_kcf_rec *rec, y2h_stream s)
{
    if (bad_batch(desc, arena, n) || !pose || !rec) return Y2H_EINVAL;
    hipLaunchKernelGGL(kcf_argmax_kernel, dim3(n), dim3(256), 0, S(s), desc, arena, pose, rec);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
