// The picture side of nightmare.c's optimize_picture / run_nightmare on the device (host half: host/y2_dream.c).
//
//   y2h_dream_resample   crop_image (image.c:1512, constrain_int repeats edge pixels) -> resize_image (image.c:1950, two
//                        separable fp32 passes) -> crop_image, with flip_image (image.c:1056) on either end and either
//                        layout on either end: picture -> NHWC network input, NHWC image gradient -> picture-sized update,
//                        and the zoom of a round's end are this one pair of kernels.  The arithmetic and its order are
//                        those of y2h_resize_chw (y2_detect.hip); this file is built with -ffp-contract=off like the
//                        reference, so no product is contracted into an FMA.
//   y2h_dream_loss       calculate_loss (nightmare.c:23-32): mean, variance about that mean, thresholded copy, and the
//                        count of what was kept.
//   y2h_dream_apply      normalize_array (utils.c:482), axpy_cpu, constrain_image (image.c:1115) on the picture in HBM.
//   y2h_dream_rotate     rotate_image (image.c:1481) with bilinear_interpolate (image.c:1935).
//
// Reductions are deterministic: chunk b of Y2H_DREAM_CHUNK values is summed by block b (each thread 16 values in index
// order, then a fixed 256-leaf tree in LDS) into partials[b]; whoever needs the total sums the partials in chunk order
// with the same tree.  No floating-point atomics; the only atomic is the integer count of selected values.
#include "y2_common.hpp"

#define DREAM_NT 256
#define DREAM_PER (Y2H_DREAM_CHUNK / DREAM_NT)

__device__ __forceinline__ int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

// ---------------------------------------------------------------------------
// resample
// ---------------------------------------------------------------------------
__device__ __forceinline__ float resample_src(const y2h_dream_resample &r, const float *__restrict__ src, int k, int row, int x)
{
    // pixel (x, row) of crop_image(src, cx, cy, cw, ch); x is held inside the crop, so no address leaves the source
    const int sr = clampi(row + r.cy, 0, r.sh - 1);
    int sx = clampi(clampi(x, 0, r.cw - 1) + r.cx, 0, r.sw - 1);
    if (r.src_flip) sx = r.sw - 1 - sx;
    return r.src_nhwc ? src[((long)sr * r.sw + sx) * r.c + k] : src[((long)k * r.sh + sr) * r.sw + sx];
}

__global__ __launch_bounds__(DREAM_NT) void dream_cols_kernel(y2h_dream_resample r, const float *__restrict__ src,
                                                              float *__restrict__ part, float w_scale)
{
    const long total = (long)r.c * r.ch * r.ow;
    for (long idx = (long)blockIdx.x * DREAM_NT + threadIdx.x; idx < total; idx += (long)gridDim.x * DREAM_NT) {
        const int col = (int)(idx % r.ow);
        const int row = (int)((idx / r.ow) % r.ch);
        const int k = (int)(idx / ((long)r.ow * r.ch));
        float val;
        if (col == r.ow - 1 || r.cw == 1) val = resample_src(r, src, k, row, r.cw - 1);
        else {
            const float sx = col * w_scale;
            const int ix = (int)sx;
            const float dx = sx - ix;
            val = (1 - dx) * resample_src(r, src, k, row, ix) + dx * resample_src(r, src, k, row, ix + 1);
        }
        part[idx] = val;
    }
}

__global__ __launch_bounds__(DREAM_NT) void dream_rows_kernel(y2h_dream_resample r, const float *__restrict__ part,
                                                              float *__restrict__ dst, float h_scale)
{
    const long total = (long)r.c * r.oh * r.ow;
    for (long idx = (long)blockIdx.x * DREAM_NT + threadIdx.x; idx < total; idx += (long)gridDim.x * DREAM_NT) {
        const int i = (int)(idx % r.ow);
        const int j = (int)((idx / r.ow) % r.oh);
        const int k = (int)(idx / ((long)r.ow * r.oh));
        // pixel (i, j) of crop_image(resized, px, py, ow, oh)
        const int row = clampi(j + r.py, 0, r.oh - 1);
        const int col = clampi(i + r.px, 0, r.ow - 1);
        const float sy = row * h_scale;
        int iy = (int)sy;
        const float dy = sy - iy;
        if (iy > r.ch - 1) iy = r.ch - 1;
        const float *p = part + ((long)k * r.ch + iy) * r.ow + col;
        float val = (1 - dy) * p[0];
        if (!(row == r.oh - 1 || r.ch == 1)) val = val + dy * p[iy + 1 < r.ch ? r.ow : 0];
        const int di = r.dst_flip ? r.ow - 1 - i : i;
        if (r.dst_nhwc) dst[((long)j * r.ow + di) * r.c + k] = val;
        else dst[((long)k * r.oh + j) * r.ow + di] = val;
    }
}

extern "C" size_t y2h_dream_resample_tmp_floats(const y2h_dream_resample *r)
{
    if (!r || r->c <= 0 || r->ch <= 0 || r->ow <= 0) return 0;
    return (size_t)r->c * r->ch * r->ow;
}

extern "C" int y2h_dream_resample_run(const y2h_dream_resample *r, const float *src, float *tmp, float *dst, y2h_stream s)
{
    if (!r || !src || !tmp || !dst || r->c <= 0 || r->sh <= 0 || r->sw <= 0 || r->ch <= 0 || r->cw <= 0 || r->oh <= 0 || r->ow <= 0)
        return Y2H_EINVAL;
    // a one-pixel result takes the last column / the first row whatever the scale (0/0 in the reference, which never uses it)
    const float w_scale = r->ow > 1 ? (float)(r->cw - 1) / (r->ow - 1) : 0.f;
    const float h_scale = r->oh > 1 ? (float)(r->ch - 1) / (r->oh - 1) : 0.f;
    hipLaunchKernelGGL(dream_cols_kernel, dim3(y2h_grid((long)r->c * r->ch * r->ow, DREAM_NT)), dim3(DREAM_NT), 0, S(s), *r, src, tmp, w_scale);
    Y2H_LAUNCH_CHECK();
    hipLaunchKernelGGL(dream_rows_kernel, dim3(y2h_grid((long)r->c * r->oh * r->ow, DREAM_NT)), dim3(DREAM_NT), 0, S(s), *r, tmp, dst, h_scale);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// deterministic sums
// ---------------------------------------------------------------------------
__device__ __forceinline__ float block_tree(float v, float *sh)
{
    const int t = threadIdx.x;
    __syncthreads();                    // sh may still be read from the tree before
    sh[t] = v;
    __syncthreads();
    for (int s = DREAM_NT / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// the partials in chunk order: thread t takes t, t + 256, ...; then the tree
__device__ __forceinline__ float total_of(const float *__restrict__ partials, int chunks, float *sh)
{
    float acc = 0.f;
    for (int i = threadIdx.x; i < chunks; i += DREAM_NT) acc += partials[i];
    return block_tree(acc, sh);
}

// mode 0: sum x; mode 1: sum (x - mean)^2 with mean = total(sums) / n
__global__ __launch_bounds__(DREAM_NT) void dream_partial_kernel(const float *__restrict__ x, long n, int chunks, int mode,
                                                                 const float *__restrict__ sums, float *__restrict__ partials,
                                                                 float *__restrict__ stat, int *__restrict__ selected)
{
    __shared__ float sh[DREAM_NT];
    float mean = 0.f;
    if (mode) {
        mean = total_of(sums, chunks, sh) / n;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            stat[0] = mean;
            if (selected) *selected = 0;
        }
    }
    const long base = (long)blockIdx.x * Y2H_DREAM_CHUNK + threadIdx.x;
    float acc = 0.f;
    for (int j = 0; j < DREAM_PER; ++j) {
        const long i = base + (long)j * DREAM_NT;
        if (i < n) {
            const float v = x[i];
            acc += mode ? (v - mean) * (v - mean) : v;
        }
    }
    const float tot = block_tree(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// nightmare.c:29: delta[i] > mean + thresh*sqrt(var) is a comparison of doubles
__global__ __launch_bounds__(DREAM_NT) void dream_threshold_kernel(const float *__restrict__ x, float *__restrict__ delta, long n,
                                                                   int chunks, float thresh, const float *__restrict__ sums,
                                                                   const float *__restrict__ sqs, float *__restrict__ stat,
                                                                   int *__restrict__ selected)
{
    __shared__ float sh[DREAM_NT];
    __shared__ int cnt;
    const float mean = total_of(sums, chunks, sh) / n;
    const float var = total_of(sqs, chunks, sh) / n;
    const double limit = (double)mean + (double)thresh * sqrt((double)var);
    if (threadIdx.x == 0) cnt = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) stat[1] = var;
    __syncthreads();
    const long base = (long)blockIdx.x * Y2H_DREAM_CHUNK + threadIdx.x;
    int mine = 0;
    for (int j = 0; j < DREAM_PER; ++j) {
        const long i = base + (long)j * DREAM_NT;
        if (i < n) {
            const float v = x[i];
            const int keep = (double)v > limit;
            delta[i] = keep ? v : 0.f;
            mine += keep;
        }
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(selected, cnt);
}

extern "C" int y2h_dream_chunks(long n) { return n <= 0 ? 0 : (int)((n + Y2H_DREAM_CHUNK - 1) / Y2H_DREAM_CHUNK); }

static int launch_moments(const float *x, long n, float *partials, float *stat, int *selected, y2h_stream s)
{
    const int chunks = y2h_dream_chunks(n);
    hipLaunchKernelGGL(dream_partial_kernel, dim3(chunks), dim3(DREAM_NT), 0, S(s), x, n, chunks, 0, (const float *)nullptr, partials,
                       stat, (int *)nullptr);
    Y2H_LAUNCH_CHECK();
    hipLaunchKernelGGL(dream_partial_kernel, dim3(chunks), dim3(DREAM_NT), 0, S(s), x, n, chunks, 1, (const float *)partials,
                       partials + chunks, stat, selected);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_dream_loss(const float *output, float *delta, long n, float thresh, float *partials, float *stat, int *selected,
                              y2h_stream s)
{
    if (!output || !delta || !partials || !stat || !selected || n <= 0 || n > (long)Y2H_DREAM_CHUNK * 0x7fffff) return Y2H_EINVAL;
    const int chunks = y2h_dream_chunks(n);
    int rc = launch_moments(output, n, partials, stat, selected, s);
    if (rc != Y2H_OK) return rc;
    hipLaunchKernelGGL(dream_threshold_kernel, dim3(chunks), dim3(DREAM_NT), 0, S(s), output, delta, n, chunks, thresh,
                       (const float *)partials, (const float *)(partials + chunks), stat, selected);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// the update of the picture
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DREAM_NT) void dream_apply_kernel(float *__restrict__ picture, const float *__restrict__ out, long n,
                                                               float rate, int norm, int chunks, const float *__restrict__ sums,
                                                               const float *__restrict__ sqs, float *__restrict__ stat)
{
    __shared__ float sh[DREAM_NT];
    float mu = 0.f, sigma = 1.f;
    if (norm) {
        mu = total_of(sums, chunks, sh) / n;
        const float var = total_of(sqs, chunks, sh) / n;
        sigma = (float)sqrt((double)var);                   // utils.c:486
        if (blockIdx.x == 0 && threadIdx.x == 0) stat[1] = var;
    }
    for (long i = (long)blockIdx.x * DREAM_NT + threadIdx.x; i < n; i += (long)gridDim.x * DREAM_NT) {
        float v = out[i];
        if (norm) v = (v - mu) / sigma;                     // 0/0 when nothing was selected: NaN, as in the reference
        float p = picture[i] + rate * v;                    // axpy_cpu
        if (p < 0) p = 0;                                   // constrain_image: a NaN passes both tests
        if (p > 1) p = 1;
        picture[i] = p;
    }
}

extern "C" int y2h_dream_apply(float *picture, const float *out, long n, float rate, int norm, float *partials, float *stat,
                               y2h_stream s)
{
    if (!picture || !out || !partials || !stat || n <= 0 || n > (long)Y2H_DREAM_CHUNK * 0x7fffff) return Y2H_EINVAL;
    const int chunks = y2h_dream_chunks(n);
    if (norm) {
        int rc = launch_moments(out, n, partials, stat, nullptr, s);
        if (rc != Y2H_OK) return rc;
    }
    hipLaunchKernelGGL(dream_apply_kernel, dim3(y2h_grid(n, DREAM_NT)), dim3(DREAM_NT), 0, S(s), picture, out, n, rate, norm, chunks,
                       (const float *)partials, (const float *)(partials + chunks), stat);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// rotate_image
// ---------------------------------------------------------------------------
__device__ __forceinline__ float pixel_extend(const float *__restrict__ im, int w, int h, int x, int y)
{
    if (x < 0) x = 0;
    if (x >= w) x = w - 1;
    if (y < 0) y = 0;
    if (y >= h) y = h - 1;
    return im[(long)y * w + x];
}

__global__ __launch_bounds__(DREAM_NT) void dream_rotate_kernel(const float *__restrict__ src, float *__restrict__ dst, int c, int h,
                                                                int w, double cs, double sn)
{
    const long total = (long)c * h * w;
    const float cx = (float)(w / 2.);
    const float cy = (float)(h / 2.);
    for (long idx = (long)blockIdx.x * DREAM_NT + threadIdx.x; idx < total; idx += (long)gridDim.x * DREAM_NT) {
        const int x = (int)(idx % w);
        const int y = (int)((idx / w) % h);
        const float *im = src + (idx / ((long)w * h)) * ((long)w * h);
        const float rx = (float)(cs * (double)(x - cx) - sn * (double)(y - cy) + (double)cx);
        const float ry = (float)(sn * (double)(x - cx) + cs * (double)(y - cy) + (double)cy);
        const int ix = (int)floorf(rx);
        const int iy = (int)floorf(ry);
        const float dx = rx - ix;
        const float dy = ry - iy;
        dst[idx] = (1 - dy) * (1 - dx) * pixel_extend(im, w, h, ix, iy) +
                   dy * (1 - dx) * pixel_extend(im, w, h, ix, iy + 1) +
                   (1 - dy) * dx * pixel_extend(im, w, h, ix + 1, iy) +
                   dy * dx * pixel_extend(im, w, h, ix + 1, iy + 1);
    }
}

extern "C" int y2h_dream_rotate(const float *src, float *dst, int c, int h, int w, double cos_rad, double sin_rad, y2h_stream s)
{
    if (!src || !dst || src == dst || c <= 0 || h <= 0 || w <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(dream_rotate_kernel, dim3(y2h_grid((long)c * h * w, DREAM_NT)), dim3(DREAM_NT), 0, S(s), src, dst, c, h, w,
                       cos_rad, sin_rad);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
