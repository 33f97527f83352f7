// y2_image.hip -- frame ingest on the device: what every caller does
// immediately before network_predict.  Reference behaviour restated:
//   * 8-bit interleaved frame -> float planes in [0,1]       yolo_v2_class.hpp:94-113 (ipl_to_image),
//                                                            image.c:2045-2067 (load_image_stb: (float)v/255.)
//   * swap planes 0 and 2 (BGR -> RGB)                        yolo_v2_class.hpp:133-141, image.c:1181
//   * fill_image / embed_image / letterbox_image              image.c:1601, :1087, :1607-1645
// All of it is HBM-bound byte shuffling: one read + one write per element, 128-bit stores where
// the layout allows.  The arithmetic (a single double division rounded to fp32, copies) is
// bit-identical to the C code.
#include "y2_common.hpp"
#include "y2_depth_rule.h"

// dst[k][y][x] = (float)( src[y*step + x*c + sk] / 255. ), sk = k with planes 0 and 2 exchanged when swap_rb.
// One thread per output pixel; the c source bytes of a pixel are read once and fanned out to the planes.
__global__ __launch_bounds__(256) void u8_to_planes_kernel(const unsigned char *__restrict__ src, int h, int w, int c,
                                                           long step, long frame_bytes, int planes, int swap_rb,
                                                           float *__restrict__ dst)
{
    const long hw = (long)h * w;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= hw) return;
    const int b = blockIdx.y;
    const int y = (int)(idx / w), x = (int)(idx - (long)y * w);
    const unsigned char *p = src + (size_t)b * frame_bytes + (size_t)y * step + (size_t)x * c;
    float *o = dst + (size_t)b * planes * hw + idx;
    for (int k = 0; k < planes; ++k) {
        int sk = k;
        if (swap_rb && c >= 3) sk = (k == 0) ? 2 : (k == 2 ? 0 : k);
        o[(size_t)k * hw] = (float)((double)p[sk] / 255.);
    }
}

extern "C" int y2h_u8_to_planes(const unsigned char *src, int batch, int h, int w, int c, long step, long frame_bytes,
                                int planes, int swap_rb, float *dst, y2h_stream s)
{
    if (!src || !dst || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || planes <= 0 || planes > c || step < (long)w * c ||
        frame_bytes < step * h) return Y2H_EINVAL;
    const long hw = (long)h * w;
    hipLaunchKernelGGL(u8_to_planes_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)batch), dim3(256), 0, S(s),
                       src, h, w, c, step, frame_bytes, planes, swap_rb, dst);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

__global__ __launch_bounds__(256) void fill_kernel(float *__restrict__ dst, long n, float v)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = v;
}

extern "C" int y2h_fill(float *dst, long n, float v, y2h_stream s)
{
    if (!dst || n <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(fill_kernel, dim3(y2h_grid(n, 256)), dim3(256), 0, S(s), dst, n, v);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// embed_image (image.c:1087) with set_pixel's bounds test (image.c:2121-2123: writes outside dest are dropped)
__global__ __launch_bounds__(256) void embed_kernel(const float *__restrict__ src, int c, int sh, int sw,
                                                    float *__restrict__ dst, int dh, int dw, int dx, int dy)
{
    const long total = (long)c * sh * sw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % sw);
        const int y = (int)((i / sw) % sh);
        const int k = (int)(i / ((long)sw * sh));
        const int X = dx + x, Y = dy + y;
        if (X < 0 || Y < 0 || X >= dw || Y >= dh) continue;
        dst[((size_t)k * dh + Y) * dw + X] = src[i];
    }
}

extern "C" int y2h_embed_chw(const float *src, int c, int sh, int sw, float *dst, int dh, int dw, int dx, int dy,
                             y2h_stream s)
{
    if (!src || !dst || c <= 0 || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(embed_kernel, dim3(y2h_grid((long)c * sh * sw, 256)), dim3(256), 0, S(s), src, c, sh, sw, dst, dh,
                       dw, dx, dy);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// letterbox geometry (image.c:1607-1622): keep the aspect ratio, integer arithmetic as in the reference
extern "C" void y2h_letterbox_dims(int iw, int ih, int w, int h, int *new_w, int *new_h)
{
    int nw = iw, nh = ih;
    if (((float)w / iw) < ((float)h / ih)) { nw = w; nh = (ih * w) / iw; }
    else { nh = h; nw = (iw * h) / ih; }
    *new_w = nw; *new_h = nh;
}

// letterbox_image (image.c:1624): resize to (new_w,new_h), fill the box with .5, embed centred.
// tmp: c*ih*new_w floats (resize pass 1) + c*new_h*new_w floats (the resized image).
extern "C" int y2h_letterbox_chw(const float *src, int c, int ih, int iw, float *tmp, float *dst, int h, int w, y2h_stream s)
{
    if (!src || !tmp || !dst || c <= 0 || ih <= 0 || iw <= 0 || h <= 0 || w <= 0) return Y2H_EINVAL;
    int nw, nh;
    y2h_letterbox_dims(iw, ih, w, h, &nw, &nh);
    if (nw <= 0 || nh <= 0) return Y2H_EINVAL;
    float *resized = tmp + (size_t)c * ih * nw;
    int rc = y2h_resize_chw(src, c, ih, iw, tmp, resized, nh, nw, s);
    if (rc) return rc;
    rc = y2h_fill(dst, (long)c * h * w, .5f, s);
    if (rc) return rc;
    return y2h_embed_chw(resized, c, nh, nw, dst, h, w, (w - nw) / 2, (h - nh) / 2, s);
}

// ---------------------------------------------------------------------------
// A batch of regions of any size in one launch: u8_to_planes + resize_cols + resize_rows (+ fill / embed when
// letterboxing) fused per output pixel.  The chain's intermediates are recomputed where they are needed, from the same
// expressions in the same order (this file is built with -ffp-contract=off):
//   plane value      lut[v] = (float)((double)v / 255.)                         u8_to_planes_kernel
//   column pass      (1-dx)*p[ix] + dx*p[ix+1], or p[iw-1] when col == nw-1 || iw == 1      resize_cols_kernel
//   row pass         (1-dy)*part(iy), + dy*part(iy+1) unless r == nh-1 || ih == 1            resize_rows_kernel
//   letterbox        .5 outside [dx, dx+nw) x [dy, dy+nh)                        fill_kernel + embed_kernel
// Each thread writes four consecutive pixels of one output row in every plane (one 16-byte store per plane when the
// rows allow it); one block row of the grid per batch slot, slots past n are zeroed.
// ---------------------------------------------------------------------------
struct RegionPix {                       // one source row of a region, one plane
    const unsigned char *row;
    int c;
    const float *lut;
    __device__ float at(int j) const { return lut[row[(size_t)j * c]]; }
};

__device__ __forceinline__ float region_col(const RegionPix &p, int col, int iw, int nw, float w_scale)
{
    if (col == nw - 1 || iw == 1) return p.at(iw - 1);
    const float sx = col * w_scale;
    const float dx = sx - (int)sx;
    const int ix = min((int)sx, iw - 2);     // never clamps for a host-computed scale; keeps the reads in the region
    return (1 - dx) * p.at(ix) + dx * p.at(ix + 1);
}

// NOTE: regions_to_input_filtered_kernel below is this kernel with one changed source read and must stay so, expression
// for expression (tests/test_gpu_depth.py::test_filter_off_is_ingest_regions compares them): edit both together.
__global__ __launch_bounds__(256) void regions_to_input_kernel(const y2h_region *__restrict__ desc, int n,
                                                               const unsigned char *__restrict__ pixels, int planes,
                                                               int swap_rb, int h, int w, int vec, float *__restrict__ dst)
{
    __shared__ float lut[256];
    const int b = blockIdx.y;
    const long gw = (w + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int Y = (int)(g / gw), X0 = (int)(g - (long)Y * gw) * 4;
    const size_t plane = (size_t)h * w;
    float *o = dst + (size_t)b * planes * plane + (size_t)Y * w + X0;
    const int nx = min(4, w - X0);
    if (b >= n) {                        // padded slot: deterministic zeros (uniform per block)
        if (Y >= h) return;
        for (int k = 0; k < planes; ++k) {
            if (vec) *(float4 *)(o + k * plane) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int i = 0; i < nx; ++i) o[k * plane + i] = 0.f;
        }
        return;
    }
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.);
    __syncthreads();
    if (Y >= h) return;
    const y2h_region d = desc[b];
    const unsigned char *src = pixels + d.src;
    const int y = Y - d.dy;
    const bool row_in = y >= 0 && y < d.nh;
    int iy = 0;
    float dy = 0.f;
    bool two = false;
    if (row_in) {
        const float sy = y * d.h_scale;
        iy = min(max((int)sy, 0), d.ih - 1);
        dy = sy - (int)sy;
        two = !(y == d.nh - 1 || d.ih == 1);
    }
    const int iy1 = min(iy + 1, d.ih - 1);
    for (int k = 0; k < planes; ++k) {
        int sk = k;
        if (swap_rb && d.c >= 3) sk = (k == 0) ? 2 : (k == 2 ? 0 : k);
        const RegionPix p0{src + (size_t)iy * d.pitch + sk, d.c, lut};
        const RegionPix p1{src + (size_t)iy1 * d.pitch + sk, d.c, lut};
        float v[4];
        for (int i = 0; i < 4; ++i) {
            const int x = X0 + i - d.dx;
            if (i >= nx || !row_in || x < 0 || x >= d.nw) { v[i] = .5f; continue; }
            float val = (1 - dy) * region_col(p0, x, d.iw, d.nw, d.w_scale);
            if (two) val = val + dy * region_col(p1, x, d.iw, d.nw, d.w_scale);
            v[i] = val;
        }
        if (vec) *(float4 *)(o + k * plane) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int i = 0; i < nx; ++i) o[k * plane + i] = v[i];
    }
}

extern "C" int y2h_regions_to_input(const y2h_region *desc, int n, const unsigned char *pixels, int batch, int planes,
                                    int swap_rb, int h, int w, float *dst, y2h_stream s)
{
    if (!desc || !pixels || !dst || n < 0 || n > batch || batch <= 0 || planes <= 0 || h <= 0 || w <= 0) return Y2H_EINVAL;
    const int vec = (w % 4 == 0) && ((uintptr_t)dst % 16 == 0);
    const long groups = (long)h * ((w + 3) / 4);
    hipLaunchKernelGGL(regions_to_input_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)batch), dim3(256), 0, S(s),
                       desc, n, pixels, planes, swap_rb, h, w, vec, dst);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// The same chain with the hand-crop distance filter (KinectUtil_with_cam.cpp:1866-1888, applied at :1022 / :1066 before
// the crop goes to the detector) on the source read: a pixel whose aligned 8-bit depth says "no depth" or "farther than
// the hand" reads as 255 in every plane; with the grasp filter (y2_depth_set_grasp_filter) so does a pixel whose grasp16
// is 0, i.e. one on the removed table plane or without depth.  Only the read differs, so an item without a filter -- and the padded slots --
// are formed by exactly the expressions of regions_to_input_kernel.
// ---------------------------------------------------------------------------
struct RegionPixF {                      // one source row of a region, one plane, with the row of depth8 under it
    const unsigned char *row;
    int c;
    const float *lut;
    const unsigned char *depth;          // depth8 under the region's pixel (row, 0), or NULL: no filter
    float far_limit;
    const unsigned short *grasp;         // grasp16 under the region's pixel (row, 0), or NULL: no grasp filter
    __device__ float at(int j) const
    {
        if (depth && y2_depth_whitens(depth[j], far_limit)) return lut[255];
        if (grasp && grasp[j] == 0) return lut[255];
        return lut[row[(size_t)j * c]];
    }
};

__device__ __forceinline__ float region_col_f(const RegionPixF &p, int col, int iw, int nw, float w_scale)
{
    if (col == nw - 1 || iw == 1) return p.at(iw - 1);
    const float sx = col * w_scale;
    const float dx = sx - (int)sx;
    const int ix = min((int)sx, iw - 2);
    return (1 - dx) * p.at(ix) + dx * p.at(ix + 1);
}

__global__ __launch_bounds__(256) void regions_to_input_filtered_kernel(const y2h_region_f *__restrict__ desc, int n,
                                                                        const unsigned char *__restrict__ pixels,
                                                                        const unsigned char *__restrict__ depth8,
                                                                        const unsigned short *__restrict__ grasp16, int W,
                                                                        int planes, int swap_rb, int h, int w, int vec,
                                                                        float *__restrict__ dst)
{
    __shared__ float lut[256];
    const int b = blockIdx.y;
    const long gw = (w + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int Y = (int)(g / gw), X0 = (int)(g - (long)Y * gw) * 4;
    const size_t plane = (size_t)h * w;
    float *o = dst + (size_t)b * planes * plane + (size_t)Y * w + X0;
    const int nx = min(4, w - X0);
    if (b >= n) {                        // padded slot: deterministic zeros (uniform per block)
        if (Y >= h) return;
        for (int k = 0; k < planes; ++k) {
            if (vec) *(float4 *)(o + k * plane) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int i = 0; i < nx; ++i) o[k * plane + i] = 0.f;
        }
        return;
    }
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.);
    __syncthreads();
    if (Y >= h) return;
    const y2h_region_f df = desc[b];
    const y2h_region d = df.r;
    const unsigned char *src = pixels + d.src;
    const int y = Y - d.dy;
    const bool row_in = y >= 0 && y < d.nh;
    int iy = 0;
    float dy = 0.f;
    bool two = false;
    if (row_in) {
        const float sy = y * d.h_scale;
        iy = min(max((int)sy, 0), d.ih - 1);
        dy = sy - (int)sy;
        two = !(y == d.nh - 1 || d.ih == 1);
    }
    const int iy1 = min(iy + 1, d.ih - 1);
    const bool filt = df.filter && depth8;
    const unsigned char *z0 = filt ? depth8 + (size_t)(df.fy + iy) * W + df.fx : nullptr;
    const unsigned char *z1 = filt ? depth8 + (size_t)(df.fy + iy1) * W + df.fx : nullptr;
    const bool gfilt = filt && grasp16;
    const unsigned short *g0 = gfilt ? grasp16 + (size_t)(df.fy + iy) * W + df.fx : nullptr;
    const unsigned short *g1 = gfilt ? grasp16 + (size_t)(df.fy + iy1) * W + df.fx : nullptr;
    for (int k = 0; k < planes; ++k) {
        int sk = k;
        if (swap_rb && d.c >= 3) sk = (k == 0) ? 2 : (k == 2 ? 0 : k);
        const RegionPixF p0{src + (size_t)iy * d.pitch + sk, d.c, lut, z0, df.far_limit, g0};
        const RegionPixF p1{src + (size_t)iy1 * d.pitch + sk, d.c, lut, z1, df.far_limit, g1};
        float v[4];
        for (int i = 0; i < 4; ++i) {
            const int x = X0 + i - d.dx;
            if (i >= nx || !row_in || x < 0 || x >= d.nw) { v[i] = .5f; continue; }
            float val = (1 - dy) * region_col_f(p0, x, d.iw, d.nw, d.w_scale);
            if (two) val = val + dy * region_col_f(p1, x, d.iw, d.nw, d.w_scale);
            v[i] = val;
        }
        if (vec) *(float4 *)(o + k * plane) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int i = 0; i < nx; ++i) o[k * plane + i] = v[i];
    }
}

extern "C" int y2h_regions_to_input_grasp(const y2h_region_f *desc, int n, const unsigned char *pixels,
                                          const unsigned char *depth8, const unsigned short *grasp16, int W, int batch,
                                          int planes, int swap_rb, int h, int w, float *dst, y2h_stream s)
{
    if (!desc || !pixels || !dst || n < 0 || n > batch || batch <= 0 || planes <= 0 || h <= 0 || w <= 0 || (depth8 && W <= 0) ||
        (grasp16 && !depth8))
        return Y2H_EINVAL;
    const int vec = (w % 4 == 0) && ((uintptr_t)dst % 16 == 0);
    const long groups = (long)h * ((w + 3) / 4);
    hipLaunchKernelGGL(regions_to_input_filtered_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)batch), dim3(256), 0,
                       S(s), desc, n, pixels, depth8, grasp16, W, planes, swap_rb, h, w, vec, dst);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_regions_to_input_filtered(const y2h_region_f *desc, int n, const unsigned char *pixels,
                                             const unsigned char *depth8, int W, int batch, int planes, int swap_rb, int h,
                                             int w, float *dst, y2h_stream s)
{
    return y2h_regions_to_input_grasp(desc, n, pixels, depth8, nullptr, W, batch, planes, swap_rb, h, w, dst, s);
}

// ---------------------------------------------------------------------------
// Classifier views (classifier.c:336-593): a batch of crop_image windows (image.c:1512-1532, constrain_int taps: edge
// pixels repeat) of CHW float images of any size, optionally taken after flip_image (image.c:1056-1070), in one
// launch.  Pure data movement: one read and one write per value.  Each thread writes four consecutive pixels of one
// output row in every plane -- one 16-byte store per plane when the rows allow it, and one 16-byte load when its four
// taps are four consecutive, aligned source pixels (an unflipped window's interior); one block row of the grid per
// batch slot, slots past n are zeroed.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void views_to_input_kernel(const y2h_view *__restrict__ desc, int n,
                                                             const float *__restrict__ src, int planes, int h, int w,
                                                             int vec, float *__restrict__ dst)
{
    const int b = blockIdx.y;
    const long gw = (w + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int Y = (int)(g / gw), X0 = (int)(g - (long)Y * gw) * 4;
    if (Y >= h) return;
    const size_t plane = (size_t)h * w;
    float *o = dst + (size_t)b * planes * plane + (size_t)Y * w + X0;
    const int nx = min(4, w - X0);
    if (b >= n) {                        // padded slot: deterministic zeros (uniform per block)
        for (int k = 0; k < planes; ++k) {
            if (vec) *(float4 *)(o + k * plane) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int i = 0; i < nx; ++i) o[k * plane + i] = 0.f;
        }
        return;
    }
    const y2h_view d = desc[b];
    const size_t splane = (size_t)d.sh * d.sw;
    const int r = min(max(Y + d.dy, 0), d.sh - 1);
    const float *row = src + d.src + (size_t)r * d.sw;
    int c[4];
    for (int i = 0; i < 4; ++i) {
        c[i] = min(max(X0 + i + d.dx, 0), d.sw - 1);
        if (d.flip) c[i] = d.sw - 1 - c[i];
    }
    // four consecutive source pixels (no clamp hit, no flip): the clamped taps are then c[0] .. c[0] + 3
    const bool run = !d.flip && X0 + d.dx >= 0 && X0 + 3 + d.dx <= d.sw - 1;
    for (int k = 0; k < planes; ++k) {
        const float *p = row + k * splane;
        float v[4];
        if (run && ((uintptr_t)(p + c[0]) % 16 == 0)) {
            const float4 q = *(const float4 *)(p + c[0]);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int i = 0; i < 4; ++i) v[i] = p[c[i]];
        }
        if (vec) *(float4 *)(o + k * plane) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int i = 0; i < nx; ++i) o[k * plane + i] = v[i];
    }
}

extern "C" int y2h_views_to_input(const y2h_view *desc, int n, const float *src, int batch, int planes, int h, int w,
                                  float *dst, y2h_stream s)
{
    if (!dst || n < 0 || n > batch || batch <= 0 || planes <= 0 || h <= 0 || w <= 0 || (n > 0 && (!desc || !src)))
        return Y2H_EINVAL;
    const int vec = (w % 4 == 0) && ((uintptr_t)dst % 16 == 0);
    const long groups = (long)h * ((w + 3) / 4);
    hipLaunchKernelGGL(views_to_input_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)batch), dim3(256), 0, S(s),
                       desc, n, src, planes, h, w, vec, dst);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// acc[owner[s]][j] = acc[owner[s]][j] + rows[s][j] for s ascending (axpy_cpu(classes, 1, p, 1, pred, 1),
// classifier.c:393,577,580).  One thread per column j walks the slots in order, so no two threads touch the same value
// and every accumulator receives its additions in slot order, one rounding each, whatever the launch shape.  A slot
// whose owner is negative is not read.
__global__ __launch_bounds__(256) void accumulate_rows_kernel(float *acc, const float *__restrict__ rows, int ld,
                                                              const int *__restrict__ owner, int nslots, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (int s = 0; s < nslots; ++s) {
        const int o = owner[s];
        if (o < 0) continue;
        float *a = acc + (size_t)o * n + j;
        *a = *a + rows[(size_t)s * ld + j];
    }
}

extern "C" int y2h_accumulate_rows(float *acc, const float *rows, int ld, const int *owner, int nslots, int n, y2h_stream s)
{
    if (!acc || !rows || !owner || nslots <= 0 || n <= 0 || ld < n) return Y2H_EINVAL;
    hipLaunchKernelGGL(accumulate_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(s), acc, rows, ld, owner,
                       nslots, n);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// utils.c:420-432 mean_arrays on device buffers: avg = 0; for j: avg += frame j; avg /= n  (fp32, frame order)
__global__ __launch_bounds__(256) void mean_frames_kernel(const float *__restrict__ frames, int n, long els, float *__restrict__ avg)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < els; i += (long)gridDim.x * 256) {
        float a = 0.f;
        for (int j = 0; j < n; ++j) a += frames[(size_t)j * els + i];
        avg[i] = a / n;
    }
}

extern "C" int y2h_mean_frames(const float *frames, int n, long els, float *avg, y2h_stream s)
{
    if (!frames || !avg || n <= 0 || els <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(mean_frames_kernel, dim3(y2h_grid(els, 256)), dim3(256), 0, S(s), frames, n, els, avg);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
