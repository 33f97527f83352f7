// y2_augment.hip -- the pixel half of load_data_detection (data.c:676-711) on the device: one launch turns a batch of
// 8-bit frames and their draws into the trainer's dense NHWC input; behind it the classifier loader's
// (load_image_augment_paths, data.c:107-132), the same way.  Reference behaviour restated, per output pixel and in
// the reference's order (this file is built with -ffp-contract=off; every line below is one IEEE operation of the C code):
//   plane value      lut[v] = (float)((double)v / 255.)                                     image.c:2045-2067
//   crop_image       tap (i + pleft, j + ptop), both coordinates through constrain_int       image.c:1512-1532
//   column pass      (1-dx)*p[ix] + dx*p[ix+1], or p[im.w-1] when c == w-1 || im.w == 1      image.c:1957-1972
//   row pass         (1-dy)*part(iy), + dy*part(iy+1) unless r == h-1 || im.h == 1           image.c:1973-1988
//   flip_image       output column x reads sized column w-1-x                                image.c:1056-1070
//   rgb_to_hsv       max == 0 -> h = s = 0; h/6. is a double division                        image.c:1718-1753
//   distort_image    s*dsat, v*dexp, h + dhue, > 1 -> -1, < 0 -> +1                          image.c:1903-1913
//   hsv_to_rgb       floor(6h), six branches, index 6 falls into the last                    image.c:1755-1794
//   constrain_image  < 0 -> 0, > 1 -> 1                                                      image.c:1115-1122
// A grey pixel's hue is 0/0; it is carried and never read, because its saturation is 0.
// Neither kernel is bound by its bytes (12 bytes written per pixel, the touched source bytes read through the caches): they
// measure 5 to 8 times their byte floors (profiles/train_loader.txt, profiles/train_loader_cls.txt), which the arithmetic
// of one IEEE operation per C operation and the byte gathers are supposed to explain; no counter run was made.  Each thread
// forms four consecutive pixels of one output row (48 bytes) and stores them as three 16-byte words where the group is
// whole and its address allows, as single floats otherwise.
#include "y2_common.hpp"

__device__ __forceinline__ int aug_clamp(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

// image.c:1718-1794 with distort_image between the two conversions, for one pixel
__device__ __forceinline__ void aug_distort(float &r, float &g, float &b, float dhue, float dsat, float dexp)
{
    const float mx = (r > g) ? ((r > b) ? r : b) : ((g > b) ? g : b);
    const float mn = (r < g) ? ((r < b) ? r : b) : ((g < b) ? g : b);
    const float delta = mx - mn;
    float h, s, v = mx;
    if (mx == 0) {
        s = 0;
        h = 0;
    } else {
        s = delta / mx;
        if (r == mx) h = (g - b) / delta;
        else if (g == mx) h = 2 + (b - r) / delta;
        else h = 4 + (r - g) / delta;
        if (h < 0) h += 6;
        h = (float)((double)h / 6.);
    }
    s = s * dsat;
    v = v * dexp;
    h = h + dhue;
    if (h > 1) h -= 1;
    if (h < 0) h += 1;
    h = 6 * h;
    if (s == 0) {
        r = g = b = v;
    } else {
        const int index = (int)floorf(h);
        const float f = h - index;
        const float p = v * (1 - s);
        const float q = v * (1 - s * f);
        const float t = v * (1 - s * (1 - f));
        if (index == 0) { r = v; g = t; b = p; }
        else if (index == 1) { r = q; g = v; b = p; }
        else if (index == 2) { r = p; g = v; b = t; }
        else if (index == 3) { r = p; g = q; b = v; }
        else if (index == 4) { r = t; g = p; b = v; }
        else { r = v; g = p; b = q; }
    }
    if (r < 0) r = 0;
    if (r > 1) r = 1;
    if (g < 0) g = 0;
    if (g > 1) g = 1;
    if (b < 0) b = 0;
    if (b > 1) b = 1;
}

__global__ __launch_bounds__(256) void augment_to_input_kernel(const y2h_aug *__restrict__ desc, const unsigned char *__restrict__ pixels,
                                                               int swap_rb, int h, int w, float *__restrict__ dst)
{
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.);
    __syncthreads();
    const int b = blockIdx.y;
    const long gw = (w + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int Y = (int)(g / gw), X0 = (int)(g - (long)Y * gw) * 4;
    if (Y >= h) return;
    const int nx = min(4, w - X0);
    const y2h_aug d = desc[b];
    const unsigned char *src = pixels + d.src;
    // the row pass reads two rows of the column pass's image, which has the cropped image's rows
    const float sy = Y * d.h_scale;
    const int iy = aug_clamp((int)sy, 0, d.sheight - 1);    // never clamps for a host-computed scale
    const float dy = sy - (int)sy;
    const bool two = !(Y == h - 1 || d.sheight == 1);
    const int r0 = aug_clamp(aug_clamp(iy + d.ptop, 0, d.oh - 1) - d.y0, 0, d.rh - 1);
    const int r1 = aug_clamp(aug_clamp(iy + 1 + d.ptop, 0, d.oh - 1) - d.y0, 0, d.rh - 1);
    const unsigned char *row0 = src + (size_t)r0 * d.pitch;
    const unsigned char *row1 = src + (size_t)r1 * d.pitch;
    const int k0 = swap_rb ? 2 : 0, k2 = swap_rb ? 0 : 2;
    float v[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float rgb[3] = {0.f, 0.f, 0.f};
        if (i < nx) {
            const int X = X0 + i;
            const int col = d.flip ? w - 1 - X : X;
            const bool last = col == w - 1 || d.swidth == 1;
            int ix = d.swidth - 1;
            float dx = 0.f;
            if (!last) {
                const float sx = col * d.w_scale;
                ix = (int)sx;
                dx = sx - ix;
            }
            const size_t c0 = (size_t)aug_clamp(aug_clamp(ix + d.pleft, 0, d.ow - 1) - d.x0, 0, d.rw - 1) * d.c;
            const size_t c1 = (size_t)aug_clamp(aug_clamp(ix + 1 + d.pleft, 0, d.ow - 1) - d.x0, 0, d.rw - 1) * d.c;
            for (int k = 0; k < 3; ++k) {
                const int sk = k == 0 ? k0 : (k == 2 ? k2 : 1);
                float part0, part1 = 0.f;
                if (last) {
                    part0 = lut[row0[c0 + sk]];
                    if (two) part1 = lut[row1[c0 + sk]];
                } else {
                    part0 = (1 - dx) * lut[row0[c0 + sk]] + dx * lut[row0[c1 + sk]];
                    if (two) part1 = (1 - dx) * lut[row1[c0 + sk]] + dx * lut[row1[c1 + sk]];
                }
                float val = (1 - dy) * part0;
                if (two) val = val + dy * part1;
                rgb[k] = val;
            }
            aug_distort(rgb[0], rgb[1], rgb[2], d.dhue, d.dsat, d.dexp);
        }
        v[3 * i] = rgb[0]; v[3 * i + 1] = rgb[1]; v[3 * i + 2] = rgb[2];
    }
    float *o = dst + (((size_t)b * h + Y) * w + X0) * 3;
    if (nx == 4 && (uintptr_t)o % 16 == 0) {
        float4 *o4 = (float4 *)o;
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * nx) o[i] = v[i];
    }
}

// ---- the classifier loader: load_image_augment_paths (data.c:107-132) ----
//   rotate_crop_image     rx, ry in double, the expression's own order, rounded to float           image.c:1462-1479
//   bilinear_interpolate  floorf, float weights, four taps summed left to right                   image.c:1935-1948
//   get_pixel_extend      x and y clamped into the frame                                          image.c:2112-2120
//   flip_image on the crop, then distort_image and constrain_image as above
// (x - w/2.)/s*aspect stays a double division per pixel, (y - h/2.)/s one per thread (a thread's pixels share a row);
// dx/s*aspect and dy/s are float operations of the C line, made once per image on the host.  The source is gathered byte
// by byte along a rotated line, so neighbouring threads share cache lines only as far as the angle lets them.
__global__ __launch_bounds__(256) void augment_cls_to_input_kernel(const y2h_aug_cls *__restrict__ desc, const unsigned char *__restrict__ pixels,
                                                                   int swap_rb, int size, float *__restrict__ dst)
{
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.);
    __syncthreads();
    const int b = blockIdx.y;
    const long gw = (size + 3) / 4;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int Y = (int)(g / gw), X0 = (int)(g - (long)Y * gw) * 4;
    if (Y >= size) return;
    const int nx = min(4, size - X0);
    const y2h_aug_cls d = desc[b];
    const unsigned char *src = pixels + d.src;
    const double half = size / 2.;
    const double vy = (Y - half) / d.s + d.ay;              // (y - h/2.)/s + dy/s
    const double sv = d.sinr * vy, cv = d.cosr * vy;
    const int k0 = swap_rb ? 2 : 0, k2 = swap_rb ? 0 : 2;
    float v[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float rgb[3] = {0.f, 0.f, 0.f};
        if (i < nx) {
            const int X = X0 + i;
            const int col = d.flip ? size - 1 - X : X;
            const double ux = (col - half) / d.s * d.aspect + d.ax;     // (x - w/2.)/s*aspect + dx/s*aspect
            const float rx = (float)(d.cosr * ux - sv + (double)d.cx);
            const float ry = (float)(d.sinr * ux + cv + (double)d.cy);
            const int ix = (int)floorf(rx), iy = (int)floorf(ry);       // the conversion saturates; the clamps below take it from there
            const float dx = rx - ix, dy = ry - iy;
            const float w00 = (1 - dy) * (1 - dx), w01 = dy * (1 - dx), w10 = (1 - dy) * dx, w11 = dy * dx;
            const int ix1 = ix == 0x7fffffff ? ix : ix + 1, iy1 = iy == 0x7fffffff ? iy : iy + 1;
            const size_t c0 = (size_t)aug_clamp(aug_clamp(ix, 0, d.ow - 1) - d.x0, 0, d.rw - 1) * d.c;
            const size_t c1 = (size_t)aug_clamp(aug_clamp(ix1, 0, d.ow - 1) - d.x0, 0, d.rw - 1) * d.c;
            const unsigned char *row0 = src + (size_t)aug_clamp(aug_clamp(iy, 0, d.oh - 1) - d.y0, 0, d.rh - 1) * d.pitch;
            const unsigned char *row1 = src + (size_t)aug_clamp(aug_clamp(iy1, 0, d.oh - 1) - d.y0, 0, d.rh - 1) * d.pitch;
            for (int k = 0; k < 3; ++k) {
                const int sk = k == 0 ? k0 : (k == 2 ? k2 : 1);
                rgb[k] = w00 * lut[row0[c0 + sk]] + w01 * lut[row1[c0 + sk]] + w10 * lut[row0[c1 + sk]] + w11 * lut[row1[c1 + sk]];
            }
            aug_distort(rgb[0], rgb[1], rgb[2], d.dhue, d.dsat, d.dexp);
        }
        v[3 * i] = rgb[0]; v[3 * i + 1] = rgb[1]; v[3 * i + 2] = rgb[2];
    }
    float *o = dst + (((size_t)b * size + Y) * size + X0) * 3;
    if (nx == 4 && (uintptr_t)o % 16 == 0) {
        float4 *o4 = (float4 *)o;
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * nx) o[i] = v[i];
    }
}

extern "C" int y2h_augment_cls_to_input(const y2h_aug_cls *desc, int n, const unsigned char *pixels, int swap_rb, int size,
                                        float *dst_nhwc, y2h_stream s)
{
    if (!desc || !pixels || !dst_nhwc || n <= 0 || n > 65535 || size <= 0) return Y2H_EINVAL;
    const long groups = (long)size * ((size + 3) / 4);
    hipLaunchKernelGGL(augment_cls_to_input_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)n), dim3(256), 0, S(s), desc, pixels,
                       swap_rb, size, dst_nhwc);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_augment_to_input(const y2h_aug *desc, int n, const unsigned char *pixels, int swap_rb, int h, int w,
                                    float *dst_nhwc, y2h_stream s)
{
    if (!desc || !pixels || !dst_nhwc || n <= 0 || n > 65535 || h <= 0 || w <= 0) return Y2H_EINVAL;
    const long groups = (long)h * ((w + 3) / 4);
    hipLaunchKernelGGL(augment_to_input_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)n), dim3(256), 0, S(s), desc, pixels,
                       swap_rb, h, w, dst_nhwc);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
