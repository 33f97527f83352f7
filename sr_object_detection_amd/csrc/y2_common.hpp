// Shared helpers for the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <utility>
#include "y2_hip.h"

extern "C" void y2h_set_error_(const char *what, const char *detail);

#define Y2H_CHECK(expr)                                                      \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            y2h_set_error_(#expr, hipGetErrorString(e_));                    \
            return Y2H_EHIP;                                                 \
        }                                                                    \
    } while (0)

#define Y2H_LAUNCH_CHECK()                                                   \
    do {                                                                     \
        hipError_t e_ = hipGetLastError();                                   \
        if (e_ != hipSuccess) {                                              \
            y2h_set_error_("kernel launch", hipGetErrorString(e_));          \
            return Y2H_EHIP;                                                 \
        }                                                                    \
    } while (0)

static inline hipStream_t S(y2h_stream s) { return (hipStream_t)s; }

// memory-bound elementwise launches: cap the grid and grid-stride the rest
static inline unsigned y2h_grid(long n, int block, int max_blocks = 256 * 16)
{
    long g = (n + block - 1) / block;
    if (g > max_blocks) g = max_blocks;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// The two storage types of an activation, fp32 and IEEE half (fp16 mode), for the layer kernels that have one body for
// both: the vector of one 16-byte access, how many elements it holds, and the most negative finite value.
template <typename T> struct storage;
template <> struct storage<float> {
    typedef float vec __attribute__((ext_vector_type(4)));
    static constexpr int VEC = 4;
    static constexpr float LOWEST = -FLT_MAX;
};
template <> struct storage<_Float16> {
    typedef _Float16 vec __attribute__((ext_vector_type(8)));
    static constexpr int VEC = 8;
    static constexpr float LOWEST = -65504.f;
};

// 16-byte accesses to rows of c elements at leading dimensions ldx, ldy (counted in elements) are possible
template <typename T>
static inline bool y2h_vec_ok(int c, int ldx, int ldy, const void *x, const void *y)
{
    constexpr int V = storage<T>::VEC;
    return (c % V == 0) && (ldx % V == 0) && (ldy % V == 0) && (((uintptr_t)x | (uintptr_t)y) % 16 == 0);
}

// Dynamic LDS above the default needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel, per device.  The attribute
// call is not free, so the largest size granted so far is remembered per (kernel, device) and the call is made only when
// a launch asks for more.  One table for the whole library (inline: shared by every translation unit), safe to call from
// several threads.
inline hipError_t y2h_lds_limit(const void *fn, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = granted[{fn, dev}];
    if (have >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

// softmax of one row or one tree group by one thread (src_yolo2/blas.c:205-221): max-subtract, exp in double, fp32 running
// sum in index order, divide -- the summation order is the reference's.  in / out may be the same pointer.
__device__ __forceinline__ void softmax_seq(const float *in, int n, float temp, float *out)
{
    float sum = 0.f, largest = -FLT_MAX;
    for (int i = 0; i < n; ++i) if (in[i] > largest) largest = in[i];
    for (int i = 0; i < n; ++i) {
        const float e = (float)exp((double)(in[i] / temp - largest / temp));
        sum += e;
        out[i] = e;
    }
    for (int i = 0; i < n; ++i) out[i] /= sum;
}

// every activation of activations.h:21-54, with the reference's own promotion rules (float x, double constants, the
// result rounded to float on return)
__device__ inline float activate_any(float x, int act)
{
    const double xd = (double)x;
    switch (act) {
    case Y2H_ACT_LINEAR: return x;
    case Y2H_ACT_LEAKY: return (x > 0) ? x : (float)(.1 * xd);
    case Y2H_ACT_LOGISTIC: return (float)(1. / (1. + exp(-xd)));
    case Y2H_ACT_RELU: return x * (float)(x > 0);
    case Y2H_ACT_RELIE: return (x > 0) ? x : (float)(.01 * xd);
    case Y2H_ACT_RAMP: return (float)((double)(x * (float)(x > 0)) + .1 * xd);
    case Y2H_ACT_TANH: { const float t = 2 * x; return (float)((exp((double)t) - 1) / (exp((double)t) + 1)); }
    case Y2H_ACT_PLSE:
        if (x < -4) return (float)(.01 * (double)(x + 4));
        if (x > 4) return (float)(.01 * (double)(x - 4) + 1);
        return (float)(.125 * xd + .5);
    case Y2H_ACT_ELU: return (float)((double)((float)(x >= 0) * x) + (double)(x < 0) * (exp(xd) - 1));
    case Y2H_ACT_LOGGY: return (float)(2. / (1. + exp(-xd)) - 1);
    case Y2H_ACT_STAIR: {
        const int n = (int)floor(xd);
        if (n % 2 == 0) return (float)floor(xd / 2.);
        return (float)((double)(x - (float)n) + floor(xd / 2.));
    }
    case Y2H_ACT_HARDTAN: return x < -1 ? -1.f : (x > 1 ? 1.f : x);
    case Y2H_ACT_LHTAN:
        if (x < 0) return (float)(.001 * xd);
        if (x > 1) return (float)(.001 * (double)(x - 1) + 1);
        return x;
    }
    return x;
}
