// y2_plane.hip -- the table-plane removal of the Kinect loop's Grasp branch on the device: what desk_seg
// (KinectUtil_with_cam.cpp:1931-1974) does on the host per frame with PCL's RANSAC (plane_seg.cpp:157-213) -- clip the
// depth frame, form the cloud, find the dominant plane, refit it to its inliers, zero the pixels on it -- restated as the
// deterministic rule of include/y2_plane_rule.h, which this file and the host both compile.
//   count     every hypothesis against every point: integer counts, so arrival order cannot change a value
//   sums      the ten refit sums of the best hypothesis' inliers, in doubles through the header's fixed tree
//   fit       the slab of chunk partials through the tree's last levels, the header's eigen routine, the plane record
//   apply     the dh x dw grasp depth and the number of removed pixels
//   register  the H x W grasp16 plane, gathered through the dxy plane of depth_align_kernel
// All five share one pixel layout: a thread owns four consecutive depth pixels of the flat index, a workgroup one chunk
// of 1024 (Y2_PLANE_CHUNK), which is also a chunk of the tree.  Built with -ffp-contract=off.
#include "y2_common.hpp"
#include "y2_plane_rule.h"

typedef unsigned long long u64;

static_assert(Y2_PLANE_CHUNK == 1024 && Y2_PLANE_MAX_ITERS == 256, "the kernels are written for 256 threads of 4 pixels");
static_assert(Y2H_PLANE_COUNTS > Y2_PLANE_MAX_ITERS, "counts[Y2_PLANE_MAX_ITERS] holds the valid points");

struct Px4 {
    float p[4][3];                       // camera-space points (of the valid pixels)
    unsigned short g[4];                 // clipped depth, 0 = not valid (also past the frame's end)
    int nx;                              // pixels of this thread inside the frame
};

// the four pixels of this thread: one 8-byte load of depth and two 16-byte loads of the table where all four exist
__device__ __forceinline__ long plane_load4(const y2h_plane_job &q, Px4 &v)
{
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned short d[4] = {0, 0, 0, 0};
    float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    v.nx = i0 >= q.n ? 0 : (int)min(4L, q.n - i0);
    if (v.nx == 4) {
        const ushort4 dd = *(const ushort4 *)(q.depth + i0);
        const float4 a = *(const float4 *)(q.tab + 2 * i0), b = *(const float4 *)(q.tab + 2 * i0 + 4);
        d[0] = dd.x; d[1] = dd.y; d[2] = dd.z; d[3] = dd.w;
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
    } else {
        for (int j = 0; j < v.nx; ++j) { d[j] = q.depth[i0 + j]; t[2 * j] = q.tab[2 * (i0 + j)]; t[2 * j + 1] = q.tab[2 * (i0 + j) + 1]; }
    }
    for (int j = 0; j < 4; ++j) {
        v.g[j] = j < v.nx ? y2_plane_clip(d[j], q.far_mm) : (unsigned short)0;
        y2_plane_point(v.g[j], t[2 * j], t[2 * j + 1], v.p[j]);
    }
    return i0;
}

// the best hypothesis from the finished counts: the largest count, a tie to the lowest k.  Every thread of the
// workgroup calls it and gets the same answer; false: no plane (fewer than 3 valid points or a best count below 3).
__device__ __forceinline__ bool plane_pick(const y2h_plane_job &q, u64 *red, int &best, int &count)
{
    const int tid = threadIdx.x;
    red[tid] = tid < q.iters ? ((u64)(unsigned)q.counts[tid] << 32) | (u64)(0xFFFFFFFFu - (unsigned)tid) : 0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
        __syncthreads();
    }
    const u64 key = red[0];
    count = (int)(key >> 32);
    best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
    return q.counts[Y2_PLANE_MAX_ITERS] >= 3 && count >= 3;
}

// grid (chunks, shares): the workgroups of a chunk split the hypotheses between them (k = share, share + shares, ...), as a
// chunk is one wave per SIMD and the walk over the hypotheses is a chain of dependent operations; share 0 also counts the
// valid points.  A hypothesis' LDS slot is touched by its own share only.
__global__ __launch_bounds__(256) void plane_count_kernel(y2h_plane_job q)
{
    __shared__ y2_plane_hyp hyp[Y2_PLANE_MAX_ITERS];
    __shared__ int cnt[4][Y2_PLANE_MAX_ITERS + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int share = blockIdx.y, shares = gridDim.y;
    if (tid < q.iters && tid % shares == share) y2_plane_of_triple(q.depth, q.tab, q.n, q.far_mm, q.triples + 3 * tid, &hyp[tid]);
    Px4 v;
    plane_load4(q, v);
    __syncthreads();
    if (share == 0) {
        int c = 0;
        for (int j = 0; j < 4; ++j) c += __popcll(__ballot(v.g[j] > 0));
        if (lane == 0) cnt[wave][Y2_PLANE_MAX_ITERS] = c;
    }
    for (int k = share; k < q.iters; k += shares) {
        const y2_plane_hyp h = hyp[k];
        int c = 0;
        if (h.ok)                                        // uniform: a void hypothesis counts nothing
            for (int j = 0; j < 4; ++j) c += __popcll(__ballot(v.g[j] > 0 && y2_plane_inlier(&h, v.p[j], q.dist_m)));
        if (lane == 0) cnt[wave][k] = c;
    }
    __syncthreads();
    if (tid < q.iters && tid % shares == share) {
        const int s = cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
        if (s) atomicAdd(&q.counts[tid], s);
    }
    if (tid == 255 && share == 0) {
        const int s = cnt[0][Y2_PLANE_MAX_ITERS] + cnt[1][Y2_PLANE_MAX_ITERS] + cnt[2][Y2_PLANE_MAX_ITERS] + cnt[3][Y2_PLANE_MAX_ITERS];
        if (s) atomicAdd(&q.counts[Y2_PLANE_MAX_ITERS], s);
    }
}

__global__ __launch_bounds__(256) void plane_sums_kernel(y2h_plane_job q)
{
    __shared__ u64 red[256];
    __shared__ double A[10][256];
    __shared__ y2_plane_hyp hb;
    const int tid = threadIdx.x;
    int best, count;
    if (!plane_pick(q, red, best, count)) return;        // uniform
    if (tid == 0) y2_plane_of_triple(q.depth, q.tab, q.n, q.far_mm, q.triples + 3 * best, &hb);
    Px4 v;
    plane_load4(q, v);
    __syncthreads();
    const y2_plane_hyp h = hb;
    double acc[10];
    for (int j = 0; j < 4; ++j) {                        // the leaf: ((v0 + v1) + v2) + v3
        double t[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (v.g[j] > 0 && y2_plane_inlier(&h, v.p[j], q.dist_m)) y2_plane_terms(v.p[j], t);
        for (int k = 0; k < 10; ++k) acc[k] = j ? acc[k] + t[k] : t[k];
    }
    for (int k = 0; k < 10; ++k) A[k][tid] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {                  // the chunk
        if (tid < s) for (int k = 0; k < 10; ++k) A[k][tid] = A[k][tid] + A[k][tid + s];
        __syncthreads();
    }
    if (tid < 10) q.slab[(size_t)blockIdx.x * 10 + tid] = A[tid][0];
}

__global__ __launch_bounds__(256) void plane_fit_kernel(y2h_plane_job q, int chunks)
{
    __shared__ u64 red[256];
    __shared__ double A[10][256];
    __shared__ double S[10];
    const int tid = threadIdx.x;
    int best, count;
    const bool any = plane_pick(q, red, best, count);
    if (any)                                             // uniform.  The total: a tree over every 256 chunks, the groups in order
        for (int base = 0; base < chunks; base += 256) {
            for (int k = 0; k < 10; ++k) A[k][tid] = base + tid < chunks ? q.slab[(size_t)(base + tid) * 10 + k] : 0.0;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) for (int k = 0; k < 10; ++k) A[k][tid] = A[k][tid] + A[k][tid + s];
                __syncthreads();
            }
            if (tid < 10) S[tid] = base ? S[tid] + A[tid][0] : A[tid][0];
            __syncthreads();
        }
    if (tid != 0) return;
    y2h_plane r;
    double pl[4] = {0.0, 0.0, 0.0, 0.0};
    r.found = any ? y2_plane_fit_sums(S, pl) : 0;
    r.best = r.found ? best : -1;
    r.valid_points = q.counts[Y2_PLANE_MAX_ITERS];
    r.best_count = r.found ? count : 0;
    r.removed = 0; r.pad_ = 0;
    r.a = pl[0]; r.b = pl[1]; r.c = pl[2]; r.d = pl[3];
    *q.rec = r;
}

__global__ __launch_bounds__(256) void plane_apply_kernel(y2h_plane_job q)
{
    __shared__ int cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int found = q.rec->found;
    const double pl[4] = {q.rec->a, q.rec->b, q.rec->c, q.rec->d};
    Px4 v;
    const long i0 = plane_load4(q, v);
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        const bool gone = found && v.g[j] > 0 && y2_plane_removes(pl, v.p[j], q.dist_m);
        c += __popcll(__ballot(gone));
        if (gone) v.g[j] = 0;
    }
    if (lane == 0) cnt[wave] = c;
    if (v.nx == 4) *(ushort4 *)(q.grasp_depth + i0) = make_ushort4(v.g[0], v.g[1], v.g[2], v.g[3]);
    else for (int j = 0; j < v.nx; ++j) q.grasp_depth[i0 + j] = v.g[j];
    __syncthreads();
    if (tid == 0) {
        const int s = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        if (s) atomicAdd(&q.rec->removed, s);
    }
}

extern "C" unsigned long y2h_plane_chunks(long n) { return (unsigned long)((n + Y2_PLANE_CHUNK - 1) / Y2_PLANE_CHUNK); }

extern "C" int y2h_plane_remove(const y2h_plane_job *j, int stages, y2h_stream s)
{
    if (!j || !j->depth || !j->tab || !j->triples || !j->counts || !j->slab || !j->rec || !j->grasp_depth) return Y2H_EINVAL;
    if (j->n <= 0 || j->n > (1L << 30) || j->iters < 1 || j->iters > Y2_PLANE_MAX_ITERS) return Y2H_EINVAL;
    if ((uintptr_t)j->depth % 8 || (uintptr_t)j->grasp_depth % 8 || (uintptr_t)j->tab % 16 || (uintptr_t)j->slab % 8 ||
        (uintptr_t)j->rec % 8 || (uintptr_t)j->counts % 4 || (uintptr_t)j->triples % 4)
        return Y2H_EINVAL;
    const unsigned chunks = (unsigned)y2h_plane_chunks(j->n);
    if (stages & Y2H_PLANE_CLEAR) Y2H_CHECK(hipMemsetAsync(j->counts, 0, Y2H_PLANE_COUNTS * sizeof(int), S(s)));
    if (stages & Y2H_PLANE_COUNT) {
        hipLaunchKernelGGL(plane_count_kernel, dim3(chunks, j->iters < 4 ? j->iters : 4), dim3(256), 0, S(s), *j);
        Y2H_LAUNCH_CHECK();
    }
    if (stages & Y2H_PLANE_SUMS) {
        hipLaunchKernelGGL(plane_sums_kernel, dim3(chunks), dim3(256), 0, S(s), *j);
        Y2H_LAUNCH_CHECK();
    }
    if (stages & Y2H_PLANE_FIT) {
        hipLaunchKernelGGL(plane_fit_kernel, dim3(1), dim3(256), 0, S(s), *j, (int)chunks);
        Y2H_LAUNCH_CHECK();
    }
    if (stages & Y2H_PLANE_APPLY) {
        hipLaunchKernelGGL(plane_apply_kernel, dim3(chunks), dim3(256), 0, S(s), *j);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}

// grasp16 of a colour pixel: the grasp depth under its (dx, dy), 0 where it maps nowhere (:415-421)
__global__ __launch_bounds__(256) void plane_register_kernel(const unsigned short *__restrict__ grasp_depth,
                                                             const short *__restrict__ dxy, long total, int dw,
                                                             unsigned short *__restrict__ grasp16)
{
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    const int nx = (int)min(4L, total - i0);
    short xy[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    if (nx == 4) {
        const short4 a = *(const short4 *)(dxy + 2 * i0), b = *(const short4 *)(dxy + 2 * i0 + 4);
        xy[0] = a.x; xy[1] = a.y; xy[2] = a.z; xy[3] = a.w; xy[4] = b.x; xy[5] = b.y; xy[6] = b.z; xy[7] = b.w;
    } else {
        for (int k = 0; k < nx; ++k) { xy[2 * k] = dxy[2 * (i0 + k)]; xy[2 * k + 1] = dxy[2 * (i0 + k) + 1]; }
    }
    unsigned short v[4];
    for (int k = 0; k < 4; ++k) v[k] = xy[2 * k] >= 0 ? grasp_depth[(size_t)xy[2 * k + 1] * dw + xy[2 * k]] : (unsigned short)0;
    if (nx == 4) *(ushort4 *)(grasp16 + i0) = make_ushort4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; k < nx; ++k) grasp16[i0 + k] = v[k];
}

extern "C" int y2h_plane_register(const unsigned short *grasp_depth, const short *dxy, int H, int W, int dw,
                                  unsigned short *grasp16, y2h_stream s)
{
    if (!grasp_depth || !dxy || !grasp16 || H <= 0 || W <= 0 || dw <= 0) return Y2H_EINVAL;
    if ((uintptr_t)dxy % 16 || (uintptr_t)grasp16 % 8) return Y2H_EINVAL;
    const long total = (long)H * W, groups = (total + 3) / 4;
    hipLaunchKernelGGL(plane_register_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, S(s), grasp_depth, dxy,
                       total, dw, grasp16);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
