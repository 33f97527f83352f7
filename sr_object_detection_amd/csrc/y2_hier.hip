// The hierarchical classifier head ([softmax] tree=FILE, the WordTree head of YOLO9000's classifier):
//   y2h_softmax_tree_rows   softmax_tree (src_yolo2/softmax_layer.c:35-47): one softmax per sibling group of every row
//   y2h_hierarchy_rows      hierarchy_predictions (src_yolo2/tree.c:37-51): conditional -> absolute probabilities
#include "y2_common.hpp"
#include <float.h>

#define ST_NT 512        // threads per row: 9418 double exps per row of a WordTree head

// 64 KB of dynamic LDS per workgroup, the budget of the region head's row kernels (y2_layers.hip region_tree_lds_ok)
static bool hier_lds_ok(size_t floats) { return floats * sizeof(float) <= 64 * 1024; }

// ---------------------------------------------------------------------------
// tree softmax.  Per group exactly softmax_seq (y2_common.hpp; blas.c:205-221): the maximum of the group,
// e = (float)exp((double)(v/temp - largest/temp)), an fp32 running sum in index order, a divide.  Only the order of the sum
// is fixed by the reference, so only the sum is walked by one thread per group; the maximum is also found per group (it is
// a handful of LDS compares), the exponentials -- what the layer costs -- and the divides go element by element over
// all lanes, each element finding its group through group_of[].
// One workgroup per row; LDS holds the row and one float per group (its maximum, then its sum).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ST_NT) void softmax_tree_lds_kernel(const float *x, float *y, int n, float temp, int groups,
                                                                 const int *__restrict__ gsize, const int *__restrict__ goff,
                                                                 const int *__restrict__ group_of)
{
    extern __shared__ float st_lds[];
    float *row = st_lds, *gval = st_lds + n;                    // [n] | [groups]
    const float *in = x + (long)blockIdx.x * n;
    float *out = y + (long)blockIdx.x * n;
    const int t = threadIdx.x;
    for (int i = t; i < n; i += ST_NT) row[i] = in[i];
    __syncthreads();
    for (int g = t; g < groups; g += ST_NT) {                   // 1: the group's maximum
        const int off = goff[g], sz = gsize[g];
        float largest = -FLT_MAX;
        if (off >= 0 && sz > 0 && off <= n - sz)
            for (int i = 0; i < sz; ++i) if (row[off + i] > largest) largest = row[off + i];
        gval[g] = largest;
    }
    __syncthreads();
    for (int i = t; i < n; i += ST_NT) {                        // 2: the exponentials
        const int g = group_of[i];
        if ((unsigned)g < (unsigned)groups) row[i] = (float)exp((double)(row[i] / temp - gval[g] / temp));
    }
    __syncthreads();
    for (int g = t; g < groups; g += ST_NT) {                   // 3: the group's sum, in index order
        const int off = goff[g], sz = gsize[g];
        float sum = 0.f;
        if (off >= 0 && sz > 0 && off <= n - sz)
            for (int i = 0; i < sz; ++i) sum += row[off + i];
        gval[g] = sum;
    }
    __syncthreads();
    for (int i = t; i < n; i += ST_NT) {                        // 4: divide and store
        const int g = group_of[i];
        out[i] = (unsigned)g < (unsigned)groups ? row[i] / gval[g] : row[i];
    }
}

// Rows past the LDS budget: one thread walks one (row, group) in global memory with softmax_seq, as region_tree_kernel does.
__global__ __launch_bounds__(256) void softmax_tree_global_kernel(const float *x, float *y, long rows, int n, float temp, int groups,
                                                                  const int *__restrict__ gsize, const int *__restrict__ goff)
{
    const long total = rows * groups;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int g = (int)(idx % groups);
        const long r = idx / groups;
        const int off = goff[g], sz = gsize[g];
        if (off < 0 || sz <= 0 || off > n - sz) continue;
        softmax_seq(x + r * n + off, sz, temp, y + r * n + off);
    }
}

extern "C" int y2h_softmax_tree_rows(const float *x, float *y, long rows, int n, float temp, int groups, const int *group_size,
                                     const int *group_offset, const int *group_of, y2h_stream s)
{
    if (!x || !y || rows <= 0 || n <= 0 || groups <= 0 || !group_size || !group_offset || !group_of) return Y2H_EINVAL;
    if (rows >= 0x7fffffffL) return Y2H_EINVAL;
    if (hier_lds_ok((size_t)n + groups))
        hipLaunchKernelGGL(softmax_tree_lds_kernel, dim3((unsigned)rows), dim3(ST_NT), ((size_t)n + groups) * sizeof(float), S(s),
                           x, y, n, temp, groups, group_size, group_offset, group_of);
    else
        hipLaunchKernelGGL(softmax_tree_global_kernel, dim3(y2h_grid(rows * groups, 256)), dim3(256), 0, S(s),
                           x, y, rows, n, temp, groups, group_size, group_offset);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// hierarchy_predictions, in place, one workgroup per row.  p[j] *= p[parent[j]] for j ascending: when every parent precedes
// its child each node meets its parent's FINAL value, so the nodes of one depth level are independent and the row is
// walked level by level (as decode_tree_kernel, y2_detect.hip); the products are the same fp32 multiplications.  Without
// level tables (some child stands before its parent and is multiplied by the parent's not yet multiplied value) one lane
// walks the row in the reference's order.  Then p[j] = 0 where !leaf[j], when there is a leaf table.
// LDS = true: the row is staged in LDS; otherwise it is walked where it lies.
// ---------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(256) void hierarchy_rows_kernel(float *rows, long ld, int n, const int *__restrict__ parent,
                                                             const int *__restrict__ order, const int *__restrict__ level_off,
                                                             int levels, const int *__restrict__ leaf, const int *__restrict__ row_mask)
{
    extern __shared__ float h_lds[];
    if (row_mask && !row_mask[blockIdx.x]) return;              // uniform over the workgroup
    float *g = rows + (long)blockIdx.x * ld;
    float *p = LDS ? h_lds : g;
    const int t = threadIdx.x;
    if (LDS) {
        for (int j = t; j < n; j += 256) p[j] = g[j];
        __syncthreads();
    }
    if (levels > 0) {
        for (int lv = 1; lv < levels; ++lv) {                   // level 0 = roots (parent < 0): unchanged
            const int b = level_off[lv], e = level_off[lv + 1];
            for (int q = b + t; q < e; q += 256) {
                const int j = order[q];
                p[j] *= p[parent[j]];
            }
            __syncthreads();
        }
    } else {
        if (t == 0)
            for (int j = 0; j < n; ++j) {
                const int par = parent[j];
                if (par >= 0 && par < n) p[j] *= p[par];
            }
        __syncthreads();
    }
    if (LDS) for (int j = t; j < n; j += 256) g[j] = (leaf && !leaf[j]) ? 0.f : p[j];
    else if (leaf) for (int j = t; j < n; j += 256) if (!leaf[j]) g[j] = 0.f;
}

extern "C" int y2h_hierarchy_rows(float *rows, long ld, int nrows, int n, const int *parent, const int *order,
                                  const int *level_off, int levels, const int *leaf, const int *row_mask, y2h_stream s)
{
    if (!rows || nrows <= 0 || n <= 0 || ld < n || !parent || levels < 0) return Y2H_EINVAL;
    if (levels > 0 && (!order || !level_off)) return Y2H_EINVAL;
    if (hier_lds_ok((size_t)n))
        hipLaunchKernelGGL(hierarchy_rows_kernel<true>, dim3((unsigned)nrows), dim3(256), (size_t)n * sizeof(float), S(s),
                           rows, ld, n, parent, order, level_off, levels, leaf, row_mask);
    else
        hipLaunchKernelGGL(hierarchy_rows_kernel<false>, dim3((unsigned)nrows), dim3(256), 0, S(s),
                           rows, ld, n, parent, order, level_off, levels, leaf, row_mask);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
