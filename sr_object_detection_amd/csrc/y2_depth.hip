// y2_depth.hip -- the depth stage of the Kinect RGB-D loop on the device: what the application does on the host, in
// OpenCV loops over colour-sized mats, between two detector calls.  Reference behaviour restated:
//   * registration of the depth / body-index frames to the colour frame      KinectUtil_with_cam.cpp:394-442 (drawDepth)
//   * per detection: Otsu threshold of the 8-bit depth in the box            :1564-1630 (otsuThreshold)
//                    thresholded mean depth                                  :1321-1346 (GetImgAvg), :1526
//                    five depth-space points                                 :1347-1453 (caculateXY)
//                    camera-space point, width, height                       :1540-1559
//                    owner by majority of the body-index pixels              :1632-1706 (objectBelong2Person)
// Every sum is an integer sum (depth in 64 bits), so block shape and atomic arrival order cannot change a value; the few
// float steps are single IEEE operations on those integers (this file is built with -ffp-contract=off).
#include "y2_common.hpp"
#include "y2_depth_rule.h"

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// registration: one thread per four consecutive colour pixels of the flat H*W index, so every store is one vector
// store whatever W is (the planes start 256-byte aligned); the depth / body reads are gathers into a frame that fits L2
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_align_kernel(const unsigned short *__restrict__ depth,
                                                          const unsigned char *__restrict__ body,
                                                          const float *__restrict__ map, int dh, int dw, int H, int W,
                                                          unsigned short *__restrict__ depth16, unsigned char *__restrict__ depth8,
                                                          unsigned char *__restrict__ person, short *__restrict__ dxy)
{
    const long total = (long)H * W;
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    const int nx = (int)min(4L, total - i0);
    float xy[8];
    if (map) {
        if (nx == 4) {
            const float4 a = *(const float4 *)(map + 2 * i0), b = *(const float4 *)(map + 2 * i0 + 4);
            xy[0] = a.x; xy[1] = a.y; xy[2] = a.z; xy[3] = a.w; xy[4] = b.x; xy[5] = b.y; xy[6] = b.z; xy[7] = b.w;
        } else {
            for (int k = 0; k < 4; ++k) { xy[2 * k] = k < nx ? map[2 * (i0 + k)] : 0.f; xy[2 * k + 1] = k < nx ? map[2 * (i0 + k) + 1] : 0.f; }
        }
    }
    unsigned short v16[4];
    unsigned char v8[4], vp[4];
    short vxy[8];
    for (int k = 0; k < 4; ++k) {
        int dx = 0, dy = 0, ok;
        if (map) ok = y2_depth_coord(xy[2 * k], dw, &dx) & y2_depth_coord(xy[2 * k + 1], dh, &dy);
        else { const long i = min(i0 + k, total - 1); dy = (int)(i / W); dx = (int)(i - (long)dy * W); ok = 1; }
        v16[k] = 0; v8[k] = 0; vp[k] = 255; vxy[2 * k] = -1; vxy[2 * k + 1] = -1;
        if (ok && k < nx) {
            const size_t di = (size_t)dy * dw + dx;
            const unsigned short d = depth[di];
            v16[k] = d;
            v8[k] = (unsigned char)(d >> 5);
            if (body) vp[k] = body[di];
            vxy[2 * k] = (short)dx; vxy[2 * k + 1] = (short)dy;
        }
    }
    if (nx == 4) {
        *(ushort4 *)(depth16 + i0) = make_ushort4(v16[0], v16[1], v16[2], v16[3]);
        *(uchar4 *)(depth8 + i0) = make_uchar4(v8[0], v8[1], v8[2], v8[3]);
        *(uchar4 *)(person + i0) = make_uchar4(vp[0], vp[1], vp[2], vp[3]);
        if (dxy) {
            *(short4 *)(dxy + 2 * i0) = make_short4(vxy[0], vxy[1], vxy[2], vxy[3]);
            *(short4 *)(dxy + 2 * i0 + 4) = make_short4(vxy[4], vxy[5], vxy[6], vxy[7]);
        }
    } else {
        for (int k = 0; k < nx; ++k) {
            depth16[i0 + k] = v16[k]; depth8[i0 + k] = v8[k]; person[i0 + k] = vp[k];
            if (dxy) { dxy[2 * (i0 + k)] = vxy[2 * k]; dxy[2 * (i0 + k) + 1] = vxy[2 * k + 1]; }
        }
    }
}

extern "C" int y2h_depth_align(const unsigned short *depth, const unsigned char *body, const float *map, int dh, int dw, int H,
                               int W, unsigned short *depth16, unsigned char *depth8, unsigned char *person, short *dxy,
                               y2h_stream s)
{
    if (!depth || !depth16 || !depth8 || !person || dh <= 0 || dw <= 0 || H <= 0 || W <= 0 || dh > 32767 || dw > 32767)
        return Y2H_EINVAL;
    if (map ? !dxy : (H != dh || W != dw)) return Y2H_EINVAL;
    if ((uintptr_t)depth16 % 8 || (uintptr_t)depth8 % 4 || (uintptr_t)person % 4 || (uintptr_t)dxy % 16 || (uintptr_t)map % 32)
        return Y2H_EINVAL;
    const long groups = ((long)H * W + 3) / 4;
    hipLaunchKernelGGL(depth_align_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, S(s), depth, body, map, dh,
                       dw, H, W, depth16, depth8, person, map ? dxy : (short *)nullptr);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

// ---------------------------------------------------------------------------
// per-box statistics
// ---------------------------------------------------------------------------
struct DepthAcc {                        // one box's accumulators, zeroed before pass 1; integer adds only
    int hist[256];                       // depth8 histogram of the ROI
    int person[8];                       // pixels of body labels 1..6 (slots 0 and 7 unused)
    u64 sum_all;                         // depth16 over the ROI
    u64 sum, idx;                        // depth16 and count of pixels with 0 < d < thr
    u64 pt[5][3];                        // centre, top, bottom, left, right: sum dx, sum dy, count
    int otsu, pad_;
    u64 sum_all_g;                       // Grasp event: grasp16 over the ROI (GetImgAvg's own sumAll)
};

struct DepthJob {
    y2h_depth_planes p;
    const float *boxes; int stride_box; long stride_item;
    const int *counts; const y2h_box_map *maps;
    int per_item;
    DepthAcc *acc;
};

struct Roi { int left, top, right, bot; };

// slot -> its box in its frame -> ROI.  false: the slot holds no box.  valid tells whether the ROI is non-empty.
__device__ __forceinline__ bool depth_slot_roi(const DepthJob &q, int slot, Roi &r, bool &valid)
{
    const int b = slot / q.per_item, j = slot - b * q.per_item;
    if (q.counts && j >= q.counts[b]) return false;
    const float *bp = q.boxes + ((size_t)b * q.stride_item + j) * q.stride_box;
    float x = bp[0], y = bp[1], w = bp[2], h = bp[3];
    if (q.maps) {                        // y2_region_box_to_frame, the same fp32 expressions in the same order
        const y2h_box_map m = q.maps[b];
        if (m.letterbox) {
            x = (x * m.net_w - (m.net_w - m.nw) / 2) / m.nw;
            y = (y * m.net_h - (m.net_h - m.nh) / 2) / m.nh;
            w = w * m.net_w / m.nw;
            h = h * m.net_h / m.nh;
        }
        if (!m.whole) {
            x = (x * m.rw + m.rx) / m.fw;
            y = (y * m.rh + m.ry) / m.fh;
            w = w * m.rw / m.fw;
            h = h * m.rh / m.fh;
        }
    }
    y2_roi_axis(x, w, q.p.W, &r.left, &r.right);
    y2_roi_axis(y, h, q.p.H, &r.top, &r.bot);
    valid = r.right > r.left && r.bot > r.top;
    return true;
}

// Launch shape of both passes: grid (chunks, rows).  The `chunks` workgroups of a row share each box's ROI by flat pixel
// index (up to 64 of them, whatever the number of slots); row y walks the slots y, y + rows, ... and skips those past
// their item's count after one read of it, so a launch for thousands of mostly empty slots costs a few thousand
// workgroups, not one per slot and chunk.  Every condition on a slot is uniform per workgroup.
//
// pass 1: histogram of depth8, body-label counts, sum of depth16.  One LDS histogram per wave, merged and added to the
// box's accumulators with integer atomics.
__global__ __launch_bounds__(256) void depth_pass1_kernel(DepthJob q, int slots)
{
    __shared__ int hist[4][256];
    __shared__ int lperson[8];
    __shared__ u64 lsum, lsumg;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int slot = blockIdx.y; slot < slots; slot += gridDim.y) {
    Roi r; bool valid;
    if (!depth_slot_roi(q, slot, r, valid) || !valid) continue;
    if ((long)blockIdx.x * 256 >= (long)(r.right - r.left) * (r.bot - r.top)) continue;     // a small ROI needs few chunks
    __syncthreads();                                    // the last box's merge has read the LDS
    for (int k = 0; k < 4; ++k) hist[k][tid] = 0;
    if (tid < 8) lperson[tid] = 0;
    if (tid == 0) { lsum = 0; lsumg = 0; }
    __syncthreads();
    const int rw = r.right - r.left;
    const long n = (long)rw * (r.bot - r.top);
    const long nround = (n + 255) / 256 * 256;          // whole waves stay in the loop: the ballots below need every lane
    u64 s = 0, sg = 0;
    int pc[7] = {0, 0, 0, 0, 0, 0, 0};                  // wave-uniform label counts
    for (long i = (long)blockIdx.x * 256 + tid; i < nround; i += (long)gridDim.x * 256) {
        int lab = 0;
        if (i < n) {
            const int rr = (int)(i / rw), cc = (int)(i - (long)rr * rw);
            const size_t at = (size_t)(r.top + rr) * q.p.W + r.left + cc;
            atomicAdd(&hist[wave][q.p.depth8[at]], 1);
            s += q.p.depth16[at];
            if (q.p.grasp16) sg += q.p.grasp16[at];
            lab = q.p.person[at];
        }
        const bool is_person = lab >= 1 && lab <= 6;
        if (__any(is_person))
            for (int l = 1; l <= 6; ++l) pc[l] += __popcll(__ballot(lab == l));
    }
    if (s) atomicAdd(&lsum, s);
    if (sg) atomicAdd(&lsumg, sg);
    if ((tid & 63) == 0) for (int l = 1; l <= 6; ++l) if (pc[l]) atomicAdd(&lperson[l], pc[l]);
    __syncthreads();
    DepthAcc *a = q.acc + slot;
    const int hsum = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
    if (hsum) atomicAdd(&a->hist[tid], hsum);
    if (tid >= 1 && tid <= 6 && lperson[tid]) atomicAdd(&a->person[tid], lperson[tid]);
    if (tid == 0 && lsum) atomicAdd(&a->sum_all, lsum);
    if (tid == 0 && lsumg) atomicAdd(&a->sum_all_g, lsumg);
    }
}

// pass 2: every block of a slot recomputes the Otsu threshold from the finished histogram (one lane per candidate i,
// each with its own 255-step loop, as the association of the running sums differs per i), then the thresholded depth sum
// and the five point sums.  In the Grasp event (:1508-1518) there is no Otsu step: the threshold is 255 * 32 and the
// thresholded sum reads grasp16.
__global__ __launch_bounds__(256) void depth_pass2_kernel(DepthJob q, int slots)
{
    __shared__ float pro[256];
    __shared__ float delta[256];
    __shared__ int s_otsu;
    __shared__ u64 l[17];                // sum, idx, pt[5][3]
    const int tid = threadIdx.x;
    for (int slot = blockIdx.y; slot < slots; slot += gridDim.y) {
    Roi r; bool valid;
    if (!depth_slot_roi(q, slot, r, valid) || !valid) continue;
    if ((long)blockIdx.x * 256 >= (long)(r.right - r.left) * (r.bot - r.top)) continue;     // chunk 0 always stays: it stores otsu
    DepthAcc *a = q.acc + slot;
    __syncthreads();                                    // the last box's merge has read the LDS
    const int rw = r.right - r.left, rh = r.bot - r.top;
    const long n = (long)rw * rh;
    const unsigned short *avg_src = q.p.grasp16 ? q.p.grasp16 : q.p.depth16;
    if (tid < 17) l[tid] = 0;
    if (q.p.grasp16) {
        if (tid == 0) {
            s_otsu = 255;
            if (blockIdx.x == 0) a->otsu = s_otsu;
        }
    } else {
        const int hist0 = a->hist[0];
        pro[tid] = y2_otsu_prob(a->hist[tid], tid, (int)n - hist0);
        __syncthreads();
        delta[tid] = tid ? y2_otsu_delta(pro, tid) : 0.f;
        __syncthreads();
        if (tid == 0) {
            s_otsu = y2_otsu_mostly_empty(hist0, (int)n) ? 0 : y2_otsu_pick(delta);
            if (blockIdx.x == 0) a->otsu = s_otsu;
        }
    }
    __syncthreads();
    const int thr = s_otsu * 32;
    u64 sum = 0, idx = 0, cx = 0, cy = 0, cn = 0;
    for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256) {
        const int rr = (int)(i / rw), cc = (int)(i - (long)rr * rw);
        const int Y = r.top + rr, X = r.left + cc;
        const size_t at = (size_t)Y * q.p.W + X;
        const int d = avg_src[at];
        if (d > 0 && d < thr) { sum += d; ++idx; }
        int dx = X, dy = Y;
        if (q.p.dxy) { const short2 v = *(const short2 *)(q.p.dxy + 2 * at); dx = v.x; dy = v.y; }
        if (dx < 0) continue;                                        // unmapped
        // :1373 compares the 8-bit value with the threshold that is already x32 (the reference's quirk)
        if ((int)q.p.depth8[at] < thr) { cx += dx; cy += dy; ++cn; }
        if (rr == 0) { atomicAdd(&l[5], (u64)dx); atomicAdd(&l[6], (u64)dy); atomicAdd(&l[7], (u64)1); }
        if (rr == rh - 1) { atomicAdd(&l[8], (u64)dx); atomicAdd(&l[9], (u64)dy); atomicAdd(&l[10], (u64)1); }
        if (cc == 0) { atomicAdd(&l[11], (u64)dx); atomicAdd(&l[12], (u64)dy); atomicAdd(&l[13], (u64)1); }
        if (cc == rw - 1) { atomicAdd(&l[14], (u64)dx); atomicAdd(&l[15], (u64)dy); atomicAdd(&l[16], (u64)1); }
    }
    if (idx) { atomicAdd(&l[0], sum); atomicAdd(&l[1], idx); }
    if (cn) { atomicAdd(&l[2], cx); atomicAdd(&l[3], cy); atomicAdd(&l[4], cn); }
    __syncthreads();
    if (tid < 17 && l[tid]) {
        u64 *dst = tid == 0 ? &a->sum : tid == 1 ? &a->idx : &a->pt[0][0] + (tid - 2);
        atomicAdd(dst, l[tid]);
    }
    }
}

struct CamPoint { float x, y, z; };

// our definition of MapDepthPointToCameraSpace (the SDK's mapper is closed): the GetDepthFrameToCameraSpaceTable entry
// under the rounded depth-space point, scaled by the depth in metres; -inf outside the table, as the SDK answers
__device__ __forceinline__ CamPoint depth_to_camera(const y2h_depth_planes &p, float px, float py, float z)
{
    const float ninf = -__builtin_inff();
    CamPoint c = {ninf, ninf, ninf};
    int ix, iy;
    if (!y2_depth_coord(px, p.dw, &ix) || !y2_depth_coord(py, p.dh, &iy)) return c;
    const float *t = p.cam_table + ((size_t)iy * p.dw + ix) * 2;
    c.x = t[0] * z; c.y = t[1] * z; c.z = z;
    return c;
}

__device__ __forceinline__ bool is_inf(float v) { return v == __builtin_inff() || v == -__builtin_inff(); }

__global__ __launch_bounds__(64) void depth_finalise_kernel(DepthJob q, int slots, y2h_det3d *__restrict__ out)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= slots) return;
    Roi r; bool valid;
    if (!depth_slot_roi(q, slot, r, valid)) return;
    // results are written densely, item after item (item b's first record follows item b-1's last), so that the host
    // fetches the records that exist and not the launch's whole capacity
    int at = slot;
    if (q.counts) {
        const int b = slot / q.per_item;
        at = slot - b * q.per_item;
        for (int i = 0; i < b; ++i) at += min(q.counts[i], q.per_item);
    }
    out += at - slot;
    y2h_det3d o;
    memset(&o, 0, sizeof o);
    if (!valid) { o.cam_z = -1.f; out[slot] = o; return; }
    const DepthAcc *a = q.acc + slot;
    const long n = (long)(r.right - r.left) * (r.bot - r.top);
    o.valid = 1; o.left = r.left; o.top = r.top; o.right = r.right; o.bot = r.bot;
    o.otsu = a->otsu;
    o.mean_all_mm = (int)(a->sum_all / (u64)n);                                 // KinectUtil.cpp:489-501
    const u64 all = q.p.grasp16 ? a->sum_all_g : a->sum_all;
    const float res = (float)(a->idx ? a->sum / a->idx : all / (u64)n);          // :1340-1345, integer division
    o.avg_mm = q.p.grasp16 ? res : res - 16;                                    // :1526; :1516 subtracts nothing
    for (int k = 0; k < 5; ++k) {
        const u64 c = a->pt[k][2];
        o.pts[k][0] = c ? (float)a->pt[k][0] / (float)c : 0.f;                  // :1403-1452
        o.pts[k][1] = c ? (float)a->pt[k][1] / (float)c : 0.f;
    }
    int best = 0, label = 0;                                                    // :1684-1703; a tie goes to the lower label
    for (int k = 1; k <= 6; ++k) if (a->person[k] > best) { best = a->person[k]; label = k; }
    const float share = (float)best / (float)n;
    o.belongs = (double)share > 0.5;
    o.body_id = o.belongs ? label : 255;
    if (!q.p.cam_table) { o.cam_z = -1.f; out[slot] = o; return; }
    const float z = o.avg_mm / 1000.f;
    const CamPoint pc = depth_to_camera(q.p, o.pts[0][0], o.pts[0][1], z), pt = depth_to_camera(q.p, o.pts[1][0], o.pts[1][1], z),
                   pb = depth_to_camera(q.p, o.pts[2][0], o.pts[2][1], z), pl = depth_to_camera(q.p, o.pts[3][0], o.pts[3][1], z),
                   pr = depth_to_camera(q.p, o.pts[4][0], o.pts[4][1], z);
    o.cam_x = pc.x; o.cam_y = pc.y; o.cam_z = pc.z;                             // :1546-1559
    if (is_inf(pc.x) || is_inf(pc.y) || is_inf(pc.z)) { o.cam_x = 0; o.cam_y = 0; o.cam_z = -1; }
    {
        const float ax = pl.x - pr.x, ay = pl.y - pr.y, axx = ax * ax, ayy = ay * ay, sw = axx + ayy;
        const float bx = pt.x - pb.x, by = pt.y - pb.y, bxx = bx * bx, byy = by * by, sh = bxx + byy;
        o.cam_w = (float)((double)sqrtf(sw) - 0.02);
        o.cam_h = sqrtf(sh);
    }
    out[slot] = o;
}

extern "C" unsigned long y2h_depth_acc_bytes(void) { return sizeof(DepthAcc); }

extern "C" int y2h_depth_boxes(const y2h_depth_planes *p, const float *boxes, int stride_box, long stride_item,
                               const int *counts, const y2h_box_map *maps, int items, int per_item, void *acc, y2h_det3d *out,
                               int stages, y2h_stream s)
{
    if (!p || !p->depth16 || !p->depth8 || !p->person || p->H <= 0 || p->W <= 0 || !boxes || stride_box < 4 || items <= 0 ||
        per_item <= 0 || stride_item < per_item || !acc || !out)
        return Y2H_EINVAL;
    if (p->cam_table && (p->dh <= 0 || p->dw <= 0)) return Y2H_EINVAL;
    const long slots = (long)items * per_item;
    if (slots > (1L << 24)) return Y2H_EINVAL;
    DepthJob q;
    q.p = *p; q.boxes = boxes; q.stride_box = stride_box; q.stride_item = stride_item; q.counts = counts; q.maps = maps;
    q.per_item = per_item; q.acc = (DepthAcc *)acc;
    // workgroups per box: enough for a full-frame box to keep the chip busy, bounded by the frame alone (4096 pixels, 16 per
    // thread, is the least a workgroup is worth starting for); a small ROI's spare chunks return at once
    long chunks = ((long)p->H * p->W + 4095) / 4096;
    if (chunks > 64) chunks = 64;
    const unsigned rows = (unsigned)(slots < 128 ? slots : 128);
    if (stages & Y2H_DEPTH_CLEAR) Y2H_CHECK(hipMemsetAsync(acc, 0, (size_t)slots * sizeof(DepthAcc), S(s)));
    if (stages & Y2H_DEPTH_PASS1) {
        hipLaunchKernelGGL(depth_pass1_kernel, dim3((unsigned)chunks, rows), dim3(256), 0, S(s), q, (int)slots);
        Y2H_LAUNCH_CHECK();
    }
    if (stages & Y2H_DEPTH_PASS2) {
        hipLaunchKernelGGL(depth_pass2_kernel, dim3((unsigned)chunks, rows), dim3(256), 0, S(s), q, (int)slots);
        Y2H_LAUNCH_CHECK();
    }
    if (stages & Y2H_DEPTH_FINALISE) {
        hipLaunchKernelGGL(depth_finalise_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, S(s), q, (int)slots, out);
        Y2H_LAUNCH_CHECK();
    }
    return Y2H_OK;
}
