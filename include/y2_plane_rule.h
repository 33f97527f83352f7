/*
 * The rule of the table-plane removal (the Grasp branch of the Kinect loop) that the C host code and the HIP kernels
 * both compile, so that there is one statement of it.  It restates what KinectUtil_with_cam.cpp:1931-1974 (desk_seg)
 * and plane_seg.cpp:157-213 do -- clip the depth frame, turn it into a cloud, RANSAC a plane with PCL, refit, zero the
 * inliers -- as a DETERMINISTIC procedure: PCL's sampler is seeded from the clock and the SDK's depth-to-camera mapping
 * is closed, so there is no bit pattern to be compatible with and this header is the definition.  Everything here is
 * IEEE basic arithmetic (+ - * / sqrt) on named intermediates (build with -ffp-contract=off), so host and device give
 * the same bits.
 *
 * The reduction tree of the refit sums.  N = dh*dw depth pixels, flat index i = y*dw + x; a pixel that is not an inlier
 * of the best hypothesis, and every index >= N, contributes +0.0 to each of the ten sums.
 *   leaf   L[j]    = ((v[4j] + v[4j+1]) + v[4j+2]) + v[4j+3]                      j = 0 .. 256*C-1, C = ceil(N / 1024)
 *   chunk  P[c]    = the binary tree over A[t] = L[256c + t], t = 0..255:
 *                    for s = 128, 64, ..., 1:  A[t] = A[t] + A[t+s] for every t < s;   P[c] = A[0]
 *   group  G[m]    = the same binary tree over B[t] = P[256m + t], t = 0..255 (+0.0 for 256m + t >= C), m = 0 .. ceil(C / 256)-1
 *   total  S       = (...((G[0] + G[1]) + G[2]) ... )      (a 512 x 424 frame has C = 212 chunks and one group: S = G[0])
 * It depends on nothing but N: not on the launch shape and not on the order in which anything arrives.
 */
#ifndef Y2_PLANE_RULE_H
#define Y2_PLANE_RULE_H

#include <math.h>

#ifdef __HIPCC__
#define Y2P_HD __host__ __device__ static inline
#else
#define Y2P_HD static inline
#endif

#define Y2_PLANE_MAX_ITERS 256           /* hypotheses of one frame */
#define Y2_PLANE_MAX_DRAWS 64            /* sampler draws of one hypothesis, rejected ones included */
#define Y2_PLANE_CHUNK 1024              /* depth pixels of one chunk of the tree: 256 leaves of 4 */
#define Y2_PLANE_SWEEPS 6                /* cyclic Jacobi sweeps of the refit */

typedef struct { float nx, ny, nz, d; int ok; } y2_plane_hyp;

/* :1944-1950  g = ((float)d > far_m * 1000.f) ? 0 : d, with far_mm = far_m * 1000.f formed once in fp32 */
Y2P_HD float y2_plane_far_mm(float far_m) { return far_m * 1000.f; }
Y2P_HD unsigned short y2_plane_clip(unsigned short d, float far_mm) { return (float)d > far_mm ? (unsigned short)0 : d; }

/* the camera-space point of a valid depth pixel: our MapDepthPointToCameraSpace at an integer pixel */
Y2P_HD void y2_plane_point(unsigned short g, float tx, float ty, float *p)
{
    const float z = (float)g / 1000.f;
    p[0] = tx * z;
    p[1] = ty * z;
    p[2] = z;
}

/* the sampler's generator; the index drawn is (state >> 8) % (dh*dw) */
Y2P_HD unsigned y2_plane_lcg(unsigned state) { return state * 1664525u + 1013904223u; }

/* the plane through three points, all in fp32; ok = 0: degenerate (void) */
Y2P_HD void y2_plane_of_points(const float *p0, const float *p1, const float *p2, y2_plane_hyp *h)
{
    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const float vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const float yz = uy * vz, zy = uz * vy, zx = uz * vx, xz = ux * vz, xy = ux * vy, yx = uy * vx;
    const float cx = yz - zy, cy = zx - xz, cz = xy - yx;
    const float xx = cx * cx, yy = cy * cy, zz = cz * cz;
    const float len = sqrtf((xx + yy) + zz);
    h->nx = 0.f; h->ny = 0.f; h->nz = 0.f; h->d = 0.f; h->ok = 0;
    if (!(len > 0.f) || !(len <= 3.402823466e+38f)) return;
    {
        const float nx = cx / len, ny = cy / len, nz = cz / len;
        const float a = nx * p0[0], b = ny * p0[1], c = nz * p0[2];
        h->nx = nx; h->ny = ny; h->nz = nz;
        h->d = -((a + b) + c);
        h->ok = 1;
    }
}

/* the hypothesis of a triple of depth-pixel indices: void when an index is outside the frame, repeats another of the
 * triple or names a pixel that is not valid, or when the three points span no plane */
Y2P_HD void y2_plane_of_triple(const unsigned short *depth, const float *tab, long n, float far_mm, const int *t, y2_plane_hyp *h)
{
    float p[3][3];
    int k;
    h->nx = 0.f; h->ny = 0.f; h->nz = 0.f; h->d = 0.f; h->ok = 0;
    if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) return;
    for (k = 0; k < 3; ++k) {
        unsigned short g;
        if (t[k] < 0 || t[k] >= n) return;
        g = y2_plane_clip(depth[t[k]], far_mm);
        if (!(g > 0)) return;
        y2_plane_point(g, tab[2 * (long)t[k]], tab[2 * (long)t[k] + 1], p[k]);
    }
    y2_plane_of_points(p[0], p[1], p[2], h);
}

/* PCL's countWithinDistance: strict < */
Y2P_HD int y2_plane_inlier(const y2_plane_hyp *h, const float *p, float dist_m)
{
    const float a = h->nx * p[0], b = h->ny * p[1], c = h->nz * p[2];
    const float s = ((a + b) + c) + h->d;
    return fabsf(s) < dist_m;
}

/* what one inlier adds to the ten sums: n, x, y, z, xx, xy, xz, yy, yz, zz with the components converted to double */
Y2P_HD void y2_plane_terms(const float *p, double *v)
{
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    v[0] = 1.0; v[1] = x; v[2] = y; v[3] = z;
    v[4] = x * x; v[5] = x * y; v[6] = x * z; v[7] = y * y; v[8] = y * z; v[9] = z * z;
}

/* one rotation of the cyclic Jacobi method on the symmetric 3x3 A (eigenvectors accumulate in the columns of V); p < q
 * and r is the third index.  A zero off-diagonal element is left alone. */
Y2P_HD void y2_plane_rotate(double A[3][3], double V[3][3], int p, int q, int r)
{
    const double apq = A[p][q];
    double theta, at, t, c, s, app, aqq, arp, arq, tt;
    int k;
    if (apq == 0.0) return;
    theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    at = theta < 0.0 ? -theta : theta;
    tt = theta * theta;
    t = 1.0 / (at + sqrt(tt + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
    app = A[p][p] - t * apq;
    aqq = A[q][q] + t * apq;
    arp = c * A[r][p] - s * A[r][q];
    arq = s * A[r][p] + c * A[r][q];
    A[p][p] = app; A[q][q] = aqq; A[p][q] = 0.0; A[q][p] = 0.0;
    A[r][p] = arp; A[p][r] = arp; A[r][q] = arq; A[q][r] = arq;
    for (k = 0; k < 3; ++k) {
        const double vp = c * V[k][p] - s * V[k][q];
        const double vq = s * V[k][p] + c * V[k][q];
        V[k][p] = vp; V[k][q] = vq;
    }
}

/* setOptimizeCoefficients(true): the least-squares plane of the inliers from their ten sums.  Covariance
 * sum_ab / n - mean_a * mean_b; the normal is the eigenvector of the smallest eigenvalue (a tie goes to the lowest index)
 * after Y2_PLANE_SWEEPS sweeps over (0,1), (0,2), (1,2); normalised; d = -n . mean; oriented towards the camera
 * (d < 0 negates all four).  0: fewer than three points or no normal. */
Y2P_HD int y2_plane_fit_sums(const double *S, double *out)
{
    double A[3][3], V[3][3], mx, my, mz, nx, ny, nz, len, d, xx, yy, zz, a, b, c;
    const double n = S[0];
    int sweep, best;
    out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0;
    if (!(n >= 3.0)) return 0;
    mx = S[1] / n; my = S[2] / n; mz = S[3] / n;
    A[0][0] = S[4] / n - mx * mx; A[0][1] = S[5] / n - mx * my; A[0][2] = S[6] / n - mx * mz;
    A[1][1] = S[7] / n - my * my; A[1][2] = S[8] / n - my * mz; A[2][2] = S[9] / n - mz * mz;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    V[0][0] = 1.0; V[0][1] = 0.0; V[0][2] = 0.0;
    V[1][0] = 0.0; V[1][1] = 1.0; V[1][2] = 0.0;
    V[2][0] = 0.0; V[2][1] = 0.0; V[2][2] = 1.0;
    for (sweep = 0; sweep < Y2_PLANE_SWEEPS; ++sweep) {
        y2_plane_rotate(A, V, 0, 1, 2);
        y2_plane_rotate(A, V, 0, 2, 1);
        y2_plane_rotate(A, V, 1, 2, 0);
    }
    best = 0;
    if (A[1][1] < A[best][best]) best = 1;
    if (A[2][2] < A[best][best]) best = 2;
    nx = V[0][best]; ny = V[1][best]; nz = V[2][best];
    xx = nx * nx; yy = ny * ny; zz = nz * nz;
    len = sqrt((xx + yy) + zz);
    if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) return 0;
    nx = nx / len; ny = ny / len; nz = nz / len;
    a = nx * mx; b = ny * my; c = nz * mz;
    d = -((a + b) + c);
    if (d < 0.0) { nx = -nx; ny = -ny; nz = -nz; d = -d; }
    out[0] = nx; out[1] = ny; out[2] = nz; out[3] = d;
    return 1;
}

/* PCL re-selects the inliers after optimising: the final test of a valid pixel, in double */
Y2P_HD int y2_plane_removes(const double *pl, const float *p, float dist_m)
{
    const double a = pl[0] * (double)p[0], b = pl[1] * (double)p[1], c = pl[2] * (double)p[2];
    const double s = ((a + b) + c) + pl[3];
    return fabs(s) < (double)dist_m;
}

#endif
