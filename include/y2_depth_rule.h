/*
 * The scalar rules of the depth stage that the C host code and the HIP kernels both compile, so that there is one
 * statement of each: the Otsu threshold of KinectUtil_with_cam.cpp:1564-1630, the box -> ROI arithmetic of :1501-1504,
 * the colour -> depth pixel rule of :413-415 and the hand-crop filter test of :1879.  Everything here is IEEE basic
 * arithmetic on named intermediates (build with -ffp-contract=off), so host and device give the same bits.
 */
#ifndef Y2_DEPTH_RULE_H
#define Y2_DEPTH_RULE_H

#ifdef __HIPCC__
#define Y2_HD __host__ __device__ static inline
#else
#define Y2_HD static inline
#endif

/* (int)v of a double with the out-of-range cases pinned down (C leaves them undefined; x86 gives INT_MIN, the GPU
 * saturates): NaN and anything below INT_MIN give INT_MIN, anything above INT_MAX gives INT_MAX.  Truncates toward 0. */
Y2_HD int y2_d2i(double v)
{
    if (!(v >= -2147483648.0)) return (-2147483647 - 1);
    if (v >= 2147483648.0) return 2147483647;
    return (int)v;
}

/* :1501-1504  lo = max(0, (int)((c - s/2.) * L)), hi = min(L, (int)((c + s/2.) * L)), all in double */
Y2_HD void y2_roi_axis(float c, float s, int L, int *lo, int *hi)
{
    const int a = y2_d2i(((double)c - (double)s / 2.) * L);
    const int b = y2_d2i(((double)c + (double)s / 2.) * L);
    *lo = a > 0 ? a : 0;
    *hi = b < L ? b : L;
}

/* :413-415  (int)(X + 0.5f), truncating toward zero (so X = -0.7 lands on 0); a coordinate that is not finite or whose
 * rounded value is outside int range is unmapped (the reference relies on x86's INT_MIN there).  1 when mapped. */
Y2_HD int y2_depth_coord(float X, int lim, int *out)
{
    const float t = X + 0.5f;
    int v;
    if (!(t > -2147483648.f && t < 2147483648.f)) return 0;
    v = (int)t;
    if (v < 0 || v >= lim) return 0;
    *out = v;
    return 1;
}

/* :1879  the pixel is whitened when depth8 <= 500/32 (= 15) or (float)depth8 >= far_m * 1000 / 32 (fp32, that order) */
Y2_HD float y2_far_limit(float far_m) { const float a = far_m * 1000; return a / 32; }
Y2_HD int y2_depth_whitens(unsigned char d8, float far_limit) { return d8 <= 15 || (float)d8 >= far_limit; }

/* :1588  no threshold when more than 85 % of the ROI has no depth */
Y2_HD int y2_otsu_mostly_empty(int hist0, int n) { return (double)hist0 > (double)n * 0.85; }

/* :1596  pixelPro[j] with bin 0 removed from both the counts and the total */
Y2_HD float y2_otsu_prob(int count, int j, int n_nonzero) { return j == 0 ? 0.f : (float)count / n_nonzero; }

/* :1604-1622  the between-class variance of threshold i: both running sums over j = 1..255 in that order in fp32, the
 * squares and the final sum in double (pow(float, 2) promotes), rounded to float on assignment.  Empty classes give
 * 0/0 = NaN, which the caller's strict > then skips. */
Y2_HD float y2_otsu_delta(const float *pro, int i)
{
    float w0 = 0, w1 = 0, u0tmp = 0, u1tmp = 0, u0, u1, u;
    double a, b, s;
    int j;
    for (j = 1; j < 256; ++j) {
        const float jp = j * pro[j];
        if (j <= i) { w0 = w0 + pro[j]; u0tmp = u0tmp + jp; }
        else { w1 = w1 + pro[j]; u1tmp = u1tmp + jp; }
    }
    u0 = u0tmp / w0;
    u1 = u1tmp / w1;
    u = u0tmp + u1tmp;
    a = (double)(u0 - u);
    b = (double)(u1 - u);
    a = a * a;
    b = b * b;
    a = (double)w0 * a;
    b = (double)w1 * b;
    s = a + b;
    return (float)s;
}

/* :1602-1628  strict > in ascending i from deltaMax = 0; delta[i] for i = 1..255 (delta[0] is not read) */
Y2_HD int y2_otsu_pick(const float *delta)
{
    float best = 0;
    int i, thr = 0;
    for (i = 1; i < 256; ++i) if (delta[i] > best) { best = delta[i]; thr = i; }
    return thr;
}

#endif
