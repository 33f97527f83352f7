"""The depth stage of the Kinect loop restated in numpy: the yardstick of tests/test_depth_host.py and
tests/test_gpu_depth.py.  The reference code (src_yolo2/KinectUtil_with_cam.cpp, KinectUtil.cpp) needs the Kinect SDK,
OpenCV and Windows, so nothing here is pinned on a reference run; every rule cites the lines it restates.  Integer
sums are int64 (Python ints), floats are np.float32 / np.float64 in the order of the C expressions."""
from __future__ import annotations

import numpy as np

f32 = np.float32
f64 = np.float64
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def d2i(v) -> int:
    """(int)v of a double with the undefined cases pinned as include/y2_depth_rule.h pins them"""
    v = float(v)
    if not v >= -2147483648.0:
        return INT_MIN
    if v >= 2147483648.0:
        return INT_MAX
    return int(v)                                             # truncates toward zero


def roi(box, W, H):
    """KinectUtil_with_cam.cpp:1501-1504 -> (valid, left, top, right, bot); the box values are fp32, the rest double"""
    x, y, w, h = (f64(f32(v)) for v in box)
    left = max(0, d2i((x - w / f64(2.)) * f64(W)))
    right = min(W, d2i((x + w / f64(2.)) * f64(W)))
    top = max(0, d2i((y - h / f64(2.)) * f64(H)))
    bot = min(H, d2i((y + h / f64(2.)) * f64(H)))
    return int(right > left and bot > top), left, top, right, bot


def depth_coord(X, lim):
    """:413-415 (int)(X + 0.5f), truncation toward zero; not finite or outside int range: unmapped -> index or None"""
    with np.errstate(all="ignore"):
        t = f32(X) + f32(0.5)
    if not (t > f32(-2147483648.) and t < f32(2147483648.)):
        return None
    v = int(t)
    return v if 0 <= v < lim else None


def align(depth, body, map_):
    """:407-423 drawDepth -> (depth16, depth8, person, dxy int32 [H][W][2] with -1 = unmapped)"""
    dh, dw = depth.shape
    if map_ is None:
        H, W = dh, dw
        ys, xs = np.mgrid[0:H, 0:W]
        dxy = np.stack([xs, ys], axis=-1).astype(np.int32)
    else:
        H, W = map_.shape[:2]
        dxy = np.full((H, W, 2), -1, np.int32)
        for r in range(H):
            for c in range(W):
                x, y = depth_coord(map_[r, c, 0], dw), depth_coord(map_[r, c, 1], dh)
                if x is not None and y is not None:
                    dxy[r, c] = (x, y)
    ok = dxy[..., 0] >= 0
    yy, xx = np.where(ok, dxy[..., 1], 0), np.where(ok, dxy[..., 0], 0)
    d16 = np.where(ok, depth[yy, xx], 0).astype(np.uint16)
    d8 = (d16 >> 5).astype(np.uint8)                          # :418 static_cast<BYTE>(depth >> 5)
    person = np.where(ok, body[yy, xx] if body is not None else 255, 255).astype(np.uint8)
    return d16, d8, person, dxy


def whiten(frame, rect, depth8, far_m):
    """:1866-1888 colorImgFilterbyDistance on the crop `rect` of `frame` (a copy of the frame is returned): a pixel is
    set to 255 in every channel when depth8 <= 500/32 or (float)depth8 >= distance * 1000 / 32 (fp32, that order)"""
    out = frame.copy()
    if not far_m > 0:
        return out
    H, W = frame.shape[:2]
    x, y, rw, rh = rect if rect is not None and (rect[2] or rect[3]) else (0, 0, W, H)
    lim = f32(f32(far_m) * f32(1000)) / f32(32)
    d = depth8[y:y + rh, x:x + rw]
    mask = (d <= 15) | (d.astype(np.float32) >= lim)
    out[y:y + rh, x:x + rw][mask] = 255
    return out


def otsu(hist) -> int:
    """:1564-1630 otsuThreshold from the histogram of the ROI"""
    hist = [int(v) for v in hist]
    n = sum(hist)
    if f64(hist[0]) > f64(n) * f64(0.85):                     # :1588
        return 0
    nz = n - hist[0]
    with np.errstate(all="ignore"):
        pro = [f32(0)] + [f32(hist[j]) / f32(nz) for j in range(1, 256)]     # :1591-1597
        pro = np.array(pro, np.float32)
        jp = np.arange(256, dtype=np.float32) * pro
        # element i of each array is the i-th pass of the outer loop (:1602); the inner loop (:1605-1617) runs here once
        # for all of them, so every pass still adds its terms in j order, one fp32 rounding each
        i = np.arange(256)
        w0, w1, u0t, u1t = (np.zeros(256, np.float32) for _ in range(4))
        for j in range(1, 256):
            lo = j <= i
            w0 = np.where(lo, w0 + pro[j], w0)
            u0t = np.where(lo, u0t + jp[j], u0t)
            w1 = np.where(lo, w1, w1 + pro[j])
            u1t = np.where(lo, u1t, u1t + jp[j])
        u0, u1, u = u0t / w0, u1t / w1, u0t + u1t
        a, b = (u0 - u).astype(np.float64), (u1 - u).astype(np.float64)      # pow(float, 2): a double x*x
        delta = (w0.astype(np.float64) * (a * a) + w1.astype(np.float64) * (b * b)).astype(np.float32)
        best, thr = f32(0), 0
        for k in range(1, 256):
            if delta[k] > best:                               # strict, ascending i; NaN compares false
                best, thr = delta[k], k
    return thr


def _mean(sx, n):
    return f32(sx) / f32(n) if n else f32(0)                  # (float)sum / count, :1403-1452


def _camera(table, px, py, z):
    """our definition of MapDepthPointToCameraSpace (include/sr_yolo2.h): table entry under the rounded point times z"""
    dh, dw = table.shape[:2]
    ix, iy = depth_coord(px, dw), depth_coord(py, dh)
    if ix is None or iy is None:
        return (f32(-np.inf),) * 3
    with np.errstate(all="ignore"):
        return f32(table[iy, ix, 0]) * z, f32(table[iy, ix, 1]) * z, z


def box_stats(box, d16, d8, person, dxy, table):
    """:1482-1562 caculateXYZinCameraSpace (Demo_what branch) + :1632-1706 objectBelong2Person for one frame-relative box
    -> dict with the fields of y2_det3d"""
    H, W = d16.shape
    valid, left, top, right, bot = roi(box, W, H)
    out = dict(valid=0, left=0, top=0, right=0, bot=0, otsu=0, mean_all_mm=0, avg_mm=f32(0), body_id=0, belongs=0,
               cam_x=f32(0), cam_y=f32(0), cam_z=f32(-1), cam_w=f32(0), cam_h=f32(0), pts=np.zeros((5, 2), np.float32))
    if not valid:
        return out
    r16 = d16[top:bot, left:right].astype(np.int64)
    r8 = d8[top:bot, left:right].astype(np.int64)
    rp = person[top:bot, left:right]
    rxy = dxy[top:bot, left:right].astype(np.int64)
    n = r16.size
    o = otsu(np.bincount(r8.ravel(), minlength=256))
    thr = o * 32                                              # :1525
    sum_all = int(r16.sum())
    sel = (r16 > 0) & (r16 < thr)                             # :1332
    idx = int(sel.sum())
    res = int(r16[sel].sum()) // idx if idx else sum_all // n  # :1340-1345 integer division
    avg = f32(res) - f32(16)                                  # :1526
    mapped = rxy[..., 0] >= 0
    masks = [mapped & (r8 < thr), np.zeros_like(mapped), np.zeros_like(mapped), np.zeros_like(mapped), np.zeros_like(mapped)]
    masks[1][0, :] = mapped[0, :]                             # :1380 top, :1385 bottom, :1390 left, :1395 right
    masks[2][-1, :] = mapped[-1, :]
    masks[3][:, 0] = mapped[:, 0]
    masks[4][:, -1] = mapped[:, -1]
    pts = np.zeros((5, 2), np.float32)
    for k, m in enumerate(masks):
        c = int(m.sum())
        pts[k] = (_mean(int(rxy[..., 0][m].sum()), c), _mean(int(rxy[..., 1][m].sum()), c))
    best, label = 0, 0                                        # :1684-1703; a tie goes to the lower label
    for lab in range(1, 7):
        c = int((rp == lab).sum())
        if c > best:
            best, label = c, lab
    belongs = int(f64(f32(best) / f32(n)) > 0.5)              # :1695
    out.update(valid=1, left=left, top=top, right=right, bot=bot, otsu=o, mean_all_mm=sum_all // n, avg_mm=avg,
               body_id=label if belongs else 255, belongs=belongs, pts=pts)
    if table is None:
        return out
    with np.errstate(all="ignore"):
        z = avg / f32(1000)
        c, t, b, l, r = (_camera(table, pts[k, 0], pts[k, 1], z) for k in range(5))
        cam = c
        if any(np.isinf(v) for v in c):                       # :1549-1553
            cam = (f32(0), f32(0), f32(-1))
        ax, ay = l[0] - r[0], l[1] - r[1]
        bx, by = t[0] - b[0], t[1] - b[1]
        cam_w = f32(f64(np.sqrt(f32(ax * ax + ay * ay))) - f64(0.02))     # :1556-1557
        cam_h = np.sqrt(f32(bx * bx + by * by))               # :1558-1559
    out.update(cam_x=cam[0], cam_y=cam[1], cam_z=cam[2], cam_w=cam_w, cam_h=cam_h)
    return out


FIELDS = ("valid", "left", "top", "right", "bot", "otsu", "mean_all_mm", "avg_mm", "body_id", "belongs", "cam_x", "cam_y",
          "cam_z", "cam_w", "cam_h", "pts")


def as_records(stats, dtype):
    out = np.zeros(len(stats), dtype=dtype)
    for i, s in enumerate(stats):
        for k in FIELDS:
            out[i][k] = s[k]
    return out
