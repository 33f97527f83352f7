"""The table-plane removal of the Grasp branch in numpy: the yardstick of tests/test_plane_host.py and
tests/test_gpu_plane.py.  Two things live here.

(a) A restatement of include/y2_plane_rule.h, operation for operation: fp32 where the header is fp32 (np.float32
    scalars and arrays), fp64 where it is fp64 (Python floats are IEEE doubles; math.sqrt is correctly rounded), the same
    reduction tree, the same cyclic Jacobi.  Everything that is compared with it is compared with array_equal.

(b) An INDEPENDENT solver over the same triples: float64 points, np.cross planes, inliers by plain numpy, the refit by
    two-pass np.cov and np.linalg.eigh.  It shares no arithmetic with (a); it says what the answer should be, (a) says
    which bits the library gives.

The reference (KinectUtil_with_cam.cpp:1931-1974 desk_seg, plane_seg.cpp:157-213) runs PCL's RANSAC seeded from the clock
on the closed SDK's cloud, so nothing here is pinned on a reference run."""
from __future__ import annotations

import math

import numpy as np

from tests import depth_rule

f32 = np.float32
f64 = np.float64
MAX_DRAWS, CHUNK, SWEEPS = 64, 1024, 6


# ---------------------------------------------------------------------------
# (a) the header, restated
# ---------------------------------------------------------------------------
def clip(depth, far_m):
    """:1944-1950  g = ((float)d > far_m * 1000.f) ? 0 : d"""
    far_mm = f32(far_m) * f32(1000)
    return np.where(depth.astype(np.float32) > far_mm, 0, depth).astype(np.uint16)


def points(g, tab):
    """z = (float)g / 1000.f; p = (tab.x * z, tab.y * z, z) -> float32 [dh*dw][3]"""
    with np.errstate(all="ignore"):
        z = g.astype(np.float32).ravel() / f32(1000)
        t = tab.astype(np.float32).reshape(-1, 2)
        return np.stack([t[:, 0] * z, t[:, 1] * z, z], axis=-1).astype(np.float32)


def samples(depth, far_m, iters, seed):
    """the sampler: LCG, index = (state >> 8) % n, at most 64 draws per hypothesis, the state running on"""
    g = clip(depth, far_m).ravel()
    n, state = g.size, seed & 0xFFFFFFFF
    out = np.full((iters, 3), -1, np.int32)
    for k in range(iters):
        got = []
        for _ in range(MAX_DRAWS):
            if len(got) == 3:
                break
            state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
            idx = (state >> 8) % n
            if g[idx] > 0 and idx not in got:
                got.append(idx)
        if len(got) == 3:
            out[k] = got
    return out


def plane_of_points(p0, p1, p2):
    """-> (ok, float32 [4] = nx, ny, nz, d), all fp32, every product named"""
    p0, p1, p2 = (np.asarray(p, np.float32) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        ux, uy, uz = p1 - p0
        vx, vy, vz = p2 - p0
        cx, cy, cz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        ln = np.sqrt(f32(f32(cx * cx + cy * cy) + cz * cz))
        if not (ln > 0) or not np.isfinite(ln):
            return 0, np.zeros(4, np.float32)
        nx, ny, nz = cx / ln, cy / ln, cz / ln
        d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
    return 1, np.array([nx, ny, nz, d], np.float32)


def plane_of_triple(g, P, t):
    """void: an index outside the frame, a repeat, a pixel that is not valid, or three points that span no plane"""
    t = [int(v) for v in t]
    if len(set(t)) < 3 or any(v < 0 or v >= g.size for v in t) or any(not g.ravel()[v] > 0 for v in t):
        return 0, np.zeros(4, np.float32)
    return plane_of_points(P[t[0]], P[t[1]], P[t[2]])


def inliers(h, P, dist_m):
    """fabsf((((nx*px) + (ny*py)) + (nz*pz)) + d) < dist_m in fp32, strict"""
    with np.errstate(all="ignore"):
        s = ((h[0] * P[:, 0] + h[1] * P[:, 1]) + h[2] * P[:, 2]) + h[3]
        return np.abs(s) < f32(dist_m)


def tree_sums(P, sel):
    """the ten sums over the selected points through the header's tree: leaves of 4, a halving tree over 256 leaves per
    chunk, the same tree over every 256 chunks, those groups in index order.  Everything not selected, and the padding,
    is +0.0."""
    n = len(P)
    chunks = (n + CHUNK - 1) // CHUNK
    x, y, z = (P[:, k].astype(np.float64) for k in range(3))
    terms = np.stack([np.ones(n), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=-1)
    v = np.zeros((chunks * CHUNK, 10), np.float64)
    v[:n][sel] = terms[sel]
    v = v.reshape(chunks, 256, 4, 10)
    a = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) + v[:, :, 3]                # [chunks][256][10]
    s = 128
    while s > 0:
        a = a[:, :s] + a[:, s:2 * s]
        s //= 2
    part = a[:, 0]                                                          # [chunks][10]
    groups = (chunks + 255) // 256
    b = np.zeros((groups * 256, 10), np.float64)
    b[:chunks] = part
    b = b.reshape(groups, 256, 10)
    s = 128
    while s > 0:
        b = b[:, :s] + b[:, s:2 * s]
        s //= 2
    total = b[0, 0].copy()
    for m in range(1, groups):
        total = total + b[m, 0]
    return total


def _rotate(A, V, p, q, r):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    at = -theta if theta < 0.0 else theta
    tt = theta * theta
    t = 1.0 / (at + math.sqrt(tt + 1.0))
    if theta < 0.0:
        t = -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    app, aqq = A[p][p] - t * apq, A[q][q] + t * apq
    arp, arq = c * A[r][p] - s * A[r][q], s * A[r][p] + c * A[r][q]
    A[p][p], A[q][q], A[p][q], A[q][p] = app, aqq, 0.0, 0.0
    A[r][p] = A[p][r] = arp
    A[r][q] = A[q][r] = arq
    for k in range(3):
        vp, vq = c * V[k][p] - s * V[k][q], s * V[k][p] + c * V[k][q]
        V[k][p], V[k][q] = vp, vq


def fit(S):
    """the refit from the ten sums -> (ok, float64 [4]); Python floats are the header's doubles"""
    S = [float(v) for v in S]
    n = S[0]
    if not n >= 3.0:
        return 0, np.zeros(4)
    mx, my, mz = S[1] / n, S[2] / n, S[3] / n
    A = [[0.0] * 3 for _ in range(3)]
    A[0][0], A[0][1], A[0][2] = S[4] / n - mx * mx, S[5] / n - mx * my, S[6] / n - mx * mz
    A[1][1], A[1][2], A[2][2] = S[7] / n - my * my, S[8] / n - my * mz, S[9] / n - mz * mz
    A[1][0], A[2][0], A[2][1] = A[0][1], A[0][2], A[1][2]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    best = 0
    if A[1][1] < A[best][best]:
        best = 1
    if A[2][2] < A[best][best]:
        best = 2
    nx, ny, nz = V[0][best], V[1][best], V[2][best]
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    if not ln > 0.0 or not math.isfinite(ln):
        return 0, np.zeros(4)
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    d = -((nx * mx + ny * my) + nz * mz)
    if d < 0.0:
        nx, ny, nz, d = -nx, -ny, -nz, -d
    return 1, np.array([nx, ny, nz, d], np.float64)


def removes(pl, P, dist_m):
    """PCL re-selects after optimising: fabs(a*x + b*y + c*z + d) < (double)dist_m"""
    Pd = P.astype(np.float64)
    with np.errstate(all="ignore"):
        s = ((pl[0] * Pd[:, 0] + pl[1] * Pd[:, 1]) + pl[2] * Pd[:, 2]) + pl[3]
        return np.abs(s) < float(f32(dist_m))


def remove_plane(depth, tab, far_m, dist_m, triples):
    """the whole rule -> (dict of the fields of y2_plane, grasp_depth [dh][dw] uint16)"""
    g = clip(depth, far_m)
    gv = g.ravel()
    valid = gv > 0
    P = points(g, tab)
    counts = []
    for t in triples:
        ok, h = plane_of_triple(g, P, t)
        counts.append(int((inliers(h, P, dist_m) & valid).sum()) if ok else 0)
    best = int(np.argmax(counts)) if counts else 0            # the largest count, a tie to the lowest k
    rec = dict(found=0, best=-1, valid_points=int(valid.sum()), best_count=0, removed=0, a=0.0, b=0.0, c=0.0, d=0.0)
    if rec["valid_points"] < 3 or not counts or counts[best] < 3:
        return rec, g
    _, h = plane_of_triple(g, P, triples[best])
    ok, pl = fit(tree_sums(P, inliers(h, P, dist_m) & valid))
    if not ok:
        return rec, g
    gone = removes(pl, P, dist_m) & valid
    rec.update(found=1, best=best, best_count=counts[best], removed=int(gone.sum()), a=pl[0], b=pl[1], c=pl[2], d=pl[3])
    return rec, np.where(gone, 0, gv).astype(np.uint16).reshape(g.shape)


def register(grasp_depth, dxy):
    """:402-438: grasp16 of a colour pixel is the grasp depth under its (dx, dy), 0 where unmapped"""
    ok = dxy[..., 0] >= 0
    yy, xx = np.where(ok, dxy[..., 1], 0), np.where(ok, dxy[..., 0], 0)
    return np.where(ok, grasp_depth[yy, xx], 0).astype(np.uint16)


def box_stats_grasp(box, d16, d8, person, dxy, table, g16):
    """:1508-1518, the Grasp branch of caculateXYZinCameraSpace: thr = 255 * 32, avg_mm = GetImgAvg(grasp16 ROI, thr) with
    nothing subtracted (:1321-1346: integer sum and division, sumAll / (cols * rows) when nothing passes), the centre
    point over every mapped pixel (depth8 < thr always holds), otsu reported as 255; the rest as the Demo_what branch"""
    out = depth_rule.box_stats(box, d16, d8, person, dxy, table)
    if not out["valid"]:
        return out
    left, top, right, bot = (out[k] for k in ("left", "top", "right", "bot"))
    rg = g16[top:bot, left:right].astype(np.int64)
    rxy = dxy[top:bot, left:right].astype(np.int64)
    thr = 255 * 32
    sel = (rg > 0) & (rg < thr)
    idx = int(sel.sum())
    res = int(rg[sel].sum()) // idx if idx else int(rg.sum()) // rg.size
    avg = f32(res)
    mapped = rxy[..., 0] >= 0
    c = int(mapped.sum())
    pts = out["pts"].copy()
    pts[0] = (depth_rule._mean(int(rxy[..., 0][mapped].sum()), c), depth_rule._mean(int(rxy[..., 1][mapped].sum()), c))
    out.update(otsu=255, avg_mm=avg, pts=pts)
    if table is None:
        return out
    with np.errstate(all="ignore"):
        z = avg / f32(1000)
        c_, t, b, l, r = (depth_rule._camera(table, pts[k, 0], pts[k, 1], z) for k in range(5))
        cam = c_
        if any(np.isinf(v) for v in c_):
            cam = (f32(0), f32(0), f32(-1))
        ax, ay = l[0] - r[0], l[1] - r[1]
        bx, by = t[0] - b[0], t[1] - b[1]
        cam_w = f32(f64(np.sqrt(f32(ax * ax + ay * ay))) - f64(0.02))
        cam_h = np.sqrt(f32(bx * bx + by * by))
    out.update(cam_x=cam[0], cam_y=cam[1], cam_z=cam[2], cam_w=cam_w, cam_h=cam_h)
    return out


# ---------------------------------------------------------------------------
# (b) the independent solver
# ---------------------------------------------------------------------------
def solve_independent(depth, tab, far_m, dist_m, triples):
    """-> (found, float64 [4] coefficients, removed mask [dh][dw], |distance| of every pixel to the plane [dh][dw])"""
    g = np.where(depth.astype(np.float64) > far_m * 1000.0, 0, depth).astype(np.float64)
    valid = (g > 0).ravel()
    z = g.ravel() / 1000.0
    t = tab.astype(np.float64).reshape(-1, 2)
    P = np.stack([t[:, 0] * z, t[:, 1] * z, z], axis=-1)
    best_n, best_count = None, -1
    for tri in triples:
        tri = [int(v) for v in tri]
        if len(set(tri)) < 3 or min(tri) < 0 or max(tri) >= len(P) or not valid[tri].all():
            continue
        n = np.cross(P[tri[1]] - P[tri[0]], P[tri[2]] - P[tri[0]])
        ln = np.linalg.norm(n)
        if not ln > 0:
            continue
        n = n / ln
        count = int(((np.abs(P @ n - n @ P[tri[0]]) < dist_m) & valid).sum())
        if count > best_count:
            best_n, best_d, best_count = n, -(n @ P[tri[0]]), count
    none = (0, np.zeros(4), np.zeros(depth.shape, bool), np.full(depth.shape, np.inf))
    if valid.sum() < 3 or best_count < 3:
        return none
    inl = (np.abs(P @ best_n + best_d) < dist_m) & valid
    Q = P[inl]
    w, v = np.linalg.eigh(np.cov(Q.T, bias=True))
    n = v[:, 0]
    d = -(n @ Q.mean(axis=0))
    if d < 0:
        n, d = -n, -d
    dist = np.abs(P @ n + d)
    return 1, np.array([n[0], n[1], n[2], d]), ((dist < dist_m) & valid).reshape(depth.shape), dist.reshape(depth.shape)


# ---------------------------------------------------------------------------
# the seeded scene
# ---------------------------------------------------------------------------
NONE, TABLE, OBJECT, FAR = 0, 1, 2, 3


def camera_table(dh, dw):
    """a pinhole table in the manner of GetDepthFrameToCameraSpaceTable: ((x - cx) / f, (cy - y) / f), f = 0.71 * dw"""
    f = 0.71 * dw
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    return np.stack([(xs - (dw - 1) / 2.0) / f, ((dh - 1) / 2.0 - ys) / f], axis=-1).astype(np.float32)


def scene(dh, dw, seed):
    """A tilted table with +-4 mm of noise, three boxes standing 80-160 mm nearer the camera, 5 % dropped pixels and the
    far part of the table beyond 1 m -> (depth uint16 [dh][dw], table float32 [dh][dw][2], label uint8 [dh][dw])"""
    rng = np.random.default_rng(seed)
    tab = camera_table(dh, dw)
    n = np.array([0.04, 0.5, 0.865])
    n = n / np.linalg.norm(n)
    z = 0.70 / (n[0] * tab[..., 0].astype(np.float64) + n[1] * tab[..., 1].astype(np.float64) + n[2])     # metres along the ray
    mm = np.rint(z * 1000.0) + rng.integers(-4, 5, (dh, dw))
    label = np.full((dh, dw), TABLE, np.uint8)
    for k in range(3):                                        # boxes in the near two thirds of the frame
        bh, bw = max(3, dh // 6), max(3, dw // 8)
        top = int(rng.integers(dh // 12, dh // 2 - bh))
        left = int(rng.integers(1 + k * (dw // 3), (k + 1) * (dw // 3) - bw))
        mm[top:top + bh, left:left + bw] -= rng.integers(80, 161, (bh, bw))
        label[top:top + bh, left:left + bw] = OBJECT
    label[mm > 1000] = FAR
    drop = rng.random((dh, dw)) < 0.05
    mm[drop] = 0
    label[drop] = NONE
    return mm.astype(np.uint16), tab, label


def color_map(h, w, dh, dw, seed):
    """a random sub-pixel colour -> depth map of an h x w colour frame, with coordinates off the depth frame, a block that
    maps nowhere and values that are not finite"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    m = np.stack([xs * np.float32((dw + 3.0) / w) - np.float32(1.5) + rng.uniform(-0.6, 0.6, (h, w)).astype(np.float32),
                  ys * np.float32((dh + 3.0) / h) - np.float32(1.5) + rng.uniform(-0.6, 0.6, (h, w)).astype(np.float32)],
                 axis=-1).astype(np.float32)
    m[h // 2:h // 2 + 5, w // 3:w // 3 + 9] = np.float32(-7.0)
    m[1, 2] = (np.nan, 3.0)
    m[2, 5] = (4.0, np.inf)
    m[3, 7] = (3e9, 1.0)
    return m


SCENES = [(48, 64, 11), (53, 67, 12), (106, 128, 13)]          # (dh, dw, seed): depth 64 x 48, 67 x 53, 128 x 106
FAR_M, DIST_M, ITERS, SEED = 1.0, 0.02, 50, 2017
