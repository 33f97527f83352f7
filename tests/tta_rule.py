"""The rule of the reference's multi-view classifier evaluations (classifier.c:336-593), stated in numpy: crop_image with
its clamped taps (image.c:1512-1532), flip_image (image.c:1056-1070), resize_min's dimensions (image.c:1662-1672), the
view list of each mode and the sequential fp32 sum of the predictions (axpy_cpu, classifier.c:393,577,580).  The
fixtures, the host tests and the GPU tests all build their views from here."""
from __future__ import annotations

import numpy as np

from sr_object_detection_amd import synth, zoo

CROP10, MULTI, FULL = 0, 1, 2
DEFAULT_SCALES = (224, 288, 320, 352, 384)          # classifier.c:550
SHIFT = 32                                          # classifier.c:375
CROP10_SHIFTS = ((-32, -32), (32, -32), (0, 0), (-32, 32), (32, 32))     # (dx, dy), classifier.c:378-382

# the test network: small, fully convolutional, resizable; 3 channels, nominal 32 x 32, 10 classes
MINI_SPEC = [("conv", 16, 3, 1, "leaky"), ("max", 2, 2), ("conv", 32, 3, 1, "leaky"), ("max", 2, 2),
             ("conv", 10, 1, 0, "linear"), ("avg",), ("softmax",), ("cost",)]
# the same trunk with a dense head: resize_network refuses it
DENSE_SPEC = [("conv", 16, 3, 1, "leaky"), ("max", 2, 2), ("conv", 32, 3, 1, "leaky"), ("max", 2, 2),
              ("connected", 10, 0, "linear"), ("softmax",), ("cost",)]
MINI_SIZE, MINI_CLASSES = 32, 10
MINI_SCALES = (24, 32, 40)
FRAME_SIZES = ((50, 40), (40, 50), (64, 64), (33, 47))       # (w, h)


def crop_image(im: np.ndarray, dx: int, dy: int, w: int, h: int) -> np.ndarray:
    """im [c][sh][sw] -> [c][h][w]; taps outside the source repeat its edge (constrain_int)"""
    sh, sw = im.shape[1:]
    r = np.clip(np.arange(h) + dy, 0, sh - 1)
    c = np.clip(np.arange(w) + dx, 0, sw - 1)
    return np.ascontiguousarray(im[:, r[:, None], c[None, :]])


def flip_image(im: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(im[:, :, ::-1])


def view(im: np.ndarray, dx: int, dy: int, w: int, h: int, flip: int) -> np.ndarray:
    """what one y2h_view descriptor stands for"""
    return crop_image(flip_image(im) if flip else im, dx, dy, w, h)


def resize_min_dims(w: int, h: int, m: int):
    if w < h:
        return m, (h * m) // w
    return (w * m) // h, m


def stage_size(mode: int, frame_wh, net_w: int, net_h: int, scale: int):
    if mode == CROP10:
        return net_w + SHIFT, net_h + SHIFT
    return resize_min_dims(frame_wh[0], frame_wh[1], scale)


def mode_scales(mode: int, net_w: int, scales=None):
    if mode == CROP10:
        return (0,)
    if mode == FULL:
        return (net_w,)
    return tuple(scales) if scales is not None else DEFAULT_SCALES


def views_of(mode: int, frame: np.ndarray, net_w: int, net_h: int, resize, scales=None):
    """The views of one frame in the reference's order: list of (network (w, h), view [c][h][w]).  `resize` is
    resize_image(im, w, h); it is not called when the size is already right (image.c:1673, :2084)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    out = []
    for s in mode_scales(mode, net_w, scales):
        rw, rh = stage_size(mode, (frame.shape[2], frame.shape[1]), net_w, net_h, s)
        im = frame if (rw, rh) == (frame.shape[2], frame.shape[1]) else resize(frame, rw, rh)
        if mode == CROP10:
            for flip in (0, 1):
                for dx, dy in CROP10_SHIFTS:
                    out.append(((net_w, net_h), view(im, dx, dy, net_w, net_h, flip)))
        else:
            out.append(((rw, rh), im))
            if mode == MULTI:
                out.append(((rw, rh), flip_image(im)))
    return out


def sequential_sum(rows) -> np.ndarray:
    """pred = 0; pred += row, one fp32 rounding per addition, in order"""
    acc = np.zeros_like(np.asarray(rows[0], dtype=np.float32))
    for r in rows:
        acc = (acc + np.asarray(r, dtype=np.float32)).astype(np.float32)
    return acc


def top_k(a: np.ndarray, k: int) -> np.ndarray:
    """utils.c:179: the k largest, each found by a scan that keeps the first of equals"""
    a = np.asarray(a, dtype=np.float32)
    idx = []
    for _ in range(k):
        best = -1
        for i in range(a.size):
            if i in idx:
                continue
            if best < 0 or a[i] > a[best]:
                best = i
        idx.append(best)
    return np.array(idx, dtype=np.int32)


def progress(sums: np.ndarray, truth, classes: int, topk: int):
    """the lines the validate loops print (classifier.c:397-404) and the final (top-1, top-k) averages, in C float"""
    acc = np.float32(0)
    tk = np.float32(0)
    lines = []
    for i, s in enumerate(sums):
        idx = top_k(s[:classes], topk)
        if idx[0] == truth[i]:
            acc = np.float32(acc + np.float32(1))
        for j in idx:
            if j == truth[i]:
                tk = np.float32(tk + np.float32(1))
        lines.append("%d: top 1: %f, top %d: %f" % (i, np.float32(acc / np.float32(i + 1)), topk, np.float32(tk / np.float32(i + 1))))
    n = np.float32(len(sums))
    return lines, float(np.float32(acc / n)), float(np.float32(tk / n))


def mini_frames(seed: int):
    """the four test frames [3][h][w], values in [0, 1)"""
    return [synth.uniform01(seed + i, 3 * h * w).reshape(3, h, w) for i, (w, h) in enumerate(FRAME_SIZES)]


def write_mini(tmp: str, seed: int, w: int = MINI_SIZE, h: int = MINI_SIZE, batch: int = 1, spec=None, tag: str = "mini"):
    """cfg + weights of the test network at (w, h, batch) -> (cfg path, weights path)"""
    import os
    spec = MINI_SPEC if spec is None else spec
    cfg = os.path.join(tmp, "tta_%s_%dx%d_b%d.cfg" % (tag, w, h, batch))
    with open(cfg, "w") as f:
        f.write(zoo.cfg_text(tag, w, h, batch, spec=spec))
    wts = os.path.join(tmp, "tta_%s_s%d.weights" % (tag, seed))
    if not os.path.exists(wts):
        synth.write_weights(wts, zoo.resolve(spec, MINI_SIZE), seed, 1.0)
    return cfg, wts


def rows_of(views, predict):
    """Predict a list of (size, view) in groups of equal size: predict((w, h), x [k][c][h][w]) -> [k][outputs].
    Returns the rows in the order of `views`."""
    rows = [None] * len(views)
    sizes = []
    for size, _ in views:
        if size not in sizes:
            sizes.append(size)
    for size in sizes:
        idx = [i for i, (s, _) in enumerate(views) if s == size]
        out = np.asarray(predict(size, np.stack([views[i][1] for i in idx])), dtype=np.float32).reshape(len(idx), -1)
        for k, i in enumerate(idx):
            rows[i] = out[k]
    return np.stack(rows)


def mode_views(mode: int, frames, resize, scales=None, net_w: int = MINI_SIZE, net_h: int = MINI_SIZE):
    """every view of every frame, frame-major -> (list of (size, view), views per frame)"""
    views = []
    for f in frames:
        views += views_of(mode, f, net_w, net_h, resize, scales)
    return views, len(views) // len(frames)


def sums_of(rows: np.ndarray, per: int) -> np.ndarray:
    return np.stack([sequential_sum(rows[i:i + per]) for i in range(0, len(rows), per)])
