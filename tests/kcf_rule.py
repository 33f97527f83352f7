"""The KCF tracker of the Kinect loop (kcf.cpp, complexmat.hpp, piotr_fhog/) restated in numpy: the one statement the
tracker tests and tests/golden/gen_kcf_golden.py share.  Every function takes the working type `dt`: numpy.float64 is the
yardstick T64 of the tests, numpy.float32 the stand-in reference where no compiled one exists (its DFTs are scipy.fft in
single precision).

Defined here and not by OpenCV (parity with OpenCV unpinned, as oracle/tracking.py says for Detector::tracking):
  grey     (1868*B + 9617*G + 4899*R + 8192) >> 14 of an 8-bit BGR / BGRA pixel (CV_BGR2GRAY's fixed-point constants); a
           1-channel frame is taken as is
  halving  cv::resize(.., 0.5, 0.5, INTER_CUBIC): output round-half-even(0.5*cols) x round-half-even(0.5*rows), taps
           (-3, 19, 19, -3)/32 at source columns 2d-1 .. 2d+2 clamped to the image, horizontal pass first, then vertical,
           each sum taken left to right
The orientation of fHOG is exact arithmetic here; the reference reads a 10000-entry arc-cosine table."""
import math

import numpy as np

PADDING = 3.0
KERNEL_SIGMA = 0.5
LAMBDA = 1e-4
INTERP = 0.02
OUTPUT_SIGMA_FACTOR = 0.1
CELL = 4
NORIENT = 9
CLIP = 0.2
CHANNELS = 31
MAX_TRACKERS = 32
MAX_CELLS = 256


# ---------------------------------------------------------------- grey, halving, sub-window
def grey(frame):
    f = np.asarray(frame)
    if f.ndim == 2 or f.shape[2] == 1:
        return f.reshape(f.shape[0], f.shape[1]).astype(np.float32)
    b, g, r = (f[:, :, k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.float32)


def half_size(n):
    return n // 2 + ((n & 1) and ((n // 2) & 1))


def _cubic_axis(a, dt, axis):
    a = np.moveaxis(np.asarray(a, dt), axis, 0)
    n = a.shape[0]
    d = np.arange(half_size(n))
    taps = [np.clip(2 * d + k, 0, n - 1) for k in (-1, 0, 1, 2)]
    w = [dt(-3.0 / 32), dt(19.0 / 32), dt(19.0 / 32), dt(-3.0 / 32)]
    out = w[0] * a[taps[0]]
    for k in (1, 2, 3):
        out = out + w[k] * a[taps[k]]
    return np.moveaxis(out.astype(dt), 0, axis)


def halve(img, dt):
    return _cubic_axis(_cubic_axis(img, dt, 1), dt, 0)


def get_subwindow(img, cx, cy, width, height):
    """kcf.cpp:277-325; cx, cy are the doubles of the pose, truncated as the `int` parameters truncate them"""
    rows, cols = img.shape
    cx, cy = int(cx), int(cy)                                # C truncation toward zero
    x1, y1, x2, y2 = cx - width // 2, cy - height // 2, cx + width // 2, cy + height // 2
    zeros = np.zeros((height, width), img.dtype)
    if x1 >= cols or y1 >= rows or x2 < 0 or y2 < 0:
        return zeros
    top = left = 0
    if x1 < 0:
        left, x1 = -x1, 0
    if y1 < 0:
        top, y1 = -y1, 0
    x2 = cols if x2 >= cols else x2 + width % 2
    y2 = rows if y2 >= rows else y2 + height % 2
    if x2 - x1 == 0 or y2 - y1 == 0:
        return zeros
    jj = np.clip(np.arange(width) - left, 0, x2 - x1 - 1) + x1
    ii = np.clip(np.arange(height) - top, 0, y2 - y1 - 1) + y1
    return img[np.ix_(ii, jj)]


# ---------------------------------------------------------------- fHOG (fhog.hpp:22-97, gradientMex.cpp)
def grad_mag(patch, dt):
    """gradMag with full = true on I / 255: central differences, one-sided at the borders; M; O in [0, 2*pi)"""
    I = np.asarray(patch, dt) / dt(255)
    gx = np.empty_like(I)
    gy = np.empty_like(I)
    gx[:, 1:-1] = (I[:, 2:] - I[:, :-2]) * dt(0.5)
    gx[:, 0] = I[:, 1] - I[:, 0]
    gx[:, -1] = I[:, -1] - I[:, -2]
    gy[1:-1, :] = (I[2:, :] - I[:-2, :]) * dt(0.5)
    gy[0, :] = I[1, :] - I[0, :]
    gy[-1, :] = I[-1, :] - I[-2, :]
    M = np.sqrt(gx * gx + gy * gy).astype(dt)
    O = np.arctan2(gy.astype(np.float64), gx.astype(np.float64))
    O = np.where(O < 0, O + 2 * math.pi, O)
    return M, O


def orient_bin(O):
    """the hard bin of gradQuantize: (int)(o * oMult + .5f), wrapped at 18; also the distance to the nearest boundary"""
    t = O * (2 * NORIENT / (2 * math.pi)) + 0.5
    b = np.floor(t).astype(np.int64)
    frac = t - b
    return np.where(b >= 2 * NORIENT, 0, b), np.minimum(frac, 1 - frac)


def fhog(patch, dt):
    """FHoG::extract(patch, 2, 4, 9): [31][hb][wb]"""
    h, w = patch.shape
    hb, wb = h // CELL, w // CELL
    h0, w0 = hb * CELL, wb * CELL
    M, O = grad_mag(patch, dt)
    bins, _ = orient_bin(O)
    nor = 2 * NORIENT
    # gradHist, softBin = -1: hard orientation, bilinear in space, column by column as the reference walks them
    R1 = np.zeros((nor, hb, wb), dt)
    xs, ys = np.meshgrid(np.arange(w0), np.arange(h0), indexing="ij")       # x outer, y inner
    xs, ys = xs.ravel(), ys.ravel()
    m = (M[ys, xs] * dt(1.0 / (CELL * CELL))).astype(dt)
    o = bins[ys, xs]
    xb = ((xs + dt(0.5)) * dt(1.0 / CELL) - dt(0.5)).astype(dt)
    yb = ((ys + dt(0.5)) * dt(1.0 / CELL) - dt(0.5)).astype(dt)
    xb0 = np.where(xb >= 0, np.floor(xb), -1).astype(np.int64)
    yb0 = np.where(yb >= 0, np.floor(yb), -1).astype(np.int64)
    xd, yd = (xb - xb0).astype(dt), (yb - yb0).astype(dt)
    xyd = (xd * yd).astype(dt)
    ms = [(dt(1) - xd - yd + xyd).astype(dt), (yd - xyd).astype(dt), (xd - xyd).astype(dt), xyd]
    for k, (dx, dy) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        cx_, cy_ = xb0 + dx, yb0 + dy
        ok = (cx_ >= 0) & (cx_ < wb) & (cy_ >= 0) & (cy_ < hb)
        np.add.at(R1, (o[ok], cy_[ok], cx_[ok]), (ms[k][ok] * m[ok]).astype(dt))
    f87 = dt(8.0) / dt(7.0)
    R1[:, :, 0] *= f87
    R1[:, 0, :] *= f87
    R1[:, :, wb - 1] *= f87
    R1[:, hb - 1, :] *= f87
    R2 = (R1[:NORIENT] + R1[NORIENT:]).astype(dt)
    # hogNormMatrix
    S = np.zeros((hb, wb), dt)
    for k in range(NORIENT):
        S = S + R2[k] * R2[k]
    eps = dt(np.float32(1e-4) / 4 / CELL / CELL / CELL / CELL)
    Nv = (dt(1) / np.sqrt(S[:-1, :-1] + S[1:, :-1] + S[:-1, 1:] + S[1:, 1:] + eps)).astype(dt)   # [hb-1][wb-1]
    # N[X][Y] of the padded matrix is Nv[clamp(Y, 1, hb-1) - 1][clamp(X, 1, wb-1) - 1]
    Y = np.clip(np.arange(hb + 1), 1, hb - 1) - 1
    X = np.clip(np.arange(wb + 1), 1, wb - 1) - 1
    N = Nv[np.ix_(Y, X)]                                                   # [hb+1][wb+1], indexed [Y][X]
    blocks = [N[1:, 1:], N[:-1, 1:], N[1:, :-1], N[:-1, :-1]]              # GETT(0), (1), (hb1), (hb1 + 1)
    H = np.zeros((CHANNELS, hb, wb), dt)
    clip, half, r = dt(np.float32(CLIP)), dt(0.5), dt(np.float32(0.2357))
    for base, R in ((0, R1), (nor, R2)):
        for k in range(R.shape[0]):
            acc = np.zeros((hb, wb), dt)
            for Nb in blocks:
                acc = acc + np.minimum(R[k] * Nb, clip) * half
            H[base + k] = acc
    for c, Nb in enumerate(blocks):
        acc = np.zeros((hb, wb), dt)
        for k in range(nor):
            acc = acc + np.minimum(R1[k] * Nb, clip) * r
        H[nor + NORIENT + c] = acc
    return H


# ---------------------------------------------------------------- window, labels, DFT
def cosine_window(cols, rows):
    def one(n):
        with np.errstate(divide="ignore", invalid="ignore"):
            return (0.5 * (1. - np.cos(2. * math.pi * np.arange(n, dtype=np.float64) * (1. / (float(n) - 1.))))).astype(np.float32)
    return one(rows), one(cols)


def circshift(a, x_rot, y_rot):
    return np.roll(a, (y_rot, x_rot), axis=(0, 1))


def gaussian_labels(sigma, dim1, dim2):
    ys = np.arange(-(dim2 // 2), dim2 - dim2 // 2, dtype=np.float64)
    xs = np.arange(-(dim1 // 2), dim1 - dim1 // 2, dtype=np.float64)
    lab = np.exp(-0.5 * (ys[:, None] ** 2 + xs[None, :] ** 2) / (sigma * sigma)).astype(np.float32)
    return circshift(lab, -(dim1 // 2), -(dim2 // 2))


def fft2(a, dt):
    if dt == np.float32:
        import scipy.fft
        return scipy.fft.fft2(np.asarray(a, np.float32)).astype(np.complex64)
    return np.fft.fft2(np.asarray(a, np.float64))


def ifft2_real(a, dt):
    if dt == np.float32:
        import scipy.fft
        return scipy.fft.ifft2(np.asarray(a, np.complex64)).real.astype(np.float32)
    return np.fft.ifft2(a).real


def windowed_fft(feat, win, dt):
    wr, wc = win
    return fft2(np.asarray(feat, dt) * (wr.astype(dt)[:, None] * wc.astype(dt)[None, :]).astype(dt), dt)


def sqr_norm(xf, dt):
    return dt((xf.real.astype(dt) ** 2 + xf.imag.astype(dt) ** 2).sum(dtype=dt) / dt(xf.shape[-1] * xf.shape[-2]))


def gaussian_correlation(xf, yf, dt, auto=False):
    """kcf.cpp:327-351; the channels are summed before one inverse DFT (the DFT is linear)"""
    xx = sqr_norm(xf, dt)
    yy = xx if auto else sqr_norm(yf, dt)
    xyf = (xf * np.conj(yf)).sum(axis=0)
    xy = ifft2_real(xyf, dt)
    numel_inv = dt(1.0) / dt(xf.shape[0] * xf.shape[1] * xf.shape[2])
    arg = np.maximum((xx + yy - dt(2) * xy) * numel_inv, dt(0))
    g = np.exp(dt(-1.0 / (KERNEL_SIGMA * KERNEL_SIGMA)) * arg).astype(dt)
    return fft2(g, dt), g


# ---------------------------------------------------------------- the tracker
def plan(box):
    """init's arithmetic (kcf.cpp:7-27) -> dict of y2_kcf_geometry's fields"""
    cx, cy, w, h = (float(v) for v in box)
    resized = int(w * h > 100. * 100.)
    if resized:
        cx, cy, w, h = cx * 0.5, cy * 0.5, w * 0.5, h * 0.5
    win_w, win_h = int(math.floor(w * (1. + PADDING))), int(math.floor(h * (1. + PADDING)))
    return dict(resized=resized, win_w=win_w, win_h=win_h, cells_w=win_w // CELL, cells_h=win_h // CELL, cx=cx, cy=cy, w=w, h=h,
                output_sigma=math.sqrt(w * h) * OUTPUT_SIGMA_FACTOR / float(CELL))


class Tracker:
    """KCF_Tracker with the fork's defaults (kcf.h:51-57)"""

    def __init__(self, dt):
        self.dt = dt
        self.ct = np.complex64 if dt == np.float32 else np.complex128

    def _input(self, frame):
        g = grey(frame).astype(self.dt)
        return halve(g, self.dt) if self.g["resized"] else g

    def _features(self, img, cx, cy):
        patch = get_subwindow(img, cx, cy, self.g["win_w"], self.g["win_h"])
        feat = fhog(patch, self.dt)
        return patch, feat, windowed_fft(feat, self.win, self.dt).astype(self.ct)

    def init(self, frame, box):
        dt = self.dt
        self.g = g = plan(box)
        self.cx, self.cy = g["cx"], g["cy"]
        self.yf = fft2(gaussian_labels(g["output_sigma"], g["cells_w"], g["cells_h"]), dt).astype(self.ct)
        self.win = cosine_window(g["cells_w"], g["cells_h"])
        self.patch, self.feat, self.model_xf = self._features(self._input(frame), self.cx, self.cy)
        kf, _ = gaussian_correlation(self.model_xf, self.model_xf, dt, auto=True)
        self.model_alphaf = (self.yf / (kf + dt(LAMBDA))).astype(self.ct)
        return self

    def bbox(self, cx=None, cy=None):
        s = 2.0 if self.g["resized"] else 1.0
        cx = self.cx if cx is None else cx
        cy = self.cy if cy is None else cy
        return (cx * s, cy * s, self.g["w"] * s, self.g["h"] * s)

    def track(self, frame, update=True):
        """-> (box, peak); self.response is the response map.  update = False: the application's copy-and-drop call."""
        dt = self.dt
        img = self._input(frame)
        self.patch, self.feat, zf = self._features(img, self.cx, self.cy)
        kzf, _ = gaussian_correlation(zf, self.model_xf, dt)
        self.response = resp = ifft2_real(self.model_alphaf * kzf, dt)
        rows, cols = resp.shape
        at = int(np.argmax(resp))                            # the first maximum in row-major order
        my, mx = at // cols, at % cols
        self.peak = float(resp[my, mx])
        if my > rows // 2:
            my -= rows
        if mx > cols // 2:
            mx -= cols
        self.max_loc = (mx, my)
        cx, cy = self.cx + CELL * mx, self.cy + CELL * my
        if update:
            self.cx, self.cy = cx, cy
            _, _, xf = self._features(img, cx, cy)
            kf, _ = gaussian_correlation(xf, xf, dt, auto=True)
            alphaf = self.yf / (kf + dt(LAMBDA))
            self.model_xf = (self.model_xf * dt(1. - INTERP) + xf * dt(INTERP)).astype(self.ct)
            self.model_alphaf = (self.model_alphaf * dt(1. - INTERP) + alphaf * dt(INTERP)).astype(self.ct)
        return self.bbox(cx, cy), self.peak


def err(a, t64):
    """the project's error measure: max|A - T64| / max|T64|"""
    a, t64 = np.asarray(a), np.asarray(t64)
    m = float(np.max(np.abs(t64)))
    return float(np.max(np.abs(a.astype(t64.dtype) - t64))) / (m if m > 0 else 1.0)


def bound(err_ref):
    return 4 * err_ref + 4 * 2.0 ** -23


def planes(z):
    """complex [..][R][C] -> the library's layout [..][2][R][C] (real plane, imaginary plane)"""
    return np.stack([z.real, z.imag], axis=-3)
