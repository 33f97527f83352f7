"""The pixel chain of the reference's classifier loader, restated in numpy on the WHOLE frame: what load_image_augment_paths
(src_yolo2/data.c:107-132) does to one image between load_image_color and X.vals[i] --

    (float)(v / 255.)       image.c:2045-2067
    rotate_crop_image       image.c:1462-1479   rx, ry per output pixel: every operand that is a double in C makes the operation
                                                a double one, so (x - w/2.)/s*aspect and (y - h/2.)/s are double operations on
                                                the promoted floats, while dx/s*aspect and dy/s -- three floats -- are FLOAT
                                                operations whose result is promoted; cos(rad), sin(rad) take (double)rad;
                                                the sum is rounded to float once, at the assignment
    bilinear_interpolate    image.c:1935-1948   floorf, float weights, four taps summed left to right
    get_pixel_extend        image.c:2112-2120   x and y clamped into the frame (nothing is zero outside)
    flip_image              image.c:1056-1070   on the crop
    distort_image           image.c:1903-1916   tests/aug_rule.py's, by import

cos and sin come from the C library the product's host half calls (ctypes.CDLL("libm.so.6")), not from numpy: the last bit of
either decides a tap.  It knows nothing of the packer: it reads the frame itself.

PROVENANCE: parity with a run of the reference unpinned (image.c needs OpenCV and is not in oracle/_ref/libdarknet_ref.so), as
for tests/aug_rule.py.  The draws, the sequence around them and the label rows ARE pinned to the compiled reference:
tests/golden/aug_cls.npz (tests/golden/gen_aug_cls_golden.py).
"""
import ctypes

import numpy as np

from tests.aug_rule import distort, planes

F = np.float32
D = np.float64

_libm = ctypes.CDLL("libm.so.6")
_libm.cos.restype = ctypes.c_double
_libm.cos.argtypes = [ctypes.c_double]
_libm.sin.restype = ctypes.c_double
_libm.sin.argtypes = [ctypes.c_double]


def coords(ow, oh, size, rad, scale, dx, dy, aspect):
    """rotate_crop_image's (rx, ry) as float32 [size][size] (row y, column x)"""
    rad, s32, dx, dy, a32 = F(rad), F(scale), F(dx), F(dy), F(aspect)
    cosr, sinr = D(_libm.cos(float(rad))), D(_libm.sin(float(rad)))
    s, a = D(s32), D(a32)
    cx, cy = F(D(ow) / D(2.)), F(D(oh) / D(2.))
    with np.errstate(all="ignore"):
        ax = D(F(F(dx / s32) * a32))
        ay = D(F(dy / s32))
        half = D(size) / D(2.)
        u = (np.arange(size, dtype=D) - half) / s * a + ax          # [x]
        v = (np.arange(size, dtype=D) - half) / s + ay              # [y]
        rx = (cosr * u[None, :] - sinr * v[:, None] + D(cx)).astype(F)
        ry = (sinr * u[None, :] + cosr * v[:, None] + D(cy)).astype(F)
    return rx, ry


def taps(ow, oh, rx, ry):
    """bilinear_interpolate's integer part: (x0, x1, y0, y1) after get_pixel_extend's clamp, and the float weights' dx, dy"""
    fx, fy = np.floor(rx), np.floor(ry)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    dx = (rx - ix.astype(F)).astype(F)
    dy = (ry - iy.astype(F)).astype(F)
    return (np.clip(ix, 0, ow - 1), np.clip(ix + 1, 0, ow - 1), np.clip(iy, 0, oh - 1), np.clip(iy + 1, 0, oh - 1)), dx, dy


def rotate_crop(img, size, rad, scale, dx, dy, aspect):
    """rotate_crop_image on float32 [oh][ow][3] -> [size][size][3]"""
    oh, ow = img.shape[:2]
    rx, ry = coords(ow, oh, size, rad, scale, dx, dy, aspect)
    (x0, x1, y0, y1), fx, fy = taps(ow, oh, rx, ry)
    _1 = F(1)
    w00 = ((_1 - fy) * (_1 - fx)).astype(F)[..., None]
    w01 = (fy * (_1 - fx)).astype(F)[..., None]
    w10 = ((_1 - fy) * fx).astype(F)[..., None]
    w11 = (fy * fx).astype(F)[..., None]
    val = (w00 * img[y0, x0]).astype(F)
    val = (val + (w01 * img[y1, x0]).astype(F)).astype(F)
    val = (val + (w10 * img[y0, x1]).astype(F)).astype(F)
    val = (val + (w11 * img[y1, x1]).astype(F)).astype(F)
    return val


def augment(frame, size, rad, scale, dx, dy, aspect, flip, dhue, dsat, dexp, swap_rb=False):
    """one image of the loader -> float32 [size][size][3] (the trainer's NHWC input)"""
    crop = rotate_crop(planes(frame, swap_rb), size, rad, scale, dx, dy, aspect)
    if flip:
        crop = crop[:, ::-1]
    return distort(crop, dhue, dsat, dexp)
