"""The pixel chain of the reference's detection loader, restated in numpy: what load_data_detection (src_yolo2/data.c:676-705)
does to one image between load_image_color and d.X.vals[i] --

    (float)(v / 255.)   image.c:2045-2067       crop_image       image.c:1512-1532 (constrain_int taps: edge pixels repeat)
    resize_image        image.c:1950-1992       flip_image       image.c:1056-1070
    distort_image       image.c:1903-1916  =  rgb_to_hsv (:1718-1753), scale_image_channel twice, the hue shift with its two
                                              wraps, hsv_to_rgb (:1755-1794), constrain_image (:1115-1122)

Every operation is a float32 operation in the reference's order, float64 where the C promotes ((double)v / 255., h / 6.,
floor).  It is the yardstick of tests/test_gpu_aug.py, compared with np.array_equal: each value is formed by single IEEE
operations in a fixed order, so a tolerance would only hide a reordering.

PROVENANCE: parity with a run of the reference unpinned.  image.c of the reference does not compile without OpenCV and is
not in oracle/_ref/libdarknet_ref.so (oracle/build_ref.sh), so this chain is held to this restatement of the source, as the
ingest chain of tests/test_gpu_ingest.py is.  The draws and the truth of the loader ARE pinned to the compiled reference:
tests/golden/aug_truth.npz (tests/golden/gen_aug_golden.py).
"""
import numpy as np

F = np.float32
_1, _2, _4, _6 = F(1), F(2), F(4), F(6)


def planes(frame, swap_rb=False):
    """uint8 [h][w][c >= 3] -> float32 [h][w][3], channel k = byte k (2 - k with swap_rb)"""
    rgb = np.asarray(frame)[:, :, :3]
    if swap_rb:
        rgb = rgb[:, :, ::-1]
    return (rgb.astype(np.float64) / 255.).astype(F)


def crop(img, pleft, ptop, swidth, sheight):
    oh, ow = img.shape[:2]
    rows = np.clip(np.arange(sheight) + ptop, 0, oh - 1)
    cols = np.clip(np.arange(swidth) + pleft, 0, ow - 1)
    return img[rows][:, cols]


def resize(im, w, h):
    """resize_image on [ih][iw][3]"""
    ih, iw = im.shape[:2]
    with np.errstate(all="ignore"):
        w_scale = F(iw - 1) / F(w - 1)
        h_scale = F(ih - 1) / F(h - 1)
        c = np.arange(w)
        sx = c.astype(F) * w_scale
        ix = np.nan_to_num(sx, nan=0., posinf=0., neginf=0.).astype(np.int64)
        dx = (sx - ix.astype(F)).astype(F)
        last = (c == w - 1) | (iw == 1)
        i0 = np.where(last, iw - 1, np.minimum(ix, iw - 1))
        i1 = np.minimum(i0 + 1, iw - 1)
        blend = (_1 - dx)[None, :, None] * im[:, i0] + dx[None, :, None] * im[:, i1]
        part = np.where(last[None, :, None], im[:, i0], blend).astype(F)
        r = np.arange(h)
        sy = r.astype(F) * h_scale
        iy = np.nan_to_num(sy, nan=0., posinf=0., neginf=0.).astype(np.int64)
        dy = (sy - iy.astype(F)).astype(F)
        two = ~((r == h - 1) | (ih == 1))
        j0 = np.minimum(iy, ih - 1)
        j1 = np.minimum(j0 + 1, ih - 1)
        val = ((_1 - dy)[:, None, None] * part[j0]).astype(F)
        both = (val + dy[:, None, None] * part[j1]).astype(F)
    return np.where(two[:, None, None], both, val).astype(F)


def rgb_to_hsv(im):
    """rgb_to_hsv on [h][w][3] -> (h, s, v); a grey pixel's hue is the 0/0 the reference carries"""
    r, g, b = im[..., 0], im[..., 1], im[..., 2]
    mx = np.where(r > g, np.where(r > b, r, b), np.where(g > b, g, b))
    mn = np.where(r < g, np.where(r < b, r, b), np.where(g < b, g, b))
    delta = (mx - mn).astype(F)
    with np.errstate(all="ignore"):
        s = (delta / mx).astype(F)
        hh = np.where(r == mx, (g - b) / delta, np.where(g == mx, _2 + (b - r) / delta, _4 + (r - g) / delta)).astype(F)
        hh = np.where(hh < 0, hh + _6, hh).astype(F)
        hh = (hh.astype(np.float64) / 6.).astype(F)
    zero = mx == 0
    return np.where(zero, F(0), hh).astype(F), np.where(zero, F(0), s).astype(F), mx.astype(F)


def shift_hue(hh, dhue):
    """distort_image's hue loop: + dhue, then > 1 -> - 1, then < 0 -> + 1"""
    with np.errstate(all="ignore"):
        hh = (hh + F(dhue)).astype(F)
        hh = np.where(hh > 1, hh - _1, hh).astype(F)
        return np.where(hh < 0, hh + _1, hh).astype(F)


def distort(im, dhue, dsat, dexp):
    """distort_image on [h][w][3]"""
    dhue, dsat, dexp = F(dhue), F(dsat), F(dexp)
    hh, s, v = rgb_to_hsv(im)
    with np.errstate(all="ignore"):
        s = (s * dsat).astype(F)
        v = (v * dexp).astype(F)
        hh = shift_hue(hh, dhue)
        h6 = (_6 * hh).astype(F)
        index = np.floor(np.nan_to_num(h6.astype(np.float64), nan=0.)).astype(np.int64)
        f = (h6 - index.astype(F)).astype(F)
        p = (v * (_1 - s)).astype(F)
        q = (v * (_1 - s * f)).astype(F)
        t = (v * (_1 - s * (_1 - f))).astype(F)
    table = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v)}
    out = np.stack([v, p, q], axis=-1)                      # index 5, and 6 (h == 1) falling into it
    for k, rgb in table.items():
        out = np.where((index == k)[..., None], np.stack(rgb, axis=-1), out)
    out = np.where((s == 0)[..., None], np.stack([v, v, v], axis=-1), out).astype(F)
    out = np.where(out < 0, F(0), out)
    out = np.where(out > 1, F(1), out)
    return out.astype(F)


def augment(frame, pleft, ptop, swidth, sheight, flip, dhue, dsat, dexp, w, h, swap_rb=False):
    """one image of the loader -> float32 [h][w][3] (the trainer's NHWC input)"""
    sized = resize(crop(planes(frame, swap_rb), pleft, ptop, swidth, sheight), w, h)
    if flip:
        sized = sized[:, ::-1]
    return distort(sized, dhue, dsat, dexp)
