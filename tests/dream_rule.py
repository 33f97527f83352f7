"""The reference's dream step, restated in numpy: optimize_picture (src_yolo2/nightmare.c:34-115), calculate_loss (:23-32)
and the round end of run_nightmare (:296-305).

The network part -- forward_network with train = 0, the thresholded copy, backward_network with a state.delta for layer 0
-- stands on tests/train_rule.py's Trainer (its convolution and maxpool, forward and backward, are the reference's) and is
held to the compiled reference by tests/golden/gen_dream_golden.py through tests/native/dream_ref.c.  The picture part --
crop_image, resize_image, flip_image, normalize_array, axpy_cpu, constrain_image, rotate_image -- has no compiled form
(image.c does not build without OpenCV), so it is stated here from the source, in float32 in the reference's operation
order (every product and sum rounded on its own, as -ffp-contract=off compiles them) plus the float64 twin T64, as the
classifier loader's pixel chain is in tests/aug_cls_rule.py.

    err(A) = max|A - T64| / max|T64|,       a GPU tensor passes when  err(gpu) <= 4 * err(reference) + 4 * 2^-23

(train_rule.err / train_rule.bound).  Where the reference sums n floats one after the other (mean_array, variance_array)
the float32 form does too (np.cumsum is sequential); the device sums by chunks and a tree, which is what the bound is for.

Kinks, asserted on the float64 run by the generator: no leaky / relu pre-activation within 1e-4 of zero, no two DIFFERENT
values within 1e-4 at the top of a maxpool window (exact ties come from repeated edge pixels: see SETTINGS), and no element
of the last layer within 1e-4 * max|output| of calculate_loss's threshold (`Net.min_margin`), so no comparison in the tests
is decided inside rounding error.
"""
import math

import numpy as np

from tests import train_rule as T

F = np.float32
KINK = T.KINK

_BASE = dict(batch=1, subdivisions=1, learning_rate=0.01, momentum=0.9, decay=0.0005, policy="constant")
NETS = {
    # both layer types, a maxpool as a possible last layer, a 1x1 layer, an odd-sized picture
    "D1": dict(_BASE, w=23, h=17, c=3,
               layers=[("conv", 8, 3, 1, 0, "leaky"), ("max", 2, 2), ("conv", 12, 3, 1, 0, "leaky"), ("max", 2, 2),
                       ("conv", 16, 1, 1, 0, "leaky")]),
    # vgg-shaped, relu
    "D2": dict(_BASE, w=40, h=28, c=3,
               layers=[("conv", 16, 3, 1, 0, "relu"), ("conv", 16, 3, 1, 0, "relu"), ("max", 2, 2), ("conv", 32, 3, 1, 0, "relu")]),
    # no padding anywhere: 5x5 logistic, 3x3 linear
    "D3": dict(_BASE, w=19, h=15, c=3,
               layers=[("conv", 6, 5, 0, 0, "logistic"), ("conv", 7, 3, 0, 0, "linear")]),
}


def scale_of(octave):
    """1/pow(1.33333333, octave) handed to a float parameter"""
    return float(F(1.0 / math.pow(1.33333333, octave)))


def size_of(w, h, scale):
    """(int)(orig.w * scale), (int)(orig.h * scale): int * float is a float product"""
    return int(F(w) * F(scale)), int(F(h) * F(scale))


# (max_layer, octave, dx, dy, flip, thresh, norm) per fixture; CHAIN = three steps in a row from one picture.
# A shifted crop repeats edge pixels over a band up to 8 wide.  At octave 0 the resize copies (dx = 0: 1*a + 0*b), the band
# stays constant, the convolution windows inside it are identical and a maxpool window over their outputs has an EXACT tie,
# which every form gives to the first element in scan order.  At a smaller octave the resize interpolates between equal
# values, (1-d)*a + d*a, which is a only up to rounding: the same windows now tie within an ulp and the winner is decided by
# rounding, in the reference as anywhere.  So below octave 0 a shifted crop is stored up to the first maxpool only, and the
# settings that cross a maxpool there use dx = dy = 0 (with and without the flip).
D1_DRAWS = ((-8, 7, 1), (7, -8, 0), (0, 0, 0))
SETTINGS = {
    "D1": [(0, 0, -8, 7, 1, 1.0, 1), (1, 0, 7, -8, 0, 1.0, 1), (2, 0, 0, 0, 0, 1.0, 0), (4, 0, -8, 7, 1, 0.0, 1),
           (4, 1, 0, 0, 0, 1.0, 1), (0, 1, 7, -8, 0, 0.0, 0), (2, 1, 0, 0, 1, 0.0, 0), (1, 3, 0, 0, 0, 1.0, 1),
           (0, 3, -8, 7, 1, 0.0, 1), (2, 3, 0, 0, 1, 1.0, 0)],
    "D2": [(3, 0, -8, 7, 1, 1.0, 1), (1, 1, 7, -8, 0, 0.0, 0)],
    "D3": [(1, 0, 7, -8, 0, 1.0, 1), (0, 0, -8, 7, 1, 0.0, 0)],
}
CHAIN = {"D1": [(4, 0, -8, 7, 1, 1.0, 1), (2, 1, 0, 0, 1, 1.0, 1), (4, 0, 7, -8, 0, 1.0, 1)]}
RATE = 0.04


# D2's 45000 relu pre-activations would put one within 1e-4 of zero for nearly every seed: its weights are the drawn ones
# times GAIN, which spreads the pre-activations out (the margin is absolute) and changes nothing else
GAIN = {"D1": 1.0, "D2": 4.0, "D3": 1.0}


def picture(name, seed):
    from sr_object_detection_amd import synth
    s = NETS[name]
    return synth.uniform(seed * 7907 + 17, s["c"] * s["h"] * s["w"], 0.05, 0.95).reshape(s["c"], s["h"], s["w"]).astype(F)


def materialize(tmp, name, seed):
    import os
    spec = NETS[name]
    cfg, wts = os.path.join(tmp, "dream_%s.cfg" % name), os.path.join(tmp, "dream_%s.weights" % name)
    with open(cfg, "w") as f:
        f.write(T.net_text(spec))
    params = T.initial_params(spec, seed)
    for p in params:
        if p is not None:
            p["weights"] = (p["weights"] * F(GAIN[name])).astype(F)
    T.write_weights(wts, params)
    return cfg, wts, params


# ---------------------------------------------------------------------------------------------------------------------
# the picture side; im is [c][h][w], dt is np.float32 (the reference's arithmetic) or np.float64 (T64)
# ---------------------------------------------------------------------------------------------------------------------
def crop_image(im, dx, dy, w, h):
    """image.c:1512: constrain_int repeats the edge pixels"""
    r = np.clip(np.arange(h) + dy, 0, im.shape[1] - 1)
    c = np.clip(np.arange(w) + dx, 0, im.shape[2] - 1)
    return im[:, r][:, :, c].copy()


def resize_image(im, w, h, dt=F):
    """image.c:1950: columns into `part`, then rows; (1-d)*a + d*b with every operation rounded"""
    im = np.asarray(im, dt)
    c, ih, iw = im.shape
    one = dt(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_scale = dt(iw - 1) / dt(w - 1)
        h_scale = dt(ih - 1) / dt(h - 1)
    part = np.zeros((c, ih, w), dt)
    part[:, :, w - 1] = im[:, :, iw - 1]
    if iw == 1:
        part[:] = im[:, :, iw - 1:iw]
    elif w > 1:
        sx = np.arange(w - 1).astype(dt) * w_scale
        ix = sx.astype(np.int64)
        dx = sx - ix.astype(dt)
        part[:, :, :w - 1] = (one - dx) * im[:, :, ix] + dx * im[:, :, ix + 1]
    out = np.zeros((c, h, w), dt)
    for r in range(h):
        sy = dt(r) * h_scale if h > 1 else dt(0)
        iy = int(sy)
        dy = sy - dt(iy)
        val = (one - dy) * part[:, iy, :]
        if not (r == h - 1 or ih == 1):
            val = val + dy * part[:, iy + 1, :]
        out[:, r, :] = val
    return out


def flip_image(im):
    return im[:, :, ::-1].copy()


def _seq_sum(a, dt):
    """sum_array: one float after the other"""
    return np.cumsum(np.asarray(a, dt).reshape(-1), dtype=dt)[-1] if dt == F else np.asarray(a, np.float64).sum()


def moments(a, dt=F):
    """mean_array and variance_array (utils.c:415-450): the variance about that mean, divided by n"""
    a = np.asarray(a, dt).reshape(-1)
    mean = dt(_seq_sum(a, dt) / dt(a.size))
    d = a - mean
    var = dt(_seq_sum(d * d, dt) / dt(a.size))
    return mean, var


def normalize_array(a, dt=F):
    """utils.c:482: (a - mu) / (float)sqrt(variance), no epsilon"""
    a = np.asarray(a, dt)
    mu, var = moments(a, dt)
    sigma = dt(np.sqrt(np.float64(var)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (a - mu) / sigma


def constrain_image(im):
    """image.c:1115: two tests a NaN passes"""
    im = np.where(im < 0, im.dtype.type(0), im)
    return np.where(im > 1, im.dtype.type(1), im)


def picture_to_input(pic, scale, dx, dy, flip, dt=F):
    """nightmare.c:44-46 -> [c][sh][sw]"""
    c, h, w = pic.shape
    sw, sh = size_of(w, h, scale)
    im = resize_image(crop_image(np.asarray(pic, dt), dx, dy, w, h), sw, sh, dt)
    return flip_image(im) if flip else im


def gradient_to_update(grad, w, h, dx, dy, flip, dt=F):
    """nightmare.c:81-84: the picture-sized `out` before normalisation"""
    g = np.asarray(grad, dt)
    if flip:
        g = flip_image(g)
    return crop_image(resize_image(g, w, h, dt), -dx, -dy, w, h)


def apply_update(pic, out, rate, norm, dt=F):
    """nightmare.c:94-107"""
    out = np.asarray(out, dt)
    if norm:
        out = normalize_array(out, dt)
    with np.errstate(invalid="ignore"):
        return constrain_image(np.asarray(pic, dt) + dt(F(rate)) * out)


def rotate_image(im, rad, dt=F):
    """image.c:1481 with bilinear_interpolate (:1935) and get_pixel_extend: cos / sin are libm's doubles of the float angle,
    the coordinates double expressions rounded to float"""
    im = np.asarray(im, dt)
    c, h, w = im.shape
    cs, sn = math.cos(float(F(rad))), math.sin(float(F(rad)))
    cx, cy = F(w / 2.), F(h / 2.)
    x = (np.arange(w).astype(F) - cx).astype(np.float64)[None, :]
    y = (np.arange(h).astype(F) - cy).astype(np.float64)[:, None]
    rx = cs * x - sn * y + np.float64(cx)
    ry = sn * x + cs * y + np.float64(cy)
    if dt == F:
        rx, ry = rx.astype(F), ry.astype(F)
    ix, iy = np.floor(rx).astype(np.int64), np.floor(ry).astype(np.int64)
    dx, dy = (rx - ix.astype(dt)).astype(dt), (ry - iy.astype(dt)).astype(dt)
    one = dt(1)

    def px(xx, yy):
        return im[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    return ((one - dy) * (one - dx) * px(ix, iy) + dy * (one - dx) * px(ix, iy + 1) + (one - dy) * dx * px(ix + 1, iy) +
            dy * dx * px(ix + 1, iy + 1))


def zoom_args(w, h, zoom):
    """nightmare.c:301: im.w * (1. - zoom)/2. is a double, im.w*zoom a float, both truncated by the int parameters"""
    z = float(F(zoom))
    return int(w * (1. - z) / 2.), int(h * (1. - z) / 2.), int(F(w) * F(zoom)), int(F(h) * F(zoom))


def round_end(pic, rotate, zoom, dt=F):
    """nightmare.c:296-305"""
    pic = np.asarray(pic, dt)
    c, h, w = pic.shape
    if rotate:
        pic = rotate_image(pic, rotate, dt)
    cx, cy, cw, ch = zoom_args(w, h, zoom)
    return resize_image(crop_image(pic, cx, cy, cw, ch), w, h, dt)


# ---------------------------------------------------------------------------------------------------------------------
# the network side
# ---------------------------------------------------------------------------------------------------------------------
def calculate_loss(output, thresh, dt=F):
    """nightmare.c:23-32 on the flattened [c][h][w] output -> (delta, selected count, mean, variance, smallest distance of an
    element from the threshold relative to max|output|)"""
    o = np.asarray(output, dt)
    mean, var = moments(o, dt)
    limit = np.float64(mean) + np.float64(F(thresh)) * np.sqrt(np.float64(var))
    keep = o.astype(np.float64) > limit
    margin = float(np.abs(o.astype(np.float64) - limit).min() / max(np.abs(o).max(), 1e-300))
    return np.where(keep, o, dt(0)), int(keep.sum()), mean, var, margin


class Net(T.Trainer):
    """forward / calculate_loss / backward of the network truncated behind max_layer, at any input size"""

    def __init__(self, spec, params, dtype=np.float64):
        super().__init__(spec, params, dtype)
        self.min_margin = np.inf
        self.exact_ties = 0

    def _max_forward(self, l, d, x):
        """train_rule's, with the gap taken over windows whose two largest values DIFFER: crop_image repeats edge pixels
        (constrain_int), so whole bands of the input are constant along a row or a column, the windows of a convolution
        inside such a band are identical and give identical outputs in every form, and a maxpool window over them has an
        exact tie that every form gives to the first element in scan order"""
        before, self.min_gap = self.min_gap, np.inf
        out = super()._max_forward(l, d, x)
        size, stride, P, xps, oh, ow, H, W = d["geom"]
        if size * size > 1:
            xp = np.full(xps, -T.FLT_MAX, self.dt)
            xp[:, :, P:P + H, P:P + W] = x
            wins = np.stack([xp[:, :, n + size:n + size + oh * stride:stride, m + size:m + size + ow * stride:stride]
                             for n in range(size) for m in range(size)])
            top = np.sort(wins, axis=0)
            gap = top[-1] - top[-2]
            self.exact_ties += int((gap == 0).sum())
            gap = gap[gap != 0]
            before = min(before, float(gap.min()) if gap.size else np.inf)
        self.min_gap = before
        return out

    def forward(self, x, max_layer, thresh):
        """x [c][h][w]: the forward pass and calculate_loss; every margin is known after it"""
        layers = self.spec["layers"]
        x = np.array(x, dtype=self.dt)[None]
        for i in range(max_layer + 1):
            l, d = layers[i], self.L[i]
            d["output"] = self._conv_forward(l, d, x) if l[0] == "conv" else self._max_forward(l, d, x)
            x = d["output"]
        last = self.L[max_layer]
        delta, self.selected, self.mean, self.var, margin = calculate_loss(last["output"], thresh, self.dt)
        last["delta"] = delta
        self.min_margin = min(self.min_margin, margin)

    def run(self, x, max_layer, thresh):
        """x [c][h][w] -> the image gradient [c][h][w]; self.L[i]["output"] / ["delta"] as backward_network leaves them"""
        layers = self.spec["layers"]
        self.forward(x, max_layer, thresh)
        img = {}
        for i in range(max_layer, -1, -1):
            l, d = layers[i], self.L[i]
            prev = self.L[i - 1] if i else img
            if l[0] == "conv":
                self._conv_backward(l, d, prev)
            else:
                size, stride, P, xps, oh, ow, H, W = d["geom"]
                dxp = np.zeros(xps, self.dt)
                k = 0
                for n in range(size):
                    for m in range(size):
                        r0, c0 = n + size, m + size
                        dxp[:, :, r0:r0 + oh * stride:stride, c0:c0 + ow * stride:stride] += d["delta"] * (d["arg"] == k)
                        k += 1
                prev["delta"] = dxp[:, :, P:P + H, P:P + W].copy()
        return img["delta"][0]


def step(net, pic, setting, rate=RATE):
    """one optimize_picture with given draws on `pic` [c][h][w] in net.dt -> dict: input, gradient, update (before
    normalisation), picture (after), l<i>_output / l<i>_delta, selected"""
    max_layer, octave, dx, dy, flip, thresh, norm = setting
    dt = net.dt
    c, h, w = pic.shape
    x = picture_to_input(pic, scale_of(octave), dx, dy, flip, dt)
    grad = net.run(x, max_layer, thresh)
    out = gradient_to_update(grad, w, h, dx, dy, flip, dt)
    res = {"input": x, "gradient": grad, "update": out, "picture": apply_update(pic, out, rate, norm, dt), "selected": net.selected}
    for i in range(max_layer + 1):
        res["l%d_output" % i] = net.L[i]["output"][0].copy()
        res["l%d_delta" % i] = net.L[i]["delta"][0].copy()
    return res


err = T.err
bound = T.bound
