"""The half-storage rule: what a layer of a network run with set_half(True) may store, stated in numpy.

fp16 storage mode has no reference arithmetic (the reference has no half path), and two summation orders of real-valued
data legitimately differ, so the kernels cannot be pinned bit for bit.  The rule pins them as far as that allows, layer by
layer with teacher forcing:

  1. the layer's inputs are the producers' STORED activations (pull_layer_output): the exact half values the kernel read;
     for layer 0 the input is half(x) of the network input;
  2. the layer is computed in float64 from those inputs and the weights as the engine holds them: half(w), round to nearest
     even, for every layer with a half input (y2_half_weights) and for the first-layer kernels ((_Float16)w); alpha / beta
     evaluated in double and rounded to float32 as pack_dense does (host/y2_arena.c) -- the first-layer kernels fold on
     their own from the double reciprocal 1 / (sqrt(var) + 1e-6f), `first=True`; pre64 = acc64 * alpha + beta; the activation
     with float32 constants (the leaky slope is float32(0.1));
  3. the same in float32 (np.matmul on float32 for the products, one float32 operation per step after them) gives pre32, and
         delta = BOUND_FACTOR * max|pre32 - pre64| + BOUND_FLOOR * max|pre64|         (tests/train_rule.py)
     over the layer.  delta never comes from the device;
  4. with the activation monotone (linear, leaky, relu): lo = half(act(pre64 - delta)), hi = half(act(pre64 + delta)), and
     every stored element must satisfy lo <= got <= hi, infinities comparing as values.  A layer that stores fp32 (the conv
     in front of [region], the last [connected] of a head, avgpool) is held to |got - act(pre64)| <= delta instead.  With a
     fused 2x2 maxpool the convolution's output is never stored: the rule picks one accumulator per window by the sign of
     alpha as pool_pick does, and the comparison is made on the maxpool layer's output;
  5. pure selection layers (unfused maxpool, route, reorg, dropout at inference) must EQUAL the same selection applied to
     the pulled inputs.

Elements with |act(pre64)| < 2^-13 (the half subnormals and the binade above them) are exempt from containment and must
satisfy |got| <= 2^-13; their share must stay under 1 %.  A layer is only accepted as checked when at least 3/4 of its
elements have lo == hi: most of the tensor is then still pinned to a single half.

Left out on purpose: logistic (its device form uses __expf, whose error bound is not stated in this tree; such layers are
skipped and the skip is printed by name), [normalization] and [activation] (tests/test_gpu_lrn_kernels.py and
tests/test_gpu_activations.py keep the tests they have), and the head layers that run in fp32 behind an fp32 tensor
([region], [softmax], [detection], [cost]).

`RuleNet` is the rule's own float32 evaluation behind the two calls check_network makes (layer_kernel, pull_layer_output):
tests/test_half_rule_host.py runs every case of the GPU table through it, and through its eight wrong variants (MUTATIONS),
on the CPU.  The cases of tests/test_gpu_half_values.py are data in this file (CASES) for that reason."""
from __future__ import annotations

import math
import os
import struct
from typing import NamedTuple

import numpy as np

from sr_object_detection_amd import synth, zoo
from tests.train_rule import BOUND_FACTOR, BOUND_FLOOR

F, D, H = np.float32, np.float64, np.float16
TINY = 2.0 ** -13
PINNED_MIN = 0.75
TINY_MAX = 0.01
SLOPE = F(0.1)
HEADS = ("region", "softmax", "detection", "cost")


def half(a) -> np.ndarray:
    """round to nearest even to IEEE half (f32_to_f16_rne, v_cvt_f16_f32); values past 65504 + half an ulp give infinity"""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(H)


def fold(p, first: bool = False):
    """alpha, beta (float32) of y = act(acc * alpha + beta): pack_dense's formula, or with first=True the first-layer
    kernels' own (scale times the double reciprocal the arena holds as rinv)"""
    bias = np.asarray(p["bias"], F).astype(D)
    if "scale" not in p:
        return np.ones(bias.shape, F), bias.astype(F)
    den = np.sqrt(np.asarray(p["var"], F).astype(D)) + D(F(.000001))
    scale = np.asarray(p["scale"], F).astype(D)
    a = scale * (1.0 / den) if first else scale / den
    return a.astype(F), (bias - np.asarray(p["mean"], F).astype(D) * a).astype(F)


def activate(v, act: str) -> np.ndarray:
    """in v's own type, constants float32"""
    if act == "leaky":
        return np.where(v > 0, v, v * v.dtype.type(SLOPE))
    if act == "relu":
        return np.where(v > 0, v, v.dtype.type(0))
    if act == "linear":
        return v
    raise ValueError("no monotone rule for activation %r" % act)


# ---- the accumulators: x [b][c][h][w] or [b][inputs], returned [b][n][oh][ow] or [b][n] ---------------------------
def conv_acc(x, w, size: int, stride: int, pad: int, dt, chunk=None) -> np.ndarray:
    """w [n][c*size*size] in the reference's (c, kh, kw) order; one matmul per tap, the taps added in scan order.
    chunk: a function applied to the running sum after every tap (the wrong variants)"""
    x = np.asarray(x, dt)
    b, c, h, wd = x.shape
    n = w.shape[0]
    w = np.asarray(w, dt).reshape(n, c, size, size)
    oh, ow = (h + 2 * pad - size) // stride + 1, (wd + 2 * pad - size) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    acc = np.zeros((b, n, oh * ow), dt)
    for kh in range(size):
        for kw in range(size):
            xs = xp[:, :, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride].reshape(b, c, oh * ow)
            acc = acc + np.matmul(np.ascontiguousarray(w[:, :, kh, kw]), xs)
            if chunk is not None:
                acc = chunk(acc)
    return acc.reshape(b, n, oh, ow)


def connected_acc(x, w, dt) -> np.ndarray:
    """x [b][...] flattened in the reference's NCHW order, w [outputs][inputs]"""
    x = np.asarray(x, dt).reshape(x.shape[0], -1)
    return np.matmul(x, np.ascontiguousarray(np.asarray(w, dt).T))


def local_acc(x, w, size: int, stride: int, pad: int, dt) -> np.ndarray:
    """w [loc][n][c][kh][kw]; a matmul over the channels per location and tap"""
    x = np.asarray(x, dt)
    b, c, h, wd = x.shape
    oh, ow = (h + 2 * pad - size) // stride + 1, (wd + 2 * pad - size) // stride + 1
    w = np.asarray(w, dt).reshape(oh * ow, -1, c, size, size)
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    acc = np.zeros((b, oh * ow, w.shape[1], 1), dt)
    for kh in range(size):
        for kw in range(size):
            xs = xp[:, :, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride].reshape(b, c, oh * ow)
            acc = acc + np.matmul(np.ascontiguousarray(w[None, :, :, :, kh, kw]), np.transpose(xs, (0, 2, 1))[:, :, :, None])
    return np.transpose(acc[..., 0], (0, 2, 1)).reshape(b, -1, oh, ow)


def avgpool(x, dt) -> np.ndarray:
    """avgpool_layer.c:40-54: a sum in pixel order (cumsum adds one value at a time), one divide"""
    x = np.asarray(x, dt)
    b, c = x.shape[:2]
    hw = x.shape[2] * x.shape[3]
    return np.cumsum(x.reshape(b, c, hw), axis=2, dtype=dt)[:, :, -1] / dt(hw)


def _chan(v, ndim: int, dt) -> np.ndarray:
    return np.asarray(v, F).astype(dt).reshape((1, -1) + (1,) * (ndim - 2))


def pool_pick(acc, alpha) -> np.ndarray:
    """one accumulator per 2x2/2 window: the largest where the epilogue increases (alpha >= 0), else the smallest"""
    b, n, h, w = acc.shape
    win = acc[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, n, h // 2, 2, w // 2, 2)
    return np.where(_chan(alpha, 4, acc.dtype) >= 0, win.max(axis=(3, 5)), win.min(axis=(3, 5)))


def preact(acc, alpha, beta, dt) -> np.ndarray:
    """acc * alpha + beta in dt: two float32 operations in the float32 evaluation (the device's fmaf rounds once)"""
    return (acc * _chan(alpha, acc.ndim, dt)).astype(dt) + _chan(beta, acc.ndim, dt)


# ---- the selection layers -----------------------------------------------------------------------------------------
def maxpool(x, size: int, stride: int, pad: int) -> np.ndarray:
    """maxpool_layer.c:79-114: windows start at o * stride - pad, taps outside the image do not count"""
    b, c, h, w = x.shape
    oh, ow = (h + 2 * pad) // stride, (w + 2 * pad) // stride
    big = np.full((b, c, pad + oh * stride + size, pad + ow * stride + size), -np.inf, x.dtype)
    big[:, :, pad:pad + h, pad:pad + w] = x
    out = np.full((b, c, oh, ow), -np.inf, x.dtype)
    for n in range(size):
        for m in range(size):
            out = np.maximum(out, big[:, :, n:n + oh * stride:stride, m:m + ow * stride:stride])
    return out


def reorg(x, s: int) -> np.ndarray:
    """blas.c:8-29 with forward = 0, the reference's out_c = c / (s*s) quirk included: [b][c][h][w] -> [b][c*s*s][h/s][w/s]"""
    b, c, h, w = x.shape
    oc = c // (s * s)
    k, j, i = np.meshgrid(np.arange(c), np.arange(h), np.arange(w), indexing="ij")
    c2, off = k % oc, k // oc
    src = ((i * s + off % s) + w * s * ((j * s + off // s) + h * s * c2)).reshape(-1)
    return x.reshape(b, -1)[:, src].reshape(b, c * s * s, h // s, w // s)


# ---- intervals ----------------------------------------------------------------------------------------------------
def delta_of(pre32, pre64) -> float:
    return float(BOUND_FACTOR * np.abs(pre32.astype(D) - pre64).max() + BOUND_FLOOR * np.abs(pre64).max())


def interval(pre64, delta: float, act: str):
    """lo, hi as half arrays"""
    return half(activate(pre64 - delta, act)), half(activate(pre64 + delta, act))


# ---- the driver ---------------------------------------------------------------------------------------------------
class Row(NamedTuple):
    layer: int
    kernel: str
    what: str                 # "half", "f32", "select" or "skipped: ..."
    n: int
    pinned: float             # share with lo == hi
    equal: float              # share equal to half(act(pre64)) (f32 layers: to float32(act(pre64)))
    worst: float              # half layers: worst distance from half(act(pre64)) in half ulps; f32 layers: in units of delta
    tiny: float               # share in the exempt range
    outside: np.ndarray       # flat indices of the elements that break the rule

    def text(self) -> str:
        return "layer %2d %-44s %-7s n=%-8d pinned %.4f equal %.4f worst %.2f tiny %.5f outside %d" % (
            self.layer, self.kernel, self.what, self.n, self.pinned, self.equal, self.worst, self.tiny, len(self.outside))

    def failures(self):
        out = []
        if len(self.outside):
            out.append("layer %d (%s): %d of %d elements outside, first at %s" % (self.layer, self.kernel, len(self.outside), self.n,
                                                                                self.outside[:5].tolist()))
        if self.what == "half" and not self.pinned >= PINNED_MIN:
            out.append("layer %d (%s): only %.4f of the elements are pinned to one half" % (self.layer, self.kernel, self.pinned))
        if self.what in ("half", "f32") and not self.tiny < TINY_MAX:
            out.append("layer %d (%s): %.4f of the elements are in the subnormal range" % (self.layer, self.kernel, self.tiny))
        return out


def stores_f32(params, i: int) -> bool:
    """plan_half (host/y2_plan.c) restated: which layers of a half network store fp32"""
    t = params[i]["type"]
    nx = i + 1
    if t == "convolutional":
        return nx < len(params) and params[nx]["type"] == "region"
    if t == "connected":
        while nx < len(params) and params[nx]["type"] in ("dropout", "cost"):
            nx += 1
        return not (nx < len(params) and params[nx]["type"] == "connected")
    return t == "avgpool"


def _shape(l, batch):
    if l["type"] in ("connected", "avgpool"):
        return (batch, l["out_c"])
    return (batch, l["out_c"], l["out_h"], l["out_w"])


def layer_pre(l, xin, dt, first: bool = False, pooled: bool = False, mut=None, full: bool = False):
    """the pre-activation of a weighted layer in dt from its input and its weights as the engine holds them: half(w), or
    with full=True the fp32 weights (a layer 0 outside the fp16 first-layer kernels reads the fp32 input with fp32 weights
    and only stores half).  first: the fp16 first-layer kernels' own fold.  pooled: one accumulator per 2x2 window first.
    mut: one of MUTATIONS (the rule's float32 stand-in only)"""
    w = np.asarray(l["w"], F) if full else half(l["w"])
    if mut == "truncated weights":
        w = trunc_half(l["w"])
    w = w.astype(dt)
    if mut == "one K term dropped":
        w = w.copy()
        w.reshape(w.shape[0], -1)[:, -1] = 0
    alpha, beta = fold(l, first)
    if mut == "alpha off by 1e-5 relative":
        alpha = (alpha * F(1 + 1e-5)).astype(F)
    t = l["type"]
    if t == "convolutional":
        chunk = (lambda a: half(a).astype(dt)) if mut == "accumulator through half" else None
        acc = conv_acc(xin, w, l["size"], l["stride"], l["pad"], dt, chunk)
    elif t == "connected":
        acc = connected_acc(xin, w, dt)
    elif t == "local":
        acc = local_acc(xin, w, l["size"], l["stride"], l["pad"], dt)
        alpha, beta = np.ones(acc.shape[1:], F), np.asarray(l["bias"], F).reshape(acc.shape[1:])
        return (acc * alpha[None].astype(dt)).astype(dt) + beta[None].astype(dt)
    else:
        raise ValueError(t)
    if pooled:
        acc = pool_pick(acc, alpha)
    if mut == "bias after the rounding":
        return half((acc * _chan(alpha, acc.ndim, dt)).astype(dt)).astype(dt) + _chan(beta, acc.ndim, dt)
    return preact(acc, alpha, beta, dt)


def _measure(i, kernel, got, pre64, delta: float, act, f32_out) -> Row:
    got = np.asarray(got, F).reshape(pre64.shape)
    want64 = activate(pre64, act)
    tiny = np.abs(want64) < TINY
    if f32_out:
        d = np.abs(got.astype(D) - want64)
        return Row(i, kernel, "f32", got.size, float("nan"), float((got == want64.astype(F)).mean()), float(d.max() / delta),
                   float(tiny.mean()), np.flatnonzero(~(d <= delta)))
    lo, hi = interval(pre64, delta, act)
    centre = half(want64)
    bad = np.where(tiny, ~(np.abs(got) <= TINY), ~((lo <= got) & (got <= hi)))
    fin = np.isfinite(centre) & np.isfinite(got)
    ulp = np.spacing(np.abs(np.where(fin, centre, H(1)))).astype(D)
    dist = np.where(fin, np.abs(got.astype(D) - np.where(fin, centre, H(0)).astype(D)) / ulp, np.where(got == centre, 0.0, np.inf))
    return Row(i, kernel, "half", got.size, float((lo == hi).mean()), float((got == centre).mean()), float(dist.max()), float(tiny.mean()),
               np.flatnonzero(bad))


def _select(i, kernel, got, want) -> Row:
    got = np.asarray(got, F).reshape(want.shape)
    bad = np.flatnonzero(~(got == want))
    return Row(i, kernel, "select", got.size, 1.0, float((got == want).mean()), 0.0 if not len(bad) else float("inf"), 0.0, bad)


def check_network(net, x, params, echo=print):
    """walk the layers of `net` (layer_kernel, pull_layer_output; a convolution whose kernel name carries "+maxpool2" is
    fused and checked on the maxpool layer behind it) and hold each to the rule.  params: per layer the dict of zoo.resolve
    with the layer's arrays (attach).  Every row is printed before anything is asserted; the caller asserts
    `not failures(rows)`."""
    batch = x.shape[0]
    rows = []
    pulled = {}

    # layer 0: the fp16 first-layer kernels read half(x) with half(w) and fold on their own; any other kernel there (the fp32
    # first-layer kernels where the fp16 ones refuse the shape, the direct kernel) reads x with the fp32 weights
    f16_first = "_f16" in net.layer_kernel(0)

    def how(j):
        return dict(first=j == 0 and f16_first, full=j == 0 and not f16_first)

    def out(j):
        if j < 0:
            return half(x).astype(F) if f16_first else np.asarray(x, F)
        if j not in pulled:
            pulled[j] = np.asarray(net.pull_layer_output(j), F).reshape(_shape(params[j], batch))
        return pulled[j]

    def emit(r):
        rows.append(r)
        echo(r.text())

    def skip(i, kernel, why):
        emit(Row(i, kernel, "skipped: " + why, 0, float("nan"), float("nan"), float("nan"), 0.0, np.zeros(0, np.int64)))

    fused_from = None
    for i, l in enumerate(params):
        t, kernel = l["type"], net.layer_kernel(i)
        if t in ("convolutional", "connected", "local"):
            if l["activation"] == "logistic":
                skip(i, kernel, "logistic")
                continue
            if "+maxpool2" in kernel:
                fused_from = i
                continue
            xin = out(i - 1)
            pre64, pre32 = layer_pre(l, xin, D, **how(i)), layer_pre(l, xin, F, **how(i))
            emit(_measure(i, kernel, out(i), pre64, delta_of(pre32, pre64), l["activation"], stores_f32(params, i)))
        elif t == "maxpool" and fused_from == i - 1:
            c = params[i - 1]
            assert (l["size"], l["stride"], l["pad"]) == (2, 2, 0), l
            xin = out(i - 2)
            # delta over the full-resolution layer (max over a window moves a value by no more than its inputs move)
            delta = delta_of(layer_pre(c, xin, F, **how(i - 1)), layer_pre(c, xin, D, **how(i - 1)))
            emit(_measure(i, net.layer_kernel(i - 1), out(i), layer_pre(c, xin, D, pooled=True, **how(i - 1)), delta, c["activation"], False))
            fused_from = None
        elif t == "maxpool":
            emit(_select(i, kernel, out(i), maxpool(out(i - 1), l["size"], l["stride"], l["pad"])))
        elif t == "route":
            emit(_select(i, kernel, out(i), np.concatenate([out(j) for j in l["layers"]], axis=1)))
        elif t == "reorg":
            emit(_select(i, kernel, out(i), reorg(out(i - 1), l["stride"])))
        elif t == "dropout":
            emit(_select(i, kernel, out(i), out(i - 1).reshape(_shape(l, batch))))
        elif t == "avgpool":
            xin = out(i - 1)
            pre64 = avgpool(xin, D)
            emit(_measure(i, kernel, out(i), pre64, delta_of(avgpool(xin, F), pre64), "linear", True))
        else:
            skip(i, kernel, t if t in HEADS else "no rule for [%s]" % t)
    return rows


def failures(rows):
    return [f for r in rows for f in r.failures()]


# ---- the rule's float32 evaluation as a device ----------------------------------------------------------------------
MUTATIONS = ("truncating store", "truncated weights", "bias after the rounding", "accumulator through half", "slope in half",
             "alpha off by 1e-5 relative", "one K term dropped", "store rounded twice")


def trunc_half(v) -> np.ndarray:
    """float32 -> half toward zero"""
    v = np.asarray(v, F)
    h = half(v)
    over = np.abs(h.astype(F)) > np.abs(v)
    return np.where(over, np.nextafter(h, H(0)), h)


def round_bits13(v) -> np.ndarray:
    """float32 rounded to nearest even at 13 significant bits: the first of two roundings"""
    u = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x3FF) + ((u >> np.uint64(11)) & np.uint64(1))) & np.uint64(0xFFFFF800)
    return u.astype(np.uint32).view(F)


class RuleNet:
    """the rule's float32 evaluation run free (every layer reads what the layer before it stored) behind the interface
    check_network uses.  fuse: a convolution in front of a 2x2/2 maxpool is fused with it.  mutate = (layer, name): that
    layer is computed by one of the wrong variants"""

    def __init__(self, params, x, fuse: bool = True, mutate=None):
        self.params, self.n = params, len(params)
        self.store, self.kernels = {}, []
        batch = x.shape[0]
        # layer 0 as the engine dispatches it: the fp16 first-layer kernels take 3x3 convolutions of at most 64 filters on
        # an image whose width is a multiple of 4; anything else there is an fp32 kernel that stores half
        l0 = params[0]
        self.f16_first = (l0["type"] == "convolutional" and (l0["size"], l0["stride"], l0["pad"]) == (3, 1, 1) and l0["filters"] <= 64 and
                          l0["w"].shape[1] == 27 and x.shape[3] % 4 == 0)
        cur = half(x).astype(F) if self.f16_first else np.asarray(x, F)
        skip_pool = False
        routed = {j for l in params if l["type"] == "route" for j in l["layers"]}       # a layer a [route] reads is stored
        for i, l in enumerate(params):
            t = l["type"]
            name = ("rule_conv_first_f16" if self.f16_first else "rule_conv_f32") if i == 0 else "rule_" + t
            mut = mutate[1] if mutate and mutate[0] == i else None
            if t in ("convolutional", "connected", "local"):
                nxt = params[i + 1] if i + 1 < len(params) else None
                pooled = bool(fuse and i not in routed and t == "convolutional" and nxt and nxt["type"] == "maxpool" and
                              (nxt["size"], nxt["stride"], nxt["pad"]) == (2, 2, 0) and l["out_h"] % 2 == 0 and l["out_w"] % 2 == 0)
                pre = layer_pre(l, cur, F, first=i == 0 and self.f16_first, pooled=pooled, mut=mut, full=i == 0 and not self.f16_first)
                act = l["activation"]
                if mut == "slope in half" and act == "leaky":
                    v = np.where(pre > 0, pre, (pre * half(SLOPE).astype(F)).astype(F))
                else:
                    v = activate(pre, act).astype(F)
                if stores_f32(params, i):
                    cur = v
                elif mut == "truncating store":
                    cur = trunc_half(v).astype(F)
                elif mut == "store rounded twice":
                    cur = half(round_bits13(v)).astype(F)
                else:
                    cur = half(v).astype(F)
                if pooled:
                    name += "+maxpool2"
                    skip_pool = True
                    self.store[i + 1] = cur
                else:
                    self.store[i] = cur
            elif t == "maxpool":
                if skip_pool:
                    skip_pool = False
                else:
                    cur = maxpool(cur, l["size"], l["stride"], l["pad"])
                    self.store[i] = cur
            elif t == "route":
                cur = np.concatenate([self.store[j] for j in l["layers"]], axis=1)
                self.store[i] = cur
            elif t == "reorg":
                cur = reorg(cur, l["stride"])
                self.store[i] = cur
            elif t == "avgpool":
                cur = avgpool(cur, F)
                self.store[i] = cur
            elif t == "dropout":
                cur = cur.reshape(_shape(l, batch))
                self.store[i] = cur
            else:
                self.store[i] = cur
            self.kernels.append(name)

    def layer_kernel(self, i: int) -> str:
        return self.kernels[i]

    def pull_layer_output(self, i: int) -> np.ndarray:
        if i not in self.store:
            raise RuntimeError("layer %d is fused with the maxpool behind it" % i)
        return self.store[i].reshape(-1)


# ---- real-valued cases ----------------------------------------------------------------------------------------------
def normals(seed: int, n: int) -> np.ndarray:
    """standard normals by Box-Muller from the splitmix64 uniforms"""
    u1 = synth.uniform01(seed, n).astype(D) + 2.0 ** -25
    u2 = synth.uniform01(seed + 0x5bd1e995, n).astype(D)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def real_input(seed: int, shape) -> np.ndarray:
    """a mix of unit-scale and 0.1-scale normals"""
    n = int(np.prod(shape))
    return (normals(seed, n) * np.where(synth.uniform01(seed + 77, n) < 0.5, 1.0, 0.1)).astype(F).reshape(shape)


def _bn(s: int, n: int) -> dict:
    scale = synth.uniform(s + 2, n, 0.5, 1.5)
    scale[2::3] *= F(-1)
    return dict(scale=scale, mean=synth.uniform(s + 3, n, -0.5, 0.5), var=synth.uniform(s + 4, n, 0.5, 1.5))


def real_weights(seed: int, n: int, K: int) -> np.ndarray:
    """uniform with variance 1/K; |w| < 2^-13 becomes +-2^-13, so that no half weight is subnormal"""
    a = math.sqrt(3.0 / K)
    w = synth.uniform(seed, n * K, -a, a)
    small = np.abs(w) < TINY
    w[small] = np.where(np.signbit(w[small]), F(-TINY), F(TINY))
    assert np.abs(half(w).astype(F)).min() >= 2.0 ** -14
    return w.reshape(n, K)


def real_arrays(layers, seed: int) -> dict:
    """by layer index: bias / scale / mean / var / w, in the shapes of tests/layer_rule.py read_weights"""
    out = {}
    for i, l in enumerate(layers):
        s = seed * 1000003 + i * 7919
        t = l["type"]
        if t == "convolutional":
            n, K = l["filters"], l["c"] * l["size"] ** 2
            p = dict(bias=synth.uniform(s + 1, n, -0.5, 0.5), w=real_weights(s + 5, n, K))
        elif t == "connected":
            n = l["outputs"]
            p = dict(bias=synth.uniform(s + 1, n, -0.5, 0.5), w=real_weights(s + 5, n, l["inputs"]))
        elif t == "local":
            loc, n, K = l["out_w"] * l["out_h"], l["filters"], l["c"] * l["size"] ** 2
            p = dict(bias=synth.uniform(s + 1, n * loc, -0.5, 0.5).reshape(n, loc),
                     w=real_weights(s + 5, loc * n, K).reshape(loc, n, l["c"], l["size"], l["size"]))
            out[i] = p
            continue
        else:
            continue
        if l.get("batch_normalize"):
            p.update(_bn(s, n))
        out[i] = p
    return out


def write_weights(path: str, layers, arrays) -> None:
    """the record order of synth.write_weights: conv biases, (scales, mean, variance), weights; connected biases, weights,
    (scales, mean, variance); local biases, weights"""
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", 0, 1, 0, 0))
        for i, l in enumerate(layers):
            p = arrays.get(i)
            if p is None:
                continue
            bn = [np.asarray(p[k], F).tobytes() for k in ("scale", "mean", "var")] if "scale" in p else []
            f.write(np.asarray(p["bias"], F).tobytes())
            if l["type"] == "convolutional":
                f.write(b"".join(bn))
            f.write(np.asarray(p["w"], F).tobytes())
            if l["type"] == "connected":
                f.write(b"".join(bn))


def attach(layers, arrays):
    return [dict(l, **arrays.get(i, {})) for i, l in enumerate(layers)]


# edits of a case's arrays: the edges.  layer = the layer under test
def _edit_zero_scale(p):
    p["scale"][5] = 0                         # the output is half(beta) everywhere


def _edit_negative_alpha(p):
    p["scale"][:] = -np.abs(p["scale"])


def _edit_overflow(p):
    """every alpha large enough that delta (which grows with max|pre64|) stays far below the half spacing of most outputs,
    and filter 3 six times larger still: its outputs pass 65504 and must be stored as infinities"""
    p["scale"] *= F(16000.0)
    p["scale"][3] *= F(6.0)


EDITS = {"zero_scale": _edit_zero_scale, "negative_alpha": _edit_negative_alpha, "overflow": _edit_overflow}


class Case(NamedTuple):
    ident: str
    spec: tuple
    size: int
    batch: int
    seed: int
    env: tuple = ()               # ((name, value), ...)
    kernels: tuple = ()           # ((layer, name, exact), ...): exact False = a prefix
    counter: str = ""             # a launch counter of the library that must move
    fuse: bool = True
    edit: tuple = ()              # (layer, name of EDITS)
    zoo_net: str = ""             # a zoo network with synth.write_weights' parameters instead of spec

    def net_key(self):
        return (self.spec, self.size, self.batch, self.seed, self.fuse, self.edit, self.zoo_net)


def build_case(c: Case):
    """(cfg text, layers, arrays, x) of a case with its own parameters"""
    spec = [(e[0], dict(e[1])) if e[0] == "detection" else e for e in c.spec]
    layers = zoo.resolve(spec, c.size)
    arrays = real_arrays(layers, c.seed)
    if c.edit:
        EDITS[c.edit[1]](arrays[c.edit[0]])
    x = real_input(c.seed * 31 + 7, (c.batch, 3, c.size, c.size))
    return zoo.cfg_text("x", c.size, c.size, c.batch, spec=spec), layers, arrays, x


def materialize(workdir: str, c: Case):
    """cfg and .weights on disk; returns (cfg, weights, x, params)"""
    text, layers, arrays, x = build_case(c)
    stem = os.path.join(workdir, "halfrule_%s" % c.ident.replace("/", "_"))
    with open(stem + ".cfg", "w") as f:
        f.write(text)
    write_weights(stem + ".weights", layers, arrays)
    return stem + ".cfg", stem + ".weights", x, attach(layers, arrays)


# ---- the table of tests/test_gpu_half_values.py -----------------------------------------------------------------------
SWITCHES = ("Y2_CONV_TILE", "Y2_CONV_GRID", "Y2_CONV_KSPLIT", "Y2_NO_M16", "Y2_F16_NO_P8", "Y2_SK", "Y2_SK_TILES", "Y2_SK_WGS", "Y2_TAIL_TILES",
            "Y2_TAIL_TILE", "Y2_C64_MIN_TILES", "Y2_NO_C64", "Y2_NO_FIRST_NCHW", "Y2_CONN_KSPLIT", "Y2_CONN_F16", "Y2_AVGPOOL_SCALAR",
            "Y2_XCD_ORDER", "Y2_NO_FUSE")
# tests/test_gpu_tiles.py: (BM, BN, m16) of g_variants_h, and (tail tiles cut along K, workgroups, persistent grid)
F16_TILES = ((256, 256, True), (256, 256, False), (256, 128, False), (256, 64, False), (128, 128, False), (128, 64, False), (64, 64, False))
SK_CASES = ((5, 7, 7), (3, 3, 5), (12, 13, 13), (2, 7, 7), (7, 7, 7))
DET5_COPY = ("detection", (("classes", 5), ("num", 2), ("side", 4), ("softmax", 0), ("sqrt", 1)))


def _two(cin, filters, ksize, pool, act="leaky", bn=1, stride=1):
    under = ("conv", filters, ksize, bn, act) if stride == 1 else ("conv", filters, ksize, bn, act, stride)
    return (("conv", cin, 3, 1, "leaky"), under) + ((("max", 2, 2),) if pool else ())


def _pool_name(pool):
    return "+maxpool2" if pool else ""


def _tile_env(bm, bn, grid=3, **more):
    return (("Y2_CONV_TILE", "%dx%d" % (bm, bn)), ("Y2_CONV_GRID", str(grid))) + tuple(sorted(more.items()))


def cases():
    out = []
    # conv_mfma_f16 tiles (the LDS-DMA kernel conv_p8_f16 at 256x256 m16, BK 64): both K depths, 1x1 and 3x3, pool
    for bm, bn, m16 in F16_TILES:
        for bk, cin in ((64, 64), (32, 96)):
            for ks in (1, 3):
                for pool in (False, True):
                    env = _tile_env(bm, bn) if m16 else _tile_env(bm, bn, Y2_NO_M16="1")
                    name = "conv_mfma_f16_%dx%dx%d_k%d%s" % (bm, bn, bk, ks, _pool_name(pool))
                    out.append(Case("tile-%dx%d%s-bk%d-k%d%s" % (bm, bn, "m16" if m16 else "", bk, ks, "-pool" if pool else ""),
                                    _two(cin, bn + 40, ks, pool), 26, 2, 100 + bn + cin + ks, env, ((1, name, True),)))
    # a filter count that is no multiple of 8: the 2-byte store epilogue
    for bm, bn, m16 in F16_TILES:
        if m16:
            continue
        for pool in (False, True):
            out.append(Case("scalar-store-%dx%d%s" % (bm, bn, "-pool" if pool else ""), _two(64, bn + 37, 3, pool), 26, 2, 200 + bn,
                            _tile_env(bm, bn, Y2_NO_M16="1"), ((1, "conv_mfma_f16_%dx%dx64_k3%s" % (bm, bn, _pool_name(pool)), True),)))
    # the register-staged 16x16x32 form of the 256x256 tile
    for bk, cin in ((64, 64), (32, 96)):
        for ks in (1, 3):
            for pool in (False, True):
                out.append(Case("regstaged-m16-bk%d-k%d%s" % (bk, ks, "-pool" if pool else ""), _two(cin, 296, ks, pool), 26, 2, 100 + 256 + cin + ks,
                                _tile_env(256, 256, Y2_F16_NO_P8="1"),
                                ((1, "conv_mfma_f16_256x256x%d_k%d%s" % (bk, ks, _pool_name(pool)), True),)))
    # conv_p8_f16: whole tiles, stream-K with its fix-up launch, the small-tile tail
    for ks, cin in ((3, 128), (1, 64)):
        for pool in (False, True):
            spec, seed = _two(cin, 296, ks, pool), 300 + cin + ks
            name = ((1, "conv_mfma_f16_256x256x64_k%d%s" % (ks, _pool_name(pool)), True),)
            tag = "k%d-c%d%s" % (ks, cin, "-pool" if pool else "")
            out.append(Case("p8-whole-" + tag, spec, 26, 2, seed, _tile_env(256, 256, 7, Y2_SK="0"), name))
            for tiles, wgs, grid in (SK_CASES[0], SK_CASES[2]):
                out.append(Case("p8-sk%d-wg%d-%s" % (tiles, wgs, tag), spec, 26, 2, seed,
                                _tile_env(256, 256, grid, Y2_SK_TILES=str(tiles), Y2_SK_WGS=str(wgs)), name, "y2h_stream_k_launches"))
    for ntail in (5, 12):
        for tile in ((128, 64), (64, 64)):
            for pool in (False, True):
                out.append(Case("p8-tail%d-%dx%d%s" % (ntail, tile[0], tile[1], "-pool" if pool else ""), _two(128, 296, 3, pool), 26, 2, 300 + 128 + 3,
                                _tile_env(256, 256, 4, Y2_TAIL_TILES=str(ntail), Y2_TAIL_TILE="%dx%d" % tile),
                                ((1, "conv_mfma_f16_256x256x64_k3%s" % _pool_name(pool), True),), "y2h_tail_launches"))
    # the weights-stationary kernels
    for filters in (64, 48, 24):
        for fuse in (True, False):
            out.append(Case("c32-n%d-%s" % (filters, "fused" if fuse else "unfused"), _two(32, filters, 3, True), 32, 2, 400 + filters, (),
                            ((1, "conv_c32_f16_16x16" + _pool_name(fuse), True),), fuse=fuse))
    for filters in (128, 96, 72):
        for pool in (False, True):
            out.append(Case("c64-n%d%s" % (filters, "-pool" if pool else ""), _two(64, filters, 3, pool), 48, 2, 500 + filters,
                            (("Y2_C64_MIN_TILES", "1"), ("Y2_CONV_GRID", "4")), ((1, "conv_c64_f16_16x16" + _pool_name(pool), True),)))
    # the first layer: straight from the NCHW input, and behind the input transform
    for filters in (32, 24, 64):
        for size in (40, 20):
            for pool in (False, True):
                for direct in (True, False):
                    name = "conv_first_mfma_f16_%sc3_n%d%s" % ("nchw_" if direct else "", 32 if filters <= 32 else 64, _pool_name(pool))
                    out.append(Case("first-%s-n%d-%d%s" % ("nchw" if direct else "halo", filters, size, "-pool" if pool else ""),
                                    (("conv", filters, 3, 1, "leaky"),) + ((("max", 2, 2),) if pool else ()), size, 2, 600 + filters + size,
                                    () if direct else (("Y2_NO_FIRST_NCHW", "1"),), ((0, name, True),)))
    # conv_direct_f16 (three of tests/test_gpu_conv_forms.py DIRECT_F16_CASES): one strided, one 5x5, one with Cin = 16
    out.append(Case("direct-k3-s2-c32", _two(32, 40, 3, False, stride=2), 22, 2, 701, (), ((1, "conv_direct_f16", True),)))
    out.append(Case("direct-k5-c32", _two(32, 37, 5, False), 21, 2, 702, (), ((1, "conv_direct_f16", True),)))
    out.append(Case("direct-k3-c16", _two(16, 40, 3, False), 21, 2, 703, (), ((1, "conv_direct_f16", True),)))
    # dense heads: a half image into a dense layer (half out), dense into dense (half out), the last dense layer (fp32 out)
    for ksplit in (1, 3):
        for bn in (0, 1):
            if bn and ksplit == 1:
                continue
            spec = (("conv", 32, 3, 1, "leaky"), ("connected", 96, bn, "leaky"), ("dropout", 0.5), ("connected", 64, bn, "linear"),
                    ("connected", 240, 0, "linear"), DET5_COPY)
            sfx = "+ksplit%d" % ksplit if ksplit > 1 else ""
            # the 64-input last layer has two 32-steps: three ranges are clamped to two
            out.append(Case("connected-ksplit%d%s" % (ksplit, "-bn" if bn else ""), spec, 4, 5, 800 + bn, (("Y2_CONN_KSPLIT", str(ksplit)),),
                            ((1, "connected_f16" + sfx, True), (3, "connected_f16" + sfx, True), (4, "connected_f16", False))))
    out.append(Case("local", (("conv", 32, 3, 1, "leaky"), ("local", 24, 3, 1, 1, "leaky")), 8, 3, 810, (), ((1, "local_f16", True),)))
    for filters in (72, 36):
        for scalar in (False, True):
            out.append(Case("avgpool-n%d%s" % (filters, "-scalar" if scalar else ""),
                            (("conv", 16, 3, 1, "leaky"), ("conv", filters, 1, 1, "leaky"), ("avg",)), 14, 2, 820 + filters,
                            (("Y2_AVGPOOL_SCALAR", "1"),) if scalar else (), ((1, "conv_direct_f16", True), (2, "avgpool", True))))
    # edges
    for pool in (False, True):
        out.append(Case("edge-zero-scale%s" % ("-pool" if pool else ""), _two(64, 104, 3, pool), 26, 2, 900, _tile_env(64, 64, Y2_NO_M16="1"),
                        ((1, "conv_mfma_f16_64x64x64_k3" + _pool_name(pool), True),), edit=(1, "zero_scale")))
    out.append(Case("edge-negative-alpha-linear-pool", _two(64, 104, 3, True, act="linear"), 26, 2, 901, _tile_env(64, 64, Y2_NO_M16="1"),
                    ((1, "conv_mfma_f16_64x64x64_k3+maxpool2", True),), edit=(1, "negative_alpha")))
    out.append(Case("edge-overflow", _two(64, 104, 3, False, act="linear"), 26, 2, 902, _tile_env(64, 64, Y2_NO_M16="1"),
                    ((1, "conv_mfma_f16_64x64x64_k3", True),), edit=(1, "overflow")))
    return out


CASES = cases()
CASE_BY_IDENT = {c.ident: c for c in CASES}
assert len(CASE_BY_IDENT) == len(CASES)
MUTATION_CASES = ("tile-64x64-bk64-k3", "first-nchw-n32-40")           # K = 576 and K = 27
# zoo networks with synth.write_weights' parameters: route, reorg, unfused maxpools, the fp32 conv in front of [region];
# darknet19 at the smallest input it takes (five 2x2/2 maxpools: the last stage is 1x1)
WHOLE_NETWORKS = (("mini-mfma", 64, 2), ("darknet19", 32, 1))
WHOLE_SEED, WHOLE_INPUT_SEED = 11, 77
