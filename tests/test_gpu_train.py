"""Training on the device against the compiled reference (tests/golden/train_*.npz) under the rule of tests/train_rule.py:

    err(A) = max|A - T64| / max|T64|,     a GPU tensor passes when  err(gpu) <= 4 * err(reference golden) + 4 * 2^-23

where T64 is the float64 run of the numpy rule -- the GPU sums the same fp32 products in another order than the reference,
and two orders of one sum have rounding errors of the same distribution; the floor covers tensors the reference happens
to round exactly.  Every tensor's two errors are printed before anything is asserted.  Nets A, B and C, every array after
step 1 and the parameters / update buffers / losses after the later steps, through y2_train_pull.  Then: each y2h_train_*
kernel directly against numpy (the three products with integer-valued data, for which fp32 sums are exact in any order, at
C's shape and at 3 -> 5 channels on 7x5); a step run twice gives the same bytes; predict / save after training see the
trained weights; an untrained network predicts the same bytes before y2_train_prepare and after y2_train_free."""
import ctypes as C
import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_rule as T
from tests.helpers import load_golden
from tests.test_gpu_kernels import Dev, to_nchw, to_nhwc
from tests.test_train_host import REFUSALS, refusal_net, rule_snapshots

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture()
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


def golden_keys(g):
    """(step, layer, array) of every stored layer array"""
    out = []
    for key in sorted(g):
        if key.startswith("s") and "_l" in key and not key.endswith("_loss"):
            out.append((int(key[1]), int(key.split("_")[1][1:]), key.split("_", 2)[2], key))
    return out


def make_net(tmpdir, name, seed):
    cfg, wts, params = T.materialize(str(tmpdir), name, seed)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    return net, params


def gpu_run(name, tmpdir):
    """three steps on the device; what the golden holds is pulled after each (once per session)"""
    if ("gpu", name) in _CACHE:
        return _CACHE[("gpu", name)]
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    net, params = make_net(tmpdir, name, seed)
    net.train_prepare()
    keys = golden_keys(g)
    got, losses = {}, []
    for k in range(1, T.STEPS + 1):
        losses.append(net.train_step(*T.inputs(T.NETS[name], seed, k)))
        for (kk, i, a, key) in keys:
            if kk == k:
                got[key] = net.train_pull(i, a)
    res = dict(net=net, got=got, losses=losses, params=params, g=g, seed=seed)
    _CACHE[("gpu", name)] = res
    return res


def rule_run(name, seed):
    if ("rule", name) not in _CACHE:
        _CACHE[("rule", name)] = rule_snapshots(name, seed)
    return _CACHE[("rule", name)]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_steps_against_the_reference(name, tmp_path_factory):
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    g = r["g"]
    _, snaps, losses = rule_run(name, r["seed"])
    bad, worst = [], (0.0, "")
    for (k, i, a, key) in golden_keys(g):
        t64 = T.subsample(name, a, snaps[k - 1][i][a], k)
        e_ref, e_gpu = T.err(g[key], t64), T.err(T.subsample(name, a, r["got"][key], k), t64)
        ratio = e_gpu / max(e_ref, T.BOUND_FLOOR / T.BOUND_FACTOR)
        print("%s %-24s err(reference) %.3e  err(gpu) %.3e  bound %.3e  ratio %.2f" % (name, key, e_ref, e_gpu, T.bound(e_ref), ratio))
        worst = max(worst, (ratio, key))
        if not e_gpu <= T.bound(e_ref):
            bad.append((key, e_ref, e_gpu))
    for k in range(1, T.STEPS + 1):
        t64 = losses[k - 1]
        e_ref, e_gpu = abs(float(g["s%d_loss" % k][0]) - t64) / abs(t64), abs(r["losses"][k - 1] - t64) / abs(t64)
        print("%s s%d_loss  reference %.7g  gpu %.7g  err(reference) %.3e  err(gpu) %.3e" % (name, k, float(g["s%d_loss" % k][0]), r["losses"][k - 1], e_ref, e_gpu))
        if not e_gpu <= T.bound(e_ref):
            bad.append(("s%d_loss" % k, e_ref, e_gpu))
    print("%s: largest err(gpu) / max(err(reference), 2^-23): %.2f at %s" % (name, worst[0], worst[1]))
    assert not bad, bad


def test_subdivisions_update_on_the_second_call_only(tmp_path_factory):
    """B (subdivisions=2): the odd call changes no parameter and leaves its gradients in the update buffers; the second
    call adds its own to them before the update"""
    r = gpu_run("B", tmp_path_factory.mktemp("trainB"))
    got, params = r["got"], r["params"]
    convs = [i for i, p in enumerate(params) if p is not None]
    for i in convs:
        assert np.array_equal(got["s1_l%d_weights" % i], params[i]["weights"].reshape(-1))
        assert np.array_equal(got["s1_l%d_biases" % i], params[i]["biases"])
        assert np.abs(got["s1_l%d_weight_updates" % i]).max() > 0 and np.abs(got["s1_l%d_bias_updates" % i]).max() > 0
        assert not np.array_equal(got["s2_l%d_weights" % i], got["s1_l%d_weights" % i])
        # call 3 is odd again: parameters as call 2 left them, buffers = momentum * (call 1 + call 2 + decay) + call 3
        assert np.array_equal(got["s3_l%d_weights" % i], got["s2_l%d_weights" % i])
        assert not np.array_equal(got["s3_l%d_weight_updates" % i], got["s2_l%d_weight_updates" % i])
    # rolling statistics move on every call, update or not
    assert not np.array_equal(got["s1_l1_rolling_mean"], params[1]["rolling_mean"])


# ---- the kernels, one by one ----
def conv_geo(batch, h, w, c, n, size, pad):
    return darknet.TrainConv(batch, h, w, c, n, size, pad, h + 2 * pad - size + 1, w + 2 * pad - size + 1)


def small_ints(seed, shape, lo, hi):
    rng = np.random.RandomState(seed)
    return rng.randint(lo, hi + 1, size=shape).astype(np.float32)


PRODUCT_SHAPES = [(4, 32, 32, 64, 64, 3, 1), (2, 5, 7, 3, 5, 3, 1), (3, 5, 7, 3, 5, 1, 0), (2, 9, 7, 6, 7, 5, 2), (2, 7, 9, 3, 6, 3, 0),
                  (1, 11, 13, 70, 66, 3, 1)]


@pytest.mark.parametrize("shape", PRODUCT_SHAPES, ids=lambda s: "b%d_%dx%d_c%d_n%d_k%d_p%d" % s)
def test_three_products_exactly(dev, shape):
    """integer-valued operands: every fp32 partial sum is exact in any order, so each product must EQUAL numpy's"""
    b, h, w, c, n, k, p = shape
    L = dev.L
    g = conv_geo(*shape)
    oh, ow = g.out_h, g.out_w
    x = small_ints(1, (b, c, h, w), -3, 3)
    wt = small_ints(2, (n, c, k, k), -2, 2)
    dy = small_ints(3, (b, n, oh, ow), -2, 2)
    dw0 = small_ints(4, (n, c, k, k), -5, 5)
    xp = np.zeros((b, c, h + 2 * p, w + 2 * p), np.float64)
    xp[:, :, p:p + h, p:p + w] = x
    y_ref = np.zeros((b, n, oh, ow))
    dw_ref = dw0.astype(np.float64)
    dxp = np.zeros_like(xp)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + oh, kx:kx + ow]
            y_ref += np.einsum("bchw,nc->bnhw", win, wt[:, :, ky, kx].astype(np.float64))
            dw_ref[:, :, ky, kx] += np.einsum("bnhw,bchw->nc", dy.astype(np.float64), win)
            dxp[:, :, ky:ky + oh, kx:kx + ow] += np.einsum("bnhw,nc->bchw", dy.astype(np.float64), wt[:, :, ky, kx].astype(np.float64))
    dx_ref = dxp[:, :, p:p + h, p:p + w]
    assert max(np.abs(y_ref).max(), np.abs(dw_ref).max(), np.abs(dx_ref).max()) < 2 ** 24
    packed = np.ascontiguousarray(wt.transpose(2, 3, 1, 0))                 # [k][k][c][n]
    d_x, d_w, d_dy = dev.put(to_nhwc(x)), dev.put(packed), dev.put(to_nhwc(dy))
    d_y, d_dx = dev.empty(y_ref.size * 4), dev.empty(x.size * 4)
    d_dw = dev.put(np.ascontiguousarray(dw0.transpose(2, 3, 1, 0)))
    d_ws = dev.empty(L.y2h_train_dweight_ws_bytes(C.byref(g)))
    assert L.y2h_train_conv_forward(C.byref(g), d_x, d_w, d_y, None) == 0
    assert L.y2h_train_conv_dinput(C.byref(g), d_dy, d_w, d_dx, None) == 0
    assert L.y2h_train_conv_dweight(C.byref(g), d_x, d_dy, d_dw, d_ws, None) == 0
    assert np.array_equal(to_nchw(dev.get(d_y, (b, oh, ow, n))), y_ref.astype(np.float32))
    assert np.array_equal(to_nchw(dev.get(d_dx, (b, h, w, c))), dx_ref.astype(np.float32))
    assert np.array_equal(dev.get(d_dw, (k, k, c, n)).transpose(3, 2, 0, 1), dw_ref.astype(np.float32))
    if shape == PRODUCT_SHAPES[0]:
        assert L.y2h_train_dweight_splits(C.byref(g)) > 1           # the 4096-long reduction crosses its split


def test_products_refuse_bad_shapes(dev):
    g = conv_geo(1, 4, 4, 3, 2, 3, 1)
    g.out_h = 5
    assert dev.L.y2h_train_conv_forward(C.byref(g), dev.empty(64), dev.empty(64), dev.empty(64), None) != 0
    assert dev.L.y2h_train_dweight_ws_bytes(C.byref(g)) == 0


@pytest.mark.parametrize("rows,c", [(35, 7), (4096, 64), (130, 33)])
def test_batchnorm_kernels(dev, rows, c):
    """statistics, apply, the bias / scale gradients, the two delta sums and normalize_delta against float64 numpy.
    Bound: a sum of `rows` fp32 terms in any order is within rows * 2^-24 of the exact sum relative to sum|terms|; the
    statistics here have sum|terms| <= 4 * |result| except where stated."""
    L = dev.L
    rng = np.random.RandomState(rows + c)
    x = (rng.rand(rows, c).astype(np.float32) * 4 - 1)
    delta = rng.randn(rows, c).astype(np.float32)
    scales = (rng.rand(c).astype(np.float32) + .5)
    biases = rng.randn(c).astype(np.float32)
    roll_m, roll_v = rng.randn(c).astype(np.float32), rng.rand(c).astype(np.float32)
    tol = 4 * rows * 2.0 ** -24 + 2.0 ** -21
    scratch = dev.empty(L.y2h_train_reduce_scratch_bytes(rows, c))
    d_x, d_mean, d_var = dev.put(x), dev.empty(c * 4), dev.empty(c * 4)
    d_rm, d_rv = dev.put(roll_m), dev.put(roll_v)
    assert L.y2h_train_bn_stats(d_x, rows, c, d_mean, d_var, d_rm, d_rv, scratch, None) == 0
    x64 = x.astype(np.float64)
    mean64 = x64.sum(0) * float(np.float32(1. / rows))
    var64 = ((x64 - mean64) ** 2).sum(0) * float(np.float32(1. / (rows - 1)))
    mean, var = dev.get(d_mean, c), dev.get(d_var, c)
    assert np.abs(mean - mean64).max() <= tol * np.abs(x64).sum(0).max() / rows
    assert T.err(var, var64) <= tol
    assert T.err(dev.get(d_rm, c), roll_m * np.float64(np.float32(.9)) + np.float64(np.float32(.1)) * mean64) <= tol
    assert T.err(dev.get(d_rv, c), roll_v * np.float64(np.float32(.9)) + np.float64(np.float32(.1)) * var64) <= tol
    # apply: one rounding per step of (x - mean) / (sqrt(var) + 1e-6f) * scale + bias, leaky
    d_y, d_xs, d_xn = dev.put(x), dev.empty(x.nbytes), dev.empty(x.nbytes)
    assert L.y2h_train_bn_apply(d_y, d_xs, d_xn, d_mean, d_var, dev.put(scales), dev.put(biases), 1, rows, c, None) == 0
    m64, v64 = mean.astype(np.float64), var.astype(np.float64)
    xn64 = (x64 - m64) / (np.sqrt(v64) + float(np.float32(.000001)))
    pre = xn64 * scales + biases
    assert np.array_equal(dev.get(d_xs, (rows, c)), x)
    x_norm = dev.get(d_xn, (rows, c))
    assert T.err(x_norm, xn64) <= 2.0 ** -22
    assert np.abs(dev.get(d_y, (rows, c)) - np.where(pre > 0, pre, .1 * pre)).max() <= 2.0 ** -21 * np.abs(pre).max()
    # bias / scale gradients add to what the buffers hold
    b0, s0 = rng.randn(c).astype(np.float32), rng.randn(c).astype(np.float32)
    d_b, d_s, d_delta = dev.put(b0), dev.put(s0), dev.put(delta)
    assert L.y2h_train_bias_grad(d_delta, d_xn, rows, c, d_b, d_s, scratch, None) == 0
    d64, xn = delta.astype(np.float64), x_norm.astype(np.float64)
    assert np.abs(dev.get(d_b, c) - (b0 + d64.sum(0))).max() <= tol * np.abs(d64).sum(0).max() + 2.0 ** -22 * np.abs(b0).max()
    assert np.abs(dev.get(d_s, c) - (s0 + (d64 * xn).sum(0))).max() <= tol * np.abs(d64 * xn).sum(0).max() + 2.0 ** -22 * np.abs(s0).max()
    d_b2 = dev.put(b0)
    assert L.y2h_train_bias_grad(d_delta, None, rows, c, d_b2, None, scratch, None) == 0
    assert np.array_equal(dev.get(d_b2, c), dev.get(d_b, c))
    # mean_delta, variance_delta (the delta scaled on the fly), normalize_delta
    d_md, d_vd = dev.empty(c * 4), dev.empty(c * 4)
    d_sc = dev.put(scales)
    assert L.y2h_train_bn_deltas(d_delta, d_x, d_sc, d_mean, d_var, rows, c, d_md, d_vd, scratch, None) == 0
    ds = d64 * scales
    eps = float(np.float32(.00001))
    md64 = ds.sum(0) * (-1. / np.sqrt(v64 + eps))
    vd64 = (ds * (x64 - m64)).sum(0) * (-.5 * np.power(v64 + eps, -1.5))
    md, vd = dev.get(d_md, c), dev.get(d_vd, c)
    assert np.abs(md - md64).max() <= tol * (np.abs(ds).sum(0) / np.sqrt(v64 + eps)).max()
    assert np.abs(vd - vd64).max() <= tol * (np.abs(ds * (x64 - m64)).sum(0) * .5 * np.power(v64 + eps, -1.5)).max()
    assert L.y2h_train_bn_backward(d_delta, d_x, d_sc, d_mean, d_var, d_md, d_vd, rows, c, None) == 0
    want = ds / (np.sqrt(v64) + eps) + vd.astype(np.float64) * 2. * (x64 - m64) / rows + md.astype(np.float64) / rows
    assert np.abs(dev.get(d_delta, (rows, c)) - want).max() <= 2.0 ** -21 * np.abs(want).max()
    assert L.y2h_train_bn_stats(d_x, 1, c, d_mean, d_var, d_rm, d_rv, scratch, None) != 0      # rows - 1 == 0


@pytest.mark.parametrize("act,name", [(1, "leaky"), (2, "logistic"), (3, "relu"), (0, "linear")])
def test_activation_gradient(dev, act, name):
    y = small_ints(5, 1000, -4, 4) / np.float32(8)
    d = small_ints(6, 1000, -9, 9)
    d_d = dev.put(d)
    assert dev.L.y2h_train_act_gradient(dev.put(y), d_d, act, y.size, None) == 0
    grad = {"leaky": np.where(y > 0, np.float32(1), np.float32(.1)), "logistic": (1 - y) * y, "relu": (y > 0).astype(np.float32),
            "linear": np.ones_like(y)}[name]
    assert np.array_equal(dev.get(d_d, y.size), d * grad)
    assert dev.L.y2h_train_act_gradient(dev.put(y), d_d, 6, y.size, None) != 0                  # tanh is not trainable


@pytest.mark.parametrize("b,h,w,c,size,stride", [(2, 10, 12, 8, 2, 2), (3, 5, 6, 12, 2, 1), (2, 7, 9, 5, 3, 2), (1, 8, 8, 3, 3, 2)])
def test_maxpool_forward_and_backward(dev, b, h, w, c, size, stride):
    """distinct values (a permutation): the winner is unique and everything is exact; with ties (few distinct values)
    the gradient goes to the FIRST maximum in scan order"""
    L = dev.L
    pad = (size - 1) // 2
    oh, ow = (h + 2 * pad) // stride, (w + 2 * pad) // stride
    for ties in (False, True):
        rng = np.random.RandomState(b * h + size + ties)
        x = (rng.randint(0, 3, size=(b, c, h, w)) if ties else rng.permutation(b * c * h * w).reshape(b, c, h, w)).astype(np.float32)
        dy = small_ints(7, (b, c, oh, ow), -4, 4)
        y_ref, dx_ref = np.zeros((b, c, oh, ow), np.float32), np.zeros_like(x)
        for bb in range(b):                      # maxpool_layer.c:79-117 as written
            for k in range(c):
                for i in range(oh):
                    for j in range(ow):
                        best, at = -T.FLT_MAX, None
                        for n in range(size):
                            for m in range(size):
                                ch, cw = i * stride - pad + n, j * stride - pad + m
                                v = x[bb, k, ch, cw] if 0 <= ch < h and 0 <= cw < w else -T.FLT_MAX
                                if v > best:
                                    best, at = v, (ch, cw)
                        y_ref[bb, k, i, j] = best
                        dx_ref[bb, k, at[0], at[1]] += dy[bb, k, i, j]
        d_y, d_idx, d_dx = dev.empty(y_ref.nbytes), dev.empty(y_ref.nbytes), dev.empty(x.nbytes)
        assert L.y2h_train_maxpool_forward(dev.put(to_nhwc(x)), d_y, d_idx, b, h, w, c, size, stride, pad, oh, ow, None) == 0
        assert L.y2h_train_maxpool_backward(dev.put(to_nhwc(dy)), d_idx, d_dx, b, h, w, c, size, stride, pad, oh, ow, None) == 0
        assert np.array_equal(to_nchw(dev.get(d_y, (b, oh, ow, c))), y_ref)
        assert np.array_equal(to_nchw(dev.get(d_dx, (b, h, w, c))), dx_ref)


def test_avgpool_softmax_cost_sgd(dev):
    L = dev.L
    b, hw, c = 3, 35, 10
    x = small_ints(8, (b, hw, c), -8, 8)
    d_y = dev.empty(b * c * 4)
    assert L.y2h_train_avgpool_forward(dev.put(x), d_y, b, hw, c, None) == 0
    assert np.array_equal(dev.get(d_y, (b, c)), (x.sum(1) / np.float32(hw)).astype(np.float32))
    dy = small_ints(9, (b, c), -8, 8)
    d_dx = dev.empty(x.nbytes)
    assert L.y2h_train_avgpool_backward(dev.put(dy), d_dx, b, hw, c, None) == 0
    assert np.array_equal(dev.get(d_dx, (b, hw, c)), np.broadcast_to((dy / np.float32(hw))[:, None, :], x.shape))
    # softmax with a temperature: exp in double, fp32 sum in index order (blas.c:205-221)
    logits = (small_ints(10, (b, c), -20, 20) / np.float32(4))
    d_p = dev.empty(logits.nbytes)
    assert L.y2h_train_softmax(dev.put(logits), d_p, b, c, 2.0, None) == 0
    e = np.exp(logits.astype(np.float64) / 2 - logits.max(1, keepdims=True).astype(np.float64) / 2)
    assert T.err(dev.get(d_p, (b, c)), e / e.sum(1, keepdims=True)) <= c * 2.0 ** -23
    # cost: integer-valued differences, every sum exact
    pred, truth = small_ints(11, 700, -5, 5), small_ints(12, 700, -5, 5)
    d_err, d_delta, d_prev, d_cost = dev.empty(2800), dev.empty(2800), dev.empty(2800), dev.empty(16)
    assert L.y2h_train_cost_sse(dev.put(pred), dev.put(truth), d_err, d_delta, d_prev, 0.5, 700, d_cost, None) == 0
    assert np.array_equal(dev.get(d_delta, 700), truth - pred) and np.array_equal(dev.get(d_prev, 700), (truth - pred) * np.float32(.5))
    assert np.array_equal(dev.get(d_err, 700), (truth - pred) ** 2) and dev.get(d_cost, 1)[0] == ((truth - pred) ** 2).sum()
    # the update's three statements, one rounding each (the library is built without contraction)
    rng = np.random.RandomState(3)
    w, u = rng.randn(5000).astype(np.float32), rng.randn(5000).astype(np.float32)
    rate, wd, mom = np.float32(0.01 / 3), np.float32(-0.0005 * 3), np.float32(0.9)
    for decay in (wd, np.float32(0)):
        d_w, d_u = dev.put(w), dev.put(u)
        assert L.y2h_train_sgd(d_w, d_u, w.size, rate, decay, mom, None) == 0
        u1 = (u + decay * w).astype(np.float32) if decay != 0 else u
        w1 = (w + (rate * u1).astype(np.float32)).astype(np.float32)
        assert np.array_equal(dev.get(d_w, w.size), w1) and np.array_equal(dev.get(d_u, w.size), (u1 * mom).astype(np.float32))


# ---- whole steps ----
def all_arrays(net, spec):
    out = {}
    for i, l in enumerate(spec["layers"]):
        names = [a for a in T.CONV_ARRAYS if l[4] or a in ("output", "delta", "weights", "biases", "weight_updates", "bias_updates")] \
            if l[0] == "conv" else ["output", "delta"]
        for a in names:
            out[(i, a)] = net.train_pull(i, a)
    return out


@pytest.mark.parametrize("name", ["A", "C"])
def test_a_step_is_bit_identical_twice(name, tmp_path):
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    runs = []
    for rep in range(2):
        net, _ = make_net(tmp_path, name, seed)
        net.train_prepare()
        losses = [net.train_step(*T.inputs(T.NETS[name], seed, k)) for k in (1, 2)]
        runs.append((losses, all_arrays(net, T.NETS[name])))
        net.free()
    assert runs[0][0] == runs[1][0]
    for key, a in runs[0][1].items():
        assert a.tobytes() == runs[1][1][key].tobytes(), key


@pytest.mark.parametrize("name", ["A", "B"])
def test_predict_and_save_see_the_trained_weights(name, tmp_path_factory, tmp_path):
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    net, g, seed = r["net"], r["g"], r["seed"]
    x1, _ = T.inputs(T.NETS[name], seed, 1)
    out = net.network_predict(x1)                       # inference mode: rolling statistics, folded batch norm
    print("%s: max|predict - reference's predict after its three steps| = %.3g" % (name, np.abs(out - g["predict"]).max()))
    assert np.abs(out - g["predict"]).max() < 1e-4
    # the host arrays now hold the masters
    for i, p in enumerate(r["params"]):
        if p is not None:
            l = net.layer(i)
            host = np.ctypeslib.as_array(l.weights, shape=(p["weights"].size,))
            assert np.array_equal(host, net.train_pull(i, "weights")) and not np.array_equal(host, p["weights"].reshape(-1))
    saved = str(tmp_path / "trained.weights")
    net.save_weights(saved)
    cfg, _, _ = T.materialize(str(tmp_path), name, seed)
    fresh = darknet.Network.parse_network_cfg(cfg)
    fresh.load_weights(saved)
    assert fresh.network_predict(x1).tobytes() == out.tobytes()
    assert fresh.net.seen[0] == net.net.seen[0] == T.STEPS * T.NETS[name]["batch"]
    fresh.free()
    # and training goes on from where it was: a fourth step still moves the weights, predict follows
    before = net.train_pull(0, "weights").copy()
    net.train_step(*T.inputs(T.NETS[name], seed, 2))
    if name == "A":
        assert not np.array_equal(net.train_pull(0, "weights"), before)
        assert net.network_predict(x1).tobytes() != out.tobytes()


def test_untrained_predict_is_untouched_by_the_trainer(tmp_path):
    g = load_golden("train_A")
    seed = int(g["seed"])
    x1, y1 = T.inputs(T.NETS["A"], seed, 1)
    net, _ = make_net(tmp_path, "A", seed)
    before = net.network_predict(x1)
    net.train_prepare()
    assert net.network_predict(x1).tobytes() == before.tobytes()      # prepared but clean: nothing is synced
    net.train_free()
    assert net.network_predict(x1).tobytes() == before.tobytes()
    # train_network_datum prepares lazily; set_batch_network / load_weights drop the trainer
    L = darknet.lib()
    loss = L.train_network_datum(net.net, x1.ctypes.data, y1.ctypes.data)
    assert abs(loss - float(g["s1_loss"][0])) <= 1e-4 * abs(loss)
    assert net.get_network_cost() == loss and net.get_current_batch() == 1
    net.set_batch_network(T.NETS["A"]["batch"])
    with pytest.raises(darknet.Y2Error, match="no trainer"):
        net.train_pull(0, "weights")
    net.free()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_on_the_device_machine(tmp_path, what):
    net, pattern = refusal_net(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    net.free()


def host_weights(net, i):
    l = net.layer(i)
    return np.ctypeslib.as_array(l.weights, shape=(l.n * l.c * l.size * l.size,)).copy()


def test_device_entry_sync_and_null_deltas(tmp_path, dev):
    """y2_train_step_device with the batch and its truth already in HBM does what y2_train_step does, bit for bit;
    y2_train_sync brings the masters into the host layer arrays; layer.delta stays NULL throughout"""
    g = load_golden("train_A")
    seed, spec = int(g["seed"]), T.NETS["A"]
    x1, y1 = T.inputs(spec, seed, 1)
    host, _ = make_net(tmp_path, "A", seed)
    device, params = make_net(tmp_path, "A", seed)
    host.train_prepare()
    device.train_prepare()
    loss_h = host.train_step(x1, y1)
    loss_d = device.train_step_device(dev.put(x1).value, dev.put(y1).value)
    assert loss_h == loss_d
    a, b = all_arrays(host, spec), all_arrays(device, spec)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert np.array_equal(host_weights(device, 0), params[0]["weights"].reshape(-1))      # not synced yet
    device.train_sync()
    for i, p in enumerate(params):
        if p is not None:
            assert np.array_equal(host_weights(device, i), device.train_pull(i, "weights"))
            assert not np.array_equal(host_weights(device, i), p["weights"].reshape(-1))
    for net in (host, device):
        assert all(not net.layer(i).delta for i in range(net.n))
        net.free()


def arena_bytes(net):
    L = darknet.lib()
    ptr, n = C.c_void_p(), C.c_size_t(0)
    assert L.y2_weights_arena(C.byref(net.net), C.byref(ptr), C.byref(n)) == 0, L.y2_last_error()
    out = np.zeros(n.value, np.uint8)
    assert L.y2h_device_sync() == 0 and L.y2h_memcpy_d2h(out.ctypes.data, ptr, n.value, None) == 0 and L.y2h_device_sync() == 0
    return out


def test_arena_batch_change_and_denormalize_after_training(tmp_path):
    """what reads or rewrites the weights after a step sees the trained ones: y2_weights_arena hands out an arena that was
    packed from them; set_batch_network keeps the steps; y2_denormalize_network folds the trained weights;
    denormalize_convolutional_layer, which cannot reach the trainer, refuses while one exists"""
    g = load_golden("train_A")
    seed, spec = int(g["seed"]), T.NETS["A"]
    x1, y1 = T.inputs(spec, seed, 1)
    net, params = make_net(tmp_path, "A", seed)
    net.network_predict(x1)                                   # the plan is built and the arena holds the loaded weights
    before = arena_bytes(net)
    net.train_step(x1, y1)
    trained = arena_bytes(net)                                # no predict in between
    assert not np.array_equal(trained, before)
    saved = str(tmp_path / "one_step.weights")
    net.save_weights(saved)
    cfg, _, _ = T.materialize(str(tmp_path), "A", seed)
    fresh = darknet.Network.parse_network_cfg(cfg)
    fresh.load_weights(saved)
    want = fresh.network_predict(x1)
    assert np.array_equal(arena_bytes(fresh), trained)
    # train, set_batch_network, predict: the reference's sequence keeps what was trained
    L = darknet.lib()
    L.denormalize_convolutional_layer.restype = None
    L.denormalize_convolutional_layer.argtypes = [darknet.Layer]
    w1 = host_weights(net, 0)
    L.denormalize_convolutional_layer(net.layer(0))
    assert L.y2_failed_and_clear() and "has a trainer" in L.y2_last_error().decode()
    assert np.array_equal(host_weights(net, 0), w1)
    net.train_step(x1, y1)
    w2 = net.train_pull(0, "weights").copy()
    net.set_batch_network(spec["batch"])
    assert np.array_equal(host_weights(net, 0), w2)
    with pytest.raises(darknet.Y2Error, match="no trainer"):
        net.train_pull(0, "weights")
    # one more step (a new trainer), then the fold: it must fold the weights of that step, and the trainer is gone
    net.train_step(x1, y1)
    w3 = net.train_pull(0, "weights").copy()
    scales, var = net.train_pull(0, "scales"), net.train_pull(0, "rolling_variance")
    net.denormalize()
    per = w3.size // scales.size
    folded = (w3.reshape(scales.size, per) * (scales / np.sqrt(var.astype(np.float64) + .00001)).astype(np.float32)[:, None]).reshape(-1)
    assert np.allclose(host_weights(net, 0), folded, rtol=1e-6, atol=0)
    with pytest.raises(darknet.Y2Error, match="no trainer"):
        net.train_pull(0, "weights")
    net.network_predict(x1)
    assert np.allclose(host_weights(net, 0), folded, rtol=1e-6, atol=0)      # no master came back over the folded arrays
    assert want.shape == (spec["batch"] * 5,)
    fresh.free()
    net.free()
