"""The trainer's bf16 precision modes on the device (y2_train_bf16.hip; y2_train_set_precision).

1. The three products of both kernels (planes = 3: the 3-way split; planes = 1: operands rounded to bf16) on integer-valued
   operands, for which every partial sum is exact in any order: each result must EQUAL numpy's.  Three further data sets at
   planes = 3 make each of the six kept products necessary: (M) both operands of 9-12 significant bits, so both middle
   planes are non-zero; (L) / (L') one operand h = 2^17, m = 256, l = 1 (or its double) against +-1 / +-2, either way round.
   That every partial sum of the split planes is an integer below 2^24 is asserted before the device is touched.
2. The same shapes with normal operands against float64, under bounds that are derived, not measured.  R is the reduction
   length, u = 2^-24.  planes = 1: the device rounds the operands exactly as the rule's bf16_rn does, products of two bf16
   numbers are exact in fp32, and R terms summed in fp32 in any order are within R u (|A_r| . |B_r|) of their exact sum.
   planes = 3: the six kept products of a term are exact, so the result is a recursive fp32 sum of 6 R exact terms, within
   6 R u (|A| . |B|) of their sum to first order (the 1.01 covers the higher orders and the planes' |h| + |m| + |l| >= |a|),
   and the dropped products are below 2^-25 |a b| per term: (6 R + 1) u (|A| . |B|) * 1.01.
3. Split mode on the fixtures A, B, C, E, F, G under the fp32 bound of tests/test_gpu_train.py, T.bound(err(reference)).
4. bf16 mode on A, B, E against Bf16Trainer (tests/train_bf16_rule.py) run in float64 and in float32:
   err(gpu, T64) <= 4 * max(err(rule64_bf16, T64), err(rule32_bf16, T64)) + 4 * 2^-23, T64 the plain float64 rule.
5. A step run twice gives the same bytes in both modes; a mode set and taken back leaves fp32 training bit-identical; steps in
   fp32 mode around a bf16x3 step launch the fp32 kernels.
6. predict / save after bf16x3 steps see the trained weights; set_batch_network keeps the mode.

Measured on one MI355X.  bf16x3, largest err(gpu) / max(err(reference), 2^-23) over stored tensors and losses (the bound is
4): A 1.00, B 1.64, C 1.21, E 1.33, F 1.90, G 2.04.  bf16, largest err(gpu) / (4 * err(rule bf16) + 4 * 2^-23): 0.25 on A, B
and E -- the device is as far from the float64 rule as the rounded rule itself.  Products on normal operands: at most 0.44
of the derived bound (planes = 1, R = 3), below 0.04 from R = 24 up."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import test_gpu_train as G
from tests import test_gpu_train_det as GD
from tests import train_bf16_rule as R
from tests import train_det_rule as D
from tests import train_rule as T
from tests.helpers import load_golden
from tests.test_gpu_kernels import Dev, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu

_CACHE = {}
U = 2.0 ** -24


@pytest.fixture()
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


# ---- 1, 2: the products ----
PRODUCT_SHAPES = [(4, 32, 32, 64, 64, 3, 1), (2, 5, 7, 3, 5, 3, 1), (3, 5, 7, 3, 5, 1, 0), (2, 9, 7, 6, 7, 5, 2), (2, 7, 9, 3, 6, 3, 0),
                  (1, 11, 13, 70, 66, 3, 1), (1, 6, 5, 40, 24, 1, 0), (1, 3, 3, 1, 1, 3, 1)]
SHAPE_ID = lambda s: "b%d_%dx%d_c%d_n%d_k%d_p%d" % s          # noqa: E731


def products_ref(shape, x, wt, dy, dw0):
    """float64 forward, input gradient and weight gradient of one convolution, in the reference's layouts"""
    b, h, w, c, n, k, p = shape
    oh, ow = h + 2 * p - k + 1, w + 2 * p - k + 1
    x, wt, dy = x.astype(np.float64), wt.astype(np.float64), dy.astype(np.float64)
    xp = np.zeros((b, c, h + 2 * p, w + 2 * p))
    xp[:, :, p:p + h, p:p + w] = x
    y = np.zeros((b, n, oh, ow))
    dw = dw0.astype(np.float64).copy()
    dxp = np.zeros_like(xp)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + oh, kx:kx + ow]
            y += np.einsum("bchw,nc->bnhw", win, wt[:, :, ky, kx], optimize=True)
            dw[:, :, ky, kx] += np.einsum("bnhw,bchw->nc", dy, win, optimize=True)
            dxp[:, :, ky:ky + oh, kx:kx + ow] += np.einsum("bnhw,nc->bchw", dy, wt[:, :, ky, kx], optimize=True)
    return dict(fwd=y, dx=dxp[:, :, p:p + h, p:p + w], dw=dw)


def products_gpu(dev, shape, x, wt, dy, dw0, planes, which=("fwd", "dx", "dw")):
    b, h, w, c, n, k, p = shape
    L = dev.L
    g = G.conv_geo(*shape)
    oh, ow = g.out_h, g.out_w
    d_x, d_w, d_dy = dev.put(to_nhwc(x)), dev.put(np.ascontiguousarray(wt.transpose(2, 3, 1, 0))), dev.put(to_nhwc(dy))
    out = {}
    if "fwd" in which:
        d_y = dev.empty(b * n * oh * ow * 4)
        assert L.y2h_train_conv_forward_bf16(C.byref(g), d_x, d_w, d_y, planes, None) == 0
        out["fwd"] = to_nchw(dev.get(d_y, (b, oh, ow, n)))
    if "dx" in which:
        d_dx = dev.empty(x.size * 4)
        assert L.y2h_train_conv_dinput_bf16(C.byref(g), d_dy, d_w, d_dx, planes, None) == 0
        out["dx"] = to_nchw(dev.get(d_dx, (b, h, w, c)))
    if "dw" in which:
        d_dw = dev.put(np.ascontiguousarray(dw0.transpose(2, 3, 1, 0)))
        d_ws = dev.empty(L.y2h_train_dweight_ws_bytes(C.byref(g)))
        assert L.y2h_train_conv_dweight_bf16(C.byref(g), d_x, d_dy, d_dw, d_ws, planes, None) == 0
        out["dw"] = dev.get(d_dw, (k, k, c, n)).transpose(3, 2, 0, 1)
    return out


def tensor_shapes(shape):
    b, h, w, c, n, k, p = shape
    return (b, c, h, w), (n, c, k, k), (b, n, h + 2 * p - k + 1, w + 2 * p - k + 1)


def plane_abs(a):
    """|h| + |m| + |l| of the rule's split: what bounds every partial sum of the split planes"""
    h, m, l = R.split3(a)
    return sum(np.abs(R.bf16_f32(v).astype(np.float64)) for v in (h, m, l)).reshape(a.shape)


def assert_exact_in_fp32(shape, x, wt, dy, dw0, which):
    """every operand an integer, and every partial sum of the split planes' products, in any order, below 2^24"""
    for a in (x, wt, dy, dw0):
        assert np.array_equal(a, np.round(a))
    top = products_ref(shape, plane_abs(x), plane_abs(wt), plane_abs(dy), np.abs(dw0))
    for key in which:
        assert top[key].max() < 2 ** 24, (key, top[key].max())


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("shape", PRODUCT_SHAPES, ids=SHAPE_ID)
def test_products_exactly(dev, shape, planes):
    """the operands of tests/test_gpu_train.py::test_three_products_exactly: integers in [-3, 3] and [-2, 2]"""
    sx, sw, sy = tensor_shapes(shape)
    x, wt, dy, dw0 = G.small_ints(1, sx, -3, 3), G.small_ints(2, sw, -2, 2), G.small_ints(3, sy, -2, 2), G.small_ints(4, sw, -5, 5)
    assert_exact_in_fp32(shape, x, wt, dy, dw0, ("fwd", "dx", "dw"))
    ref = products_ref(shape, x, wt, dy, dw0)
    got = products_gpu(dev, shape, x, wt, dy, dw0, planes)
    for key in ("fwd", "dx", "dw"):
        assert np.array_equal(got[key], ref[key].astype(np.float32)), key
    if shape == PRODUCT_SHAPES[0]:
        assert dev.L.y2h_train_dweight_splits(C.byref(G.conv_geo(*shape))) > 1      # the 4096-long reduction crosses its split


def odd_ints(rng, shape, lo, hi):
    """signed odd integers with lo <= |v| <= hi: an odd v in [2^(k-1), 2^k) has exactly k significant bits"""
    v = rng.randint(lo // 2, (hi - 1) // 2 + 1, size=shape) * 2 + 1
    return (v * rng.choice([-1, 1], size=shape)).astype(np.float32)


def big_values(rng, shape):
    """+-131329 = 2^17 + 256 + 1 (h = 2^17, m = 256, l = 1), about one in 32 doubled: the longest reduction here has 105
    terms and 2^24 / 131329 = 127.7"""
    v = 131329.0 * np.where(rng.randint(32, size=shape) == 0, 2, 1)
    v.flat[0], v.flat[-1] = 262658.0, 131329.0                  # both occur, however small the tensor
    return (v * rng.choice([-1, 1], size=shape)).astype(np.float32)


def unit_values(rng, shape):
    v = np.where(rng.randint(32, size=shape) == 0, 2.0, 1.0)
    return (v * rng.choice([-1, 1], size=shape)).astype(np.float32)


# which two of (x, w, dy) a product reads, as (A, B) of its GEMM
OPERANDS = {"fwd": ("x", "w"), "dx": ("dy", "w"), "dw": ("x", "dy")}


@pytest.mark.parametrize("case", ["M", "L", "Lp"])
@pytest.mark.parametrize("shape", [PRODUCT_SHAPES[1], PRODUCT_SHAPES[2]], ids=SHAPE_ID)
def test_every_kept_term_is_needed(dev, shape, case):
    k = shape[5]
    shapes = dict(zip(("x", "w", "dy"), tensor_shapes(shape)))
    for prod, (an, bn) in OPERANDS.items():
        rng = np.random.RandomState(100 + len(prod) + 7 * k)
        t = {name: np.zeros(s, np.float32) for name, s in shapes.items()}
        if case == "M":
            # 9 significant bits for the activations and deltas; 9-10 (3x3) or 9-12 (1x1: reductions of 3 and 5) for the weights
            for name in (an, bn):
                t[name] = odd_ints(rng, shapes[name], 257, (4095 if k == 1 else 895) if name == "w" else 383)
        else:
            big, small = (an, bn) if case == "L" else (bn, an)
            t[big], t[small] = big_values(rng, shapes[big]), unit_values(rng, shapes[small])
        dw0 = G.small_ints(4, shapes["w"], -5, 5)
        assert_exact_in_fp32(shape, t["x"], t["w"], t["dy"], dw0, (prod,))
        # the planes the case is about are there
        (ha, ma, la), (hb, mb, lb) = R.split3(t[an]), R.split3(t[bn])
        if case == "M":
            assert ma.all() and mb.all() and not la.any() and not lb.any()
            if k == 1 and "w" in (an, bn):
                assert np.abs(t["w"]).max() >= 2048                              # 12 significant bits occur
        else:
            lbig, lsmall, msmall = (la, lb, mb) if case == "L" else (lb, la, ma)
            assert lbig.all() and not lsmall.any() and not msmall.any()
            assert len(np.unique(np.abs(t[an if case == "L" else bn]))) == 2     # l = 1 and its double
        ref = products_ref(shape, t["x"], t["w"], t["dy"], dw0)[prod]
        got = products_gpu(dev, shape, t["x"], t["w"], t["dy"], dw0, 3, (prod,))[prod]
        assert np.array_equal(got, ref.astype(np.float32)), (prod, case)
        # and the low plane was needed: the same product without the big operand's l differs
        if case != "M":
            big, (hb_, mb_) = (an, (ha, ma)) if case == "L" else (bn, (hb, mb))
            cut = dict(t)
            cut[big] = (R.bf16_f32(hb_) + R.bf16_f32(mb_)).reshape(shapes[big])
            assert not np.array_equal(products_ref(shape, cut["x"], cut["w"], cut["dy"], dw0)[prod], ref)


def reduction_length(shape, prod):
    b, h, w, c, n, k, p = shape
    return {"fwd": k * k * c, "dx": k * k * n, "dw": b * (h + 2 * p - k + 1) * (w + 2 * p - k + 1)}[prod]


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("shape", PRODUCT_SHAPES, ids=SHAPE_ID)
def test_products_within_the_derived_bound(dev, shape, planes):
    sx, sw, sy = tensor_shapes(shape)
    rng = np.random.RandomState(sum(shape))
    x, wt, dy = (rng.randn(*s).astype(np.float32) for s in (sx, sw, sy))
    dw0 = np.zeros(sw, np.float32)
    if planes == 1:
        ops = [R.bf16_round(a) for a in (x, wt, dy)]            # given data: the device and numpy round the same values
    else:
        ops = [x, wt, dy]
    ref = products_ref(shape, *ops, dw0)
    mag = products_ref(shape, *[np.abs(a) for a in ops], dw0)
    got = products_gpu(dev, shape, x, wt, dy, dw0, planes)
    bad = []
    for prod in ("fwd", "dx", "dw"):
        r = reduction_length(shape, prod)
        bound = (r * U if planes == 1 else (6 * r + 1) * U * 1.01) * mag[prod]
        diff = np.abs(got[prod].astype(np.float64) - ref[prod])
        ratio = float((diff / np.maximum(bound, 1e-300)).max())
        print("%s planes %d %-3s R %5d  max|gpu - T| %.3e  largest share of its bound %.3f" % (SHAPE_ID(shape), planes, prod, r, diff.max(), ratio))
        if not np.all(diff <= bound):
            bad.append((prod, ratio))
    assert not bad, bad


def test_entry_points_refuse_what_the_fp32_twins_refuse(dev):
    L = dev.L
    g = G.conv_geo(1, 4, 4, 3, 2, 3, 1)
    a, b, c, ws = dev.empty(1024), dev.empty(1024), dev.empty(1024), dev.empty(1 << 16)
    for planes in (0, 2, 4, -1):
        assert L.y2h_train_conv_forward_bf16(C.byref(g), a, b, c, planes, None) != 0
        assert L.y2h_train_conv_dinput_bf16(C.byref(g), a, b, c, planes, None) != 0
        assert L.y2h_train_conv_dweight_bf16(C.byref(g), a, b, c, ws, planes, None) != 0
    assert L.y2h_train_conv_forward_bf16(C.byref(g), None, b, c, 3, None) != 0
    g.out_h = 5
    for planes in (1, 3):
        assert L.y2h_train_conv_forward_bf16(C.byref(g), a, b, c, planes, None) != 0
        assert L.y2h_train_conv_dinput_bf16(C.byref(g), a, b, c, planes, None) != 0
        assert L.y2h_train_conv_dweight_bf16(C.byref(g), a, b, c, ws, planes, None) != 0


# ---- whole steps ----
def is_det(name):
    return name in D.NETS


def gpu_run(name, mode, tmpdir):
    """three steps in `mode`; what the golden holds is pulled after each (once per session)"""
    if (name, mode) in _CACHE:
        return _CACHE[(name, mode)]
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    net, params = (GD if is_det(name) else G).make_net(tmpdir, name, seed)
    net.train_set_precision(mode)
    net.train_prepare()
    assert net.train_precision() == mode
    keys = G.golden_keys(g)
    got, losses = {}, []
    for k in range(1, T.STEPS + 1):
        losses.append(net.train_step(*(D.inputs(name, seed, k) if is_det(name) else T.inputs(T.NETS[name], seed, k))))
        for (kk, i, a, key) in keys:
            if kk == k:
                got[key] = net.train_pull(i, a)
    res = dict(net=net, got=got, losses=losses, params=params, g=g, seed=seed)
    _CACHE[(name, mode)] = res
    return res


def rule64(name, seed):
    """(snapshots, losses) of the plain float64 rule: the T64 of tests/test_gpu_train.py and its detector twin"""
    r = GD.rule_run(name, seed) if is_det(name) else G.rule_run(name, seed)
    return r[1], r[2]


@pytest.mark.parametrize("name", ["A", "B", "C", "E", "F", "G"])
def test_split_steps_against_the_reference(name, tmp_path_factory):
    r = gpu_run(name, "bf16x3", tmp_path_factory.mktemp("split" + name))
    g = r["g"]
    snaps, losses = rule64(name, r["seed"])
    bad, worst = [], (0.0, "")
    for (k, i, a, key) in G.golden_keys(g):
        t64 = snaps[k - 1][i][a].reshape(-1) if is_det(name) else T.subsample(name, a, snaps[k - 1][i][a], k)
        got = r["got"][key] if is_det(name) else T.subsample(name, a, r["got"][key], k)
        e_ref, e_gpu = T.err(g[key], t64), T.err(got, t64)
        ratio = e_gpu / max(e_ref, T.BOUND_FLOOR / T.BOUND_FACTOR)
        print("%s %-24s err(reference) %.3e  err(gpu) %.3e  bound %.3e  ratio %.2f" % (name, key, e_ref, e_gpu, T.bound(e_ref), ratio))
        worst = max(worst, (ratio, key))
        if not e_gpu <= T.bound(e_ref):
            bad.append((key, e_ref, e_gpu))
    for k in range(1, T.STEPS + 1):
        t64 = losses[k - 1]
        e_ref, e_gpu = abs(float(g["s%d_loss" % k][0]) - t64) / abs(t64), abs(r["losses"][k - 1] - t64) / abs(t64)
        print("%s s%d_loss  reference %.7g  gpu %.7g  err(reference) %.3e  err(gpu) %.3e" % (name, k, float(g["s%d_loss" % k][0]), r["losses"][k - 1], e_ref, e_gpu))
        worst = max(worst, (e_gpu / max(e_ref, T.BOUND_FLOOR / T.BOUND_FACTOR), "s%d_loss" % k))
        if not e_gpu <= T.bound(e_ref):
            bad.append(("s%d_loss" % k, e_ref, e_gpu))
    print("%s bf16x3: largest err(gpu) / max(err(reference), 2^-23): %.2f at %s" % (name, worst[0], worst[1]))
    assert not bad, bad


def bf16_rule_run(name, seed, dtype):
    """Bf16Trainer / Bf16DetTrainer in `dtype`: per step the arrays, the loss and every discrete decision taken"""
    key = ("bf16rule", name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    det = is_det(name)
    spec = D.NETS[name] if det else T.NETS[name]
    t = (R.Bf16DetTrainer if det else R.Bf16Trainer)(spec, D.params_for(name, seed) if det else T.params_for(name, seed), dtype=dtype)
    snaps, losses, decisions = [], [], []
    for k in range(1, T.STEPS + 1):
        losses.append(t.step(*(D.inputs(name, seed, k) if det else T.inputs(spec, seed, k))))
        snaps.append([{a: np.array(v) for a, v in t.arrays(i).items()} for i in range(len(spec["layers"]))])
        dec = []
        for l, d in zip(spec["layers"], t.L):
            if l[0] == "conv" and l[5] in ("leaky", "relu"):
                dec.append(d["output"] > 0)
            if l[0] == "max":
                dec.append(d["arg"].copy())
        if det:
            dec.append(np.array([t.stats["count"], t.stats["class_count"]]))
            dec.append(np.array(t.stats["recall"]))                # the share of truths with iou > .5: a count over a constant
        decisions.append(dec)
    res = dict(t=t, snaps=snaps, losses=losses, decisions=decisions)
    _CACHE[key] = res
    return res


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_bf16_steps_against_the_rounded_rule(name, tmp_path_factory):
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    snaps, losses = rule64(name, seed)
    r64, r32 = bf16_rule_run(name, seed, np.float64), bf16_rule_run(name, seed, np.float32)
    keys = G.golden_keys(g)
    # on the CPU, before any GPU run: both rule runs are off the plain rule by something finite and non-zero, and no
    # discrete decision differs between them: the sign of every leaky / relu output, every maxpool winner, the head's counts,
    # and the head's own margins (threshold, anchor choice, recall, cell) keep the fixture's 1e-4 in both
    if is_det(name):
        for r in (r64, r32):
            assert all(r["t"].margins[k] >= T.KINK for k in ("thresh", "anchor", "recall", "cell")), (name, r["t"].margins)
    for d64, d32 in zip(r64["decisions"], r32["decisions"]):
        assert len(d64) == len(d32) and all(np.array_equal(a, b) for a, b in zip(d64, d32)), name
    yard = {}
    for (k, i, a, key) in keys:
        t64 = snaps[k - 1][i][a].reshape(-1)
        e64, e32 = T.err(r64["snaps"][k - 1][i][a].reshape(-1), t64), T.err(r32["snaps"][k - 1][i][a].reshape(-1), t64)
        assert np.isfinite(e64) and np.isfinite(e32), key
        yard[key] = max(e64, e32)
    assert all(v > 0 for key, v in yard.items() if key.startswith("s3_")), name
    gpu = gpu_run(name, "bf16", tmp_path_factory.mktemp("bf16" + name))
    bad, worst = [], (0.0, "")
    for (k, i, a, key) in keys:
        t64 = snaps[k - 1][i][a].reshape(-1)
        e_gpu, bound = T.err(gpu["got"][key], t64), T.BOUND_FACTOR * yard[key] + T.BOUND_FLOOR
        print("%s %-24s err(rule bf16) %.3e  err(gpu) %.3e  bound %.3e  ratio %.2f" % (name, key, yard[key], e_gpu, bound, e_gpu / bound))
        worst = max(worst, (e_gpu / bound, key))
        if not e_gpu <= bound:
            bad.append((key, yard[key], e_gpu))
    for k in range(1, T.STEPS + 1):
        t64 = losses[k - 1]
        e_rule = max(abs(r["losses"][k - 1] - t64) / abs(t64) for r in (r64, r32))
        e_gpu, bound = abs(gpu["losses"][k - 1] - t64) / abs(t64), T.BOUND_FACTOR * e_rule + T.BOUND_FLOOR
        print("%s s%d_loss  rule %.7g  gpu %.7g  err(rule bf16) %.3e  err(gpu) %.3e" % (name, k, t64, gpu["losses"][k - 1], e_rule, e_gpu))
        worst = max(worst, (e_gpu / bound, "s%d_loss" % k))
        if not e_gpu <= bound:
            bad.append(("s%d_loss" % k, e_rule, e_gpu))
    print("%s bf16: largest err(gpu) / (4 * err(rule bf16) + 4 * 2^-23): %.2f at %s" % (name, worst[0], worst[1]))
    assert not bad, bad


# ---- 5: determinism and non-interference ----
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_a_step_is_bit_identical_twice(name, mode, tmp_path):
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    runs = []
    for rep in range(2):
        net, _ = G.make_net(tmp_path, name, seed)
        net.train_set_precision(mode)
        losses = [net.train_step(*T.inputs(T.NETS[name], seed, k)) for k in (1, 2)]
        runs.append((losses, G.all_arrays(net, T.NETS[name])))
        net.free()
    assert runs[0][0] == runs[1][0]
    for key, a in runs[0][1].items():
        assert a.tobytes() == runs[1][1][key].tobytes(), key


def test_a_mode_taken_back_leaves_fp32_training_untouched(tmp_path):
    g = load_golden("train_A")
    seed, spec = int(g["seed"]), T.NETS["A"]
    plain, _ = G.make_net(tmp_path, "A", seed)
    toggled, _ = G.make_net(tmp_path, "A", seed)
    toggled.train_set_precision("bf16")
    toggled.train_set_precision("fp32")
    for net in (plain, toggled):
        net.train_prepare()
    for k in range(1, T.STEPS + 1):
        x, y = T.inputs(spec, seed, k)
        assert plain.train_step(x, y) == toggled.train_step(x, y)
    a, b = G.all_arrays(plain, spec), G.all_arrays(toggled, spec)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    plain.free()
    toggled.free()


def test_fp32_steps_around_a_split_step_launch_the_fp32_kernels(tmp_path, dev):
    """step 1 of a net that later changes mode equals the untouched net's step 1 byte for byte; its step 3, back in fp32
    mode, holds in layer 0 exactly what y2h_train_conv_forward makes of the step's input and the weights it had, and its
    step 2 what the split entry makes of them"""
    g = load_golden("train_A")
    seed, spec = int(g["seed"]), T.NETS["A"]
    plain, _ = G.make_net(tmp_path, "A", seed)
    net, _ = G.make_net(tmp_path, "A", seed)
    x1, y1 = T.inputs(spec, seed, 1)
    assert plain.train_step(x1, y1) == net.train_step(x1, y1)
    a, b = G.all_arrays(plain, spec), G.all_arrays(net, spec)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    L = dev.L
    l0 = spec["layers"][0]
    shape = (spec["batch"], spec["h"], spec["w"], spec["c"], l0[1], l0[2], l0[2] // 2)
    geo = G.conv_geo(*shape)

    def layer0(x, weights, planes):
        d_y = dev.empty(shape[0] * geo.out_h * geo.out_w * l0[1] * 4)
        d_x, d_w = dev.put(to_nhwc(x)), dev.put(np.ascontiguousarray(weights.reshape(l0[1], spec["c"], l0[2], l0[2]).transpose(2, 3, 1, 0)))
        rc = L.y2h_train_conv_forward(C.byref(geo), d_x, d_w, d_y, None) if planes == 0 else \
            L.y2h_train_conv_forward_bf16(C.byref(geo), d_x, d_w, d_y, planes, None)
        assert rc == 0
        return to_nchw(dev.get(d_y, (shape[0], geo.out_h, geo.out_w, l0[1]))).reshape(-1)

    for k, mode, planes in ((2, "bf16x3", 3), (3, "fp32", 0)):
        net.train_set_precision(mode)
        w = net.train_pull(0, "weights").copy()
        x, y = T.inputs(spec, seed, k)
        net.train_step(x, y)
        assert net.train_pull(0, "x").tobytes() == layer0(x, w, planes).tobytes(), mode
        if k == 3:
            assert net.train_pull(0, "x").tobytes() != layer0(x, w, 1).tobytes()         # and not what bf16 operands give
    plain.free()
    net.free()


# ---- 6: downstream ----
def test_predict_save_and_batch_change_after_split_steps(tmp_path_factory, tmp_path):
    r = gpu_run("A", "bf16x3", tmp_path_factory.mktemp("splitA"))
    net, g, seed = r["net"], r["g"], r["seed"]
    x1, _ = T.inputs(T.NETS["A"], seed, 1)
    out = net.network_predict(x1)                       # inference mode: rolling statistics, folded batch norm
    print("A bf16x3: max|predict - reference's predict after its three steps| = %.3g" % np.abs(out - g["predict"]).max())
    assert np.abs(out - g["predict"]).max() < 1e-4       # the bound of test_predict_and_save_see_the_trained_weights
    for i, p in enumerate(r["params"]):
        if p is not None:
            host = np.ctypeslib.as_array(net.layer(i).weights, shape=(p["weights"].size,))
            assert np.array_equal(host, net.train_pull(i, "weights")) and not np.array_equal(host, p["weights"].reshape(-1))
    saved = str(tmp_path / "trained.weights")
    net.save_weights(saved)
    cfg, _, _ = T.materialize(str(tmp_path), "A", seed)
    fresh = darknet.Network.parse_network_cfg(cfg)
    fresh.load_weights(saved)
    assert fresh.train_precision() == "fp32"
    assert fresh.network_predict(x1).tobytes() == out.tobytes()
    assert fresh.net.seen[0] == net.net.seen[0] == T.STEPS * T.NETS["A"]["batch"]
    fresh.free()
    # the mode is the engine's: a batch change drops the trainer and keeps the mode, and the next step trains in it
    net.set_batch_network(T.NETS["A"]["batch"])
    assert net.train_precision() == "bf16x3"
    with pytest.raises(darknet.Y2Error, match="no trainer"):
        net.train_pull(0, "weights")
    before = np.ctypeslib.as_array(net.layer(0).weights, shape=(r["params"][0]["weights"].size,)).copy()
    net.train_step(*T.inputs(T.NETS["A"], seed, 2))
    assert net.train_precision() == "bf16x3" and not np.array_equal(net.train_pull(0, "weights"), before)
