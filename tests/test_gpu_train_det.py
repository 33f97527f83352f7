"""Detector training on the device against the compiled reference (tests/golden/train_E.npz, train_F.npz) under the rule of
tests/train_det_rule.py:

    err(A) = max|A - T64| / max|T64|,     a GPU tensor passes when  err(gpu) <= 4 * err(reference golden) + 4 * 2^-23

where T64 is the float64 run of the numpy rule.  Every tensor's two errors are printed before anything is asserted.  Nets
E (tiny-yolo shaped, prior branch on, two truths on one (cell, anchor), an empty image) and F (yolo.cfg's tail: route,
reorg, deltas with two writers, prior branch off) and G (yolo.2.0.cfg's tail: a reorg straight behind a route): every array after step 1 and the parameters / update buffers / losses
after the later steps through y2_train_pull, and the region statistics.  Then the region head called directly against the
rule at its edges, route and reorg on integer-valued data exactly, a step run twice gives the same bytes, and predict /
save / resize after training see the trained weights.

Bounds of the direct head test (no reference run exists for those inputs, so they come from the arithmetic): an element of
the output or the delta is at most 12 + classes fp32 roundings away from its inputs (a logistic, an exp or log, a few
products, the softmax's sum), and tx = truth.x*w - i carries the half-ulp of truth.x*w, 2^floor(log2(w)) * 2^-24, into a value
of order 1: head_bound = 2 * (12 + classes) * 2^floor(log2(max(w, h))) * 2^-24 relative to the tensor's largest value, the 2
for the last-bit errors of exp and log themselves (64 * 2^-23 on the 6x5 grid with 4 classes).  The cost adds a sum of n
squares in a fixed tree: + n * 2^-24.  The statistics are sums of such values kept in double on the device: they are held to
the step tests' floor, 4 * 2^-23.
"""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_det_rule as D
from tests import train_rule as T
from tests.helpers import load_golden
from tests.test_gpu_kernels import Dev, to_nchw, to_nhwc
from tests.test_train_det_host import DET_REFUSALS, det_refusal_net

pytestmark = pytest.mark.gpu


def head_bound(h, w, classes):
    return 2 * (12 + classes) * 2.0 ** int(np.floor(np.log2(max(w, h)))) * 2.0 ** -24


STAT_KEYS = ("avg_iou", "avg_class", "avg_obj", "avg_noobj", "recall")
_CACHE = {}


@pytest.fixture()
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


def golden_keys(g):
    out = []
    for key in sorted(g):
        if key.startswith("s") and "_l" in key and not key.endswith("_loss"):
            out.append((int(key[1]), int(key.split("_")[1][1:]), key.split("_", 2)[2], key))
    return out


def make_net(tmpdir, name, seed):
    cfg, wts, params = D.materialize(str(tmpdir), name, seed)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.net.seen[0] = D.NETS[name]["seen"]
    return net, params


def gpu_run(name, tmpdir):
    """three steps on the device; what the golden holds is pulled after each, with the statistics (once per session)"""
    if ("gpu", name) in _CACHE:
        return _CACHE[("gpu", name)]
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    net, params = make_net(tmpdir, name, seed)
    net.train_prepare()
    keys = golden_keys(g)
    got, losses, stats = {}, [], []
    for k in range(1, D.STEPS + 1):
        losses.append(net.train_step(*D.inputs(name, seed, k)))
        stats.append(net.train_region_stats())
        for (kk, i, a, key) in keys:
            if kk == k:
                got[key] = net.train_pull(i, a)
    res = dict(net=net, got=got, losses=losses, stats=stats, params=params, g=g, seed=seed, cost=net.get_network_cost())
    _CACHE[("gpu", name)] = res
    return res


def rule_run(name, seed):
    if ("rule", name) not in _CACHE:
        _CACHE[("rule", name)] = D.rule_snapshots(name, seed)
    return _CACHE[("rule", name)]


@pytest.mark.parametrize("name", ["E", "F", "G"])
def test_steps_against_the_reference(name, tmp_path_factory):
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    g = r["g"]
    _, snaps, losses, _ = rule_run(name, r["seed"])
    bad, worst = [], (0.0, "")
    for (k, i, a, key) in golden_keys(g):
        t64 = snaps[k - 1][i][a]
        e_ref, e_gpu = T.err(g[key], t64.reshape(-1)), T.err(r["got"][key], t64.reshape(-1))
        ratio = e_gpu / max(e_ref, T.BOUND_FLOOR / T.BOUND_FACTOR)
        print("%s %-24s err(reference) %.3e  err(gpu) %.3e  bound %.3e  ratio %.2f" % (name, key, e_ref, e_gpu, T.bound(e_ref), ratio))
        worst = max(worst, (ratio, key))
        if not e_gpu <= T.bound(e_ref):
            bad.append((key, e_ref, e_gpu))
    for k in range(1, D.STEPS + 1):
        t64 = losses[k - 1]
        e_ref, e_gpu = abs(float(g["s%d_loss" % k][0]) - t64) / abs(t64), abs(r["losses"][k - 1] - t64) / abs(t64)
        print("%s s%d_loss  reference %.7g  gpu %.7g  err(reference) %.3e  err(gpu) %.3e" % (name, k, float(g["s%d_loss" % k][0]), r["losses"][k - 1], e_ref, e_gpu))
        if not e_gpu <= T.bound(e_ref):
            bad.append(("s%d_loss" % k, e_ref, e_gpu))
    print("%s: largest err(gpu) / max(err(reference), 2^-23): %.2f at %s" % (name, worst[0], worst[1]))
    assert not bad, bad
    assert r["cost"] == r["losses"][-1]                   # get_network_cost: the one cost layer is the region head


@pytest.mark.parametrize("name", ["E", "F", "G"])
def test_region_statistics(name, tmp_path_factory):
    """the six figures the reference prints: the counts equal the rule's, the averages are within the floor of the bound
    (the reference's own values exist only as a printf and are not stored)"""
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    _, _, _, stats = rule_run(name, r["seed"])
    for k in range(D.STEPS):
        got, want = r["stats"][k], stats[k]
        assert got["count"] == want["count"] and got["class_count"] == want["class_count"]
        for key in STAT_KEYS:
            e = abs(got[key] - want[key])
            print("%s step %d %-10s rule %.9g  gpu %.9g  |difference| %.3e  bound %.3e" % (name, k + 1, key, want[key], got[key], e, T.bound(0) * abs(want[key])))
            assert e <= T.bound(0) * abs(want[key]), (key, got[key], want[key])


# ---- the region head, called directly ----
def head_truths(case, b, h, w, reg, rng):
    y = np.zeros((b, D.TRUTHS, 5), np.float32)

    def row(x, yy, cls):
        a = rng.randint(reg["num"])
        return (x, yy, reg["anchors"][2 * a] / w * rng.uniform(.7, 1.3), reg["anchors"][2 * a + 1] / h * rng.uniform(.7, 1.3), cls)

    def inside():
        return ((rng.randint(w) + rng.uniform(.1, .9)) / w, (rng.randint(h) + rng.uniform(.1, .9)) / h)

    if case == "grid1":
        y[0, 0] = row(.4, .6, 0)
    elif case == "few":
        for b in range(y.shape[0]):
            for t in range(3):
                y[b, t] = row(*inside(), rng.randint(reg["classes"]))
    elif case == "full30":
        for t in range(D.TRUTHS):                                           # no terminator
            y[0, t] = row(*inside(), rng.randint(reg["classes"]))
    else:
        under_one = float(np.nextafter(np.float32(1), np.float32(0)))
        y[0, 0] = row(under_one, inside()[1], 1)                            # x just under 1: cell w-1
        y[0, 1] = row(*inside(), 7)                                         # a class with no output: every class delta is 0 - p
        y[2, 0] = row(1.0, inside()[1], 0)                                  # x == 1.0: outside, skipped whole
        y[2, 1] = row(*inside(), 2)                                         # ... and the list goes on behind it
        y[2, 2] = row(inside()[0], 1.5, 0)                                  # y >= 1
        y[4, 0] = row(*inside(), 0)
        y[4, 1] = y[4, 0]                                                   # the same (cell, anchor) twice
        y[4, 1, 4] = 2
    return y


HEAD_CASES = {
    # name: (batch, h, w, anchors, classes, seen, options)
    "grid1_b1_prior": ("grid1", 1, 1, 1, (.8, .9), 1, 12799, dict(bias_match=1, rescore=1)),
    "full30_b1": ("full30", 1, 5, 6, (1.0, 1.25, 2.25, 2.0, 3.5, 3.0), 4, 12800, dict(bias_match=0, rescore=0)),
    # yolo-voc's head: 845 boxes per image, so an image spans four workgroups of the per-box pass
    "voc_grid_b2": ("few", 2, 13, 13, (1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071), 20, 12800,
                    dict(bias_match=1, rescore=1)),
    "edges_b5_prior": ("edges", 5, 3, 4, (1.0, 1.2, 2.2, 1.7), 3, 12799, dict(bias_match=1, rescore=1)),
    "edges_b5": ("edges", 5, 3, 4, (1.0, 1.2, 2.2, 1.7), 3, 12800, dict(bias_match=0, rescore=1)),
}


def head_inputs(name):
    """inputs of one case whose every decision keeps the 1e-4 margin in the float64 rule (the cell margin is waived for
    the edge cases: a truth sits ON an edge there, and that decision is taken in float by rule and device alike)"""
    case, b, h, w, anchors, classes, seen, opts = HEAD_CASES[name]
    reg = dict(num=len(anchors) // 2, classes=classes, anchors=anchors, softmax=1, object_scale=5, noobject_scale=1, class_scale=1,
               coord_scale=1, thresh=.6, **opts)
    for seed in range(50):
        rng = np.random.RandomState(1000 * len(name) + seed)
        x = (rng.randn(b, reg["num"] * (5 + classes), h, w) * .4).astype(np.float32)
        truth = head_truths(case, b, h, w, reg, rng).reshape(b, -1)
        m = {}
        want = D.region_train(x, truth, reg, seen, m)
        if all(m[k] >= T.KINK for k in ("thresh", "anchor", "recall")) and (case == "edges" or m["cell"] >= T.KINK):
            return reg, x, truth, seen, want
    raise AssertionError("no inputs keep the margins")


@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_region_head_against_the_rule(dev, name):
    reg, x, truth, seen, (out64, delta64, cost64, stats64) = head_inputs(name)
    b, c, h, w = x.shape
    L = dev.L
    g = darknet.TrainRegion(b, h, w, reg["num"], reg["classes"], reg["bias_match"], reg["rescore"], reg["thresh"], reg["coord_scale"],
                            reg["object_scale"], reg["noobject_scale"], reg["class_scale"])
    nbytes = L.y2h_train_region_scratch_bytes(C.byref(g))
    assert nbytes > 0
    d_out, d_delta, d_prev = dev.empty(x.nbytes), dev.empty(x.nbytes), dev.empty(x.nbytes)
    d_cost, d_stats = dev.empty(16), dev.empty(C.sizeof(darknet.RegionStats))
    assert L.y2h_train_region_loss(C.byref(g), dev.put(to_nhwc(x)), dev.put(np.array(reg["anchors"], np.float32)), dev.put(truth), seen,
                                   d_out, d_delta, d_prev, d_cost, d_stats, dev.empty(nbytes), None) == 0
    out = dev.get(d_out, (b, h, w, c))
    delta = dev.get(d_delta, (b, h, w, c))
    e_out, e_delta = T.err(out, out64.reshape(b, h, w, c)), T.err(to_nchw(delta), delta64)
    cost = float(dev.get(d_cost, 1)[0])
    e_cost = abs(cost - cost64) / cost64
    bound = head_bound(h, w, reg["classes"])
    print("%s: err(output) %.3e  err(delta) %.3e  bound %.3e;  cost rule %.9g gpu %.9g err %.3e" % (name, e_out, e_delta, bound, cost64, cost, e_cost))
    assert e_out <= bound and e_delta <= bound
    assert e_cost <= bound + x.size * 2.0 ** -24
    assert dev.get(d_prev, (b, h, w, c)).tobytes() == delta.tobytes()           # the axpy into a zeroed buffer
    st = darknet.RegionStats.from_buffer_copy(dev.get(d_stats, C.sizeof(darknet.RegionStats), np.uint8).tobytes())
    assert (st.count, st.class_count) == (stats64["count"], stats64["class_count"])
    for key in STAT_KEYS:
        got, want = getattr(st, key), stats64[key]
        print("%s: %-10s rule %.9g gpu %.9g" % (name, key, want, got))
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= T.bound(0) * abs(want)
    if name.startswith("edges"):
        t3 = truth.reshape(b, D.TRUTHS, 5)
        assert int(t3[0, 0, 0] * np.float32(w)) == w - 1 and stats64["count"] == 5   # of 7 truths, two lie outside
        # the skipped truths leave image 2 with the deltas of its one inside truth: the rule says the same (above), and the
        # row of the truth just under 1 is in cell w-1
        j = int(t3[0, 0, 1] * np.float32(h))
        assert np.abs(delta[0, j, w - 1].reshape(reg["num"], -1)[:, 5:]).max() > 0
    if name == "grid1_b1_prior":
        assert np.abs(delta[..., :4]).max() > 0
    if name == "voc_grid_b2":
        assert h * w * reg["num"] > 3 * 256 and stats64["count"] == 6
    if name == "full30_b1":
        assert stats64["count"] == 30


def test_region_head_with_no_truth_gives_nan_averages(dev):
    b, h, w, n, classes = 2, 3, 4, 2, 3
    x = (np.random.RandomState(3).randn(b, h, w, n * (5 + classes)) * .4).astype(np.float32)
    g = darknet.TrainRegion(b, h, w, n, classes, 1, 1, .6, 1, 5, 1, 1)
    L = dev.L
    d_stats, d_delta = dev.empty(C.sizeof(darknet.RegionStats)), dev.empty(x.nbytes)
    assert L.y2h_train_region_loss(C.byref(g), dev.put(x), dev.put(np.array((1, 1, 2, 2), np.float32)), dev.put(np.zeros((b, 150), np.float32)),
                                   12800, dev.empty(x.nbytes), d_delta, dev.empty(x.nbytes), dev.empty(16), d_stats,
                                   dev.empty(L.y2h_train_region_scratch_bytes(C.byref(g))), None) == 0
    st = darknet.RegionStats.from_buffer_copy(dev.get(d_stats, C.sizeof(darknet.RegionStats), np.uint8).tobytes())
    assert st.count == 0 and np.isnan(st.avg_iou) and np.isnan(st.recall) and np.isnan(st.avg_class) and 0 < st.avg_noobj < 1
    delta = dev.get(d_delta, (b, h, w, n, 5 + classes))
    assert np.abs(delta[..., 4]).max() > 0 and np.abs(delta[..., :4]).max() == 0 and np.abs(delta[..., 5:]).max() == 0
    assert L.y2h_train_region_loss(C.byref(g), None, None, None, 0, None, None, None, None, None, None, None) != 0


# ---- route and reorg, exactly ----
def small_ints(seed, shape, lo, hi):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


@pytest.mark.parametrize("chans", [(3, 5), (4, 1, 7)])
def test_route_forward_and_backward_exactly(dev, chans):
    b, h, w = 2, 3, 5
    L = dev.L
    total = sum(chans)
    srcs = [small_ints(10 + k, (b, h, w, c), -9, 9) for k, c in enumerate(chans)]
    d_out = dev.put(np.full((b, h, w, total), 77, np.float32))
    off = 0
    for s, c in zip(srcs, chans):
        assert L.y2h_train_route_forward(dev.put(s), c, d_out, total, off, b * h * w, None) == 0
        off += c
    want = np.concatenate(srcs, axis=3)
    assert np.array_equal(dev.get(d_out, want.shape), want)
    droute = small_ints(20, (b, h, w, total), -9, 9)
    d_droute = dev.put(droute)
    off = 0
    for k, c in enumerate(chans):
        had = small_ints(30 + k, (b, h, w, c), -9, 9)
        d_store, d_add = dev.put(had), dev.put(had)
        assert L.y2h_train_route_backward(d_droute, total, off, d_store, c, b * h * w, 0, None) == 0
        assert L.y2h_train_route_backward(d_droute, total, off, d_add, c, b * h * w, 1, None) == 0
        assert np.array_equal(dev.get(d_store, had.shape), droute[..., off:off + c])
        assert np.array_equal(dev.get(d_add, had.shape), had + droute[..., off:off + c])
        off += c
    assert L.y2h_train_route_forward(d_droute, 4, d_out, total, total - 3, b * h * w, None) != 0      # the slice must fit
    a, bb = small_ints(40, 1000, -9, 9), small_ints(41, 1000, -9, 9)
    d_a = dev.put(a)
    assert L.y2h_train_add(d_a, dev.put(bb), 1000, None) == 0
    assert np.array_equal(dev.get(d_a, 1000), a + bb)


@pytest.mark.parametrize("c,h,w", [(4, 4, 6), (8, 6, 4), (12, 2, 6)])
def test_reorg_backward_inverts_the_forward_exactly(dev, c, h, w):
    b, s = 3, 2
    L = dev.L
    x = (np.arange(b * c * h * w, dtype=np.float32) + 1).reshape(b, c, h, w)
    d_y, d_back = dev.empty(x.nbytes), dev.empty(x.nbytes)
    assert L.y2h_reorg(dev.put(to_nhwc(x)), c, d_y, c * s * s, b, h, w, c, s, 0, None) == 0
    y = to_nchw(dev.get(d_y, (b, h // s, w // s, c * s * s)))
    assert np.array_equal(y, D.reorg_forward(x, s))                                  # forward equals the rule
    assert L.y2h_train_reorg_backward(d_y, d_back, b, h, w, c, s, None) == 0
    assert to_nchw(dev.get(d_back, (b, h, w, c))).tobytes() == x.tobytes()           # backward of forward: the input bytes
    dy = small_ints(50, y.shape, -99, 99)
    d_dx = dev.put(np.full(x.shape, 55, np.float32))                                 # an assignment: what was there is gone
    assert L.y2h_train_reorg_backward(dev.put(to_nhwc(dy)), d_dx, b, h, w, c, s, None) == 0
    assert np.array_equal(to_nchw(dev.get(d_dx, (b, h, w, c))), D.reorg_backward(dy, s, c, h, w))
    assert L.y2h_train_reorg_backward(d_y, d_back, b, h, w + 1, c, s, None) != 0


# ---- whole steps ----
def all_arrays(net, spec):
    out = {}
    for i, l in enumerate(spec["layers"]):
        names = [a for a in T.CONV_ARRAYS if l[4] or a in ("output", "delta", "weights", "biases", "weight_updates", "bias_updates")] \
            if l[0] == "conv" else ["output", "delta"]
        for a in names:
            out[(i, a)] = net.train_pull(i, a)
    return out


def test_a_step_of_F_is_bit_identical_twice(tmp_path):
    g = load_golden("train_F")
    seed = int(g["seed"])
    runs = []
    for rep in range(2):
        net, _ = make_net(tmp_path, "F", seed)
        net.train_prepare()
        losses = [net.train_step(*D.inputs("F", seed, k)) for k in (1, 2)]
        runs.append((losses, all_arrays(net, D.NETS["F"]), net.train_region_stats()))
        net.free()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    for key, a in runs[0][1].items():
        assert a.tobytes() == runs[1][1][key].tobytes(), key


def test_predict_save_and_resize_see_the_trained_weights(tmp_path_factory, tmp_path):
    r = gpu_run("F", tmp_path_factory.mktemp("trainF"))
    net, g, seed = r["net"], r["g"], r["seed"]
    spec = D.NETS["F"]
    x1, _ = D.inputs("F", seed, 1)
    out = net.network_predict(x1)                       # inference mode: rolling statistics, folded batch norm
    print("F: max|predict - reference's predict after its three steps| = %.3g" % np.abs(out - g["predict"]).max())
    assert out.shape == g["predict"].shape and np.abs(out - g["predict"]).max() < 1e-4      # the bound of test_gpu_train.py
    saved = str(tmp_path / "trained.weights")
    net.save_weights(saved)
    cfg, _, params = D.materialize(str(tmp_path), "F", seed)
    fresh = darknet.Network.parse_network_cfg(cfg)
    fresh.load_weights(saved)
    assert fresh.network_predict(x1).tobytes() == out.tobytes()
    assert fresh.net.seen[0] == net.net.seen[0] == spec["seen"] + D.STEPS * spec["batch"]
    for i, p in enumerate(params):
        if p is not None:
            n = p["weights"].size
            a = np.ctypeslib.as_array(fresh.layer(i).weights, shape=(n,))
            assert np.array_equal(a, net.train_pull(i, "weights")) and not np.array_equal(a, p["weights"].reshape(-1))
            assert np.array_equal(np.ctypeslib.as_array(fresh.layer(i).biases, shape=(p["biases"].size,)), net.train_pull(i, "biases"))
    fresh.free()
    # train_detector's multi-scale loop: resize, then keep stepping; the trainer is rebuilt with the trained weights
    before = net.train_pull(10, "weights").copy()
    net.resize_network(24, 16)
    with pytest.raises(darknet.Y2Error, match="no trainer"):
        net.train_pull(10, "weights")
    rng = np.random.RandomState(9)
    x = rng.uniform(-1, 1, (spec["batch"], 3, 16, 24)).astype(np.float32)
    loss = net.train_step(x, D.truths("F", 1))
    assert np.isfinite(loss) and loss > 0
    after = net.train_pull(10, "weights")
    assert net.layer(12).w == 6 and net.layer(12).h == 4 and net.train_pull(12, "delta").size == spec["batch"] * 16 * 24
    assert not np.array_equal(after, before) and np.abs(after - before).max() < .1       # one step on from the trained weights
    assert net.train_region_stats()["count"] == 3


@pytest.mark.parametrize("what", sorted(DET_REFUSALS))
def test_new_refusals_on_the_device_machine(tmp_path, what):
    net, pattern = det_refusal_net(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    net.free()
