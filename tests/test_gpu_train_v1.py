"""YOLOv1 training on the device against the compiled reference (tests/golden/train_H.npz, train_I.npz) under the rule of
tests/train_v1_rule.py and the bound of tests/train_rule.py:

    err(A) = max|A - T64| / max|T64|,     a GPU tensor passes when  err(gpu) <= 4 * err(reference golden) + 4 * 2^-23

where T64 is the float64 run of the numpy rule.  Every tensor's two errors are printed before anything is asserted.  Nets H
(tiny-yolo-v1 in small: the dense layer behind a 6x6x6 image) and I (the yolo-small head in small: a batch-normalised dense
layer over 3 rows, [dropout], softmax / forced head, two subdivisions): every array after step 1 and the parameters / update
buffers / losses after the later steps through y2_train_pull, srand(step) before each step as the reference driver calls
it; I's dropout draws must EQUAL the reference's.  Then the head's statistics, a step run twice gives the same bytes,
predict / save / load after training see the trained weights, and the [detection] head called directly against the rule.

Bound of the direct head test (no reference run exists for those inputs, so it comes from the arithmetic).  Relative to the
tensor's largest value, which the test asserts to be >= 1 (coord_scale = 5 on coordinate differences of several tenths):
  * a class delta is the per-cell softmax (an exp, the sum's `classes` additions, a division, the two subtractions of the
    maximum) and a subtraction and a product behind it: at most classes + 8 roundings of values <= 1;
  * a coordinate delta is a subtraction and a product, with sqrt one more: at most 3;
  * the object delta carries the IoU: x/side, y/side and (sqrt=1) w*w, h*h are one rounding each, an edge x +- w/2 two more,
    so an overlap (right - left, all values <= 1.5 in size) is within 4 * 2^-24 * 1.5, the intersection within 9 and the
    union (two products, a sum, a difference) within 12 units of 2^-24 * 1.5; iou = inter / union is then within
    (9 + 12 + 1) * 1.5 * 2^-24 / union of the exact value.  The boxes of these cases are between .5 and .9 wide and high, so
    union >= .25: 132 * 2^-24, and two roundings behind it.
  det_bound = (134 + classes + 8) * 2^-24.  The output is the input or the softmax: the same bound holds.
The cost is a sum of N squares in a fixed tree: its relative error is at most 2 * sqrt(N) * det_bound (Cauchy-Schwarz over
the elements' errors) + N * 2^-24.  The statistics are sums kept in double on the device: held to the step tests' floor.
"""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_rule as T
from tests import train_v1_rule as V
from tests.helpers import load_golden
from tests.test_gpu_kernels import Dev

pytestmark = pytest.mark.gpu

STAT_KEYS = ("avg_iou", "avg_cat", "avg_allcat", "avg_obj", "avg_anyobj")
_CACHE = {}


def det_bound(classes):
    return (134 + classes + 8) * 2.0 ** -24


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
    cfg, wts, params = V.materialize(str(tmpdir), name, seed)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    return net, params


def step(net, name, seed, k):
    V.libc().srand(k)                      # the [dropout] layers draw libc rand(): the reference driver seeds it the same way
    return net.train_step(*V.inputs(name, seed, k))


def gpu_run(name, tmpdir):
    if ("gpu", name) in _CACHE:
        return _CACHE[("gpu", name)]
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    net, params = make_net(tmpdir, name, seed)
    net.train_prepare()
    keys = golden_keys(g)
    got, losses, stats = {}, [], []
    for k in range(1, V.STEPS + 1):
        losses.append(step(net, name, seed, k))
        stats.append(net.train_detection_stats())
        for (kk, i, a, key) in keys:
            if kk == k:
                got[key] = net.train_pull(i, a)
    res = dict(net=net, got=got, losses=losses, stats=stats, params=params, g=g, seed=seed, cost=net.get_network_cost())
    _CACHE[("gpu", name)] = res
    return res


def rule_run(name, seed):
    if ("rule", name) not in _CACHE:
        _CACHE[("rule", name)] = V.rule_snapshots(name, seed)
    return _CACHE[("rule", name)]


@pytest.mark.parametrize("name", ["H", "I"])
def test_steps_against_the_reference(name, tmp_path_factory):
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    g = r["g"]
    _, snaps, losses, _ = rule_run(name, r["seed"])
    bad, worst = [], (0.0, "")
    for (k, i, a, key) in golden_keys(g):
        t64 = snaps[k - 1][i][a]
        if a == "rand":
            print("%s %-24s equal to the reference's: %s" % (name, key, np.array_equal(r["got"][key], g[key])))
            if not np.array_equal(r["got"][key], g[key]):
                bad.append((key, "the draws differ"))
            continue
        e_ref, e_gpu = T.err(g[key], t64.reshape(-1)), T.err(r["got"][key], t64.reshape(-1))
        ratio = e_gpu / max(e_ref, T.BOUND_FLOOR / T.BOUND_FACTOR)
        print("%s %-24s err(reference) %.3e  err(gpu) %.3e  bound %.3e  ratio %.2f" % (name, key, e_ref, e_gpu, T.bound(e_ref), ratio))
        worst = max(worst, (ratio, key))
        if not e_gpu <= T.bound(e_ref):
            bad.append((key, e_ref, e_gpu))
    for k in range(1, V.STEPS + 1):
        t64 = losses[k - 1]
        e_ref, e_gpu = abs(float(g["s%d_loss" % k][0]) - t64) / abs(t64), abs(r["losses"][k - 1] - t64) / abs(t64)
        print("%s s%d_loss  reference %.7g  gpu %.7g  err(reference) %.3e  err(gpu) %.3e" % (name, k, float(g["s%d_loss" % k][0]), r["losses"][k - 1], e_ref, e_gpu))
        if not e_gpu <= T.bound(e_ref):
            bad.append(("s%d_loss" % k, e_ref, e_gpu))
    print("%s: largest err(gpu) / max(err(reference), 2^-23): %.2f at %s" % (name, worst[0], worst[1]))
    assert not bad, bad
    assert r["cost"] == r["losses"][-1]                   # get_network_cost: the one cost is the head's
    if name == "I":
        assert any(a == "rand" for (_, _, a, _) in golden_keys(g))
    assert not r["net"].layer(0).delta and not r["net"].layer(r["net"].n - 1).delta       # layer.delta stays NULL


@pytest.mark.parametrize("name", ["H", "I"])
def test_detection_statistics(name, tmp_path_factory):
    """the six figures the reference prints: the count equals the rule's, the averages are within the floor of the bound"""
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    _, _, _, stats = rule_run(name, r["seed"])
    for k in range(V.STEPS):
        got, want = r["stats"][k], stats[k]
        assert got["count"] == want["count"] > 0
        for key in STAT_KEYS:
            e = abs(got[key] - want[key])
            print("%s step %d %-10s rule %.9g  gpu %.9g  |difference| %.3e  bound %.3e" % (name, k + 1, key, want[key], got[key], e, T.bound(0) * abs(want[key])))
            assert e <= T.bound(0) * abs(want[key]), (key, got[key], want[key])


def all_arrays(net, spec):
    out = {}
    for i, l in enumerate(spec["layers"]):
        if l[0] == "dropout":
            names = ["rand"]
        elif l[0] in ("conv", "connected"):
            bn = l[4] if l[0] == "conv" else l[2]
            names = [a for a in T.CONV_ARRAYS if bn or a in ("output", "delta", "weights", "biases", "weight_updates", "bias_updates")]
        else:
            names = ["output", "delta"]
        for a in names:
            out[(i, a)] = net.train_pull(i, a)
    return out


@pytest.mark.parametrize("name", ["H", "I"])
def test_a_step_is_bit_identical_twice(name, tmp_path):
    g = load_golden("train_" + name)
    seed = int(g["seed"])
    runs = []
    for rep in range(2):
        net, _ = make_net(tmp_path, name, seed)
        net.train_prepare()
        losses = [step(net, name, seed, k) for k in (1, 2)]
        runs.append((losses, all_arrays(net, V.NETS[name]), net.train_detection_stats()))
        net.free()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    for key, a in runs[0][1].items():
        assert a.tobytes() == runs[1][1][key].tobytes(), key


@pytest.mark.parametrize("name", ["H", "I"])
def test_predict_and_save_see_the_trained_weights(name, tmp_path_factory, tmp_path):
    r = gpu_run(name, tmp_path_factory.mktemp("train" + name))
    net, g, seed = r["net"], r["g"], r["seed"]
    x1, _ = V.inputs(name, seed, 1)
    out = net.network_predict(x1)                       # inference mode: rolling statistics, no dropout
    print("%s: max|predict - reference's predict after its three steps| = %.3g" % (name, np.abs(out - g["predict"]).max()))
    assert out.shape == g["predict"].shape and np.abs(out - g["predict"]).max() < 1e-4      # the bound of test_gpu_train_det.py
    saved = str(tmp_path / "trained.weights")
    net.save_weights(saved)
    cfg, _, params = V.materialize(str(tmp_path), name, seed)
    fresh = darknet.Network.parse_network_cfg(cfg)
    fresh.load_weights(saved)
    assert fresh.network_predict(x1).tobytes() == out.tobytes()
    for i, p in enumerate(params):
        if p is not None:                               # the dense layers' weights included: [outputs][inputs], CHW input order
            a = np.ctypeslib.as_array(fresh.layer(i).weights, shape=(p["weights"].size,))
            assert np.array_equal(a, net.train_pull(i, "weights")) and not np.array_equal(a, p["weights"].reshape(-1))
            assert np.array_equal(np.ctypeslib.as_array(fresh.layer(i).biases, shape=(p["biases"].size,)), net.train_pull(i, "biases"))
    fresh.free()


# ---- the [detection] head, called directly ----
HEAD_CASES = {
    # name: (batch, side, n, classes, options, fraction of object cells)
    "side1_n1": (2, 1, 1, 2, dict(softmax=0, sqrt=0, rescore=0), 1.0),
    "n3_softmax_sqrt_rescore": (2, 2, 3, 4, dict(softmax=1, sqrt=1, rescore=1), .6),
    "classes1": (2, 3, 2, 1, dict(softmax=1, sqrt=0, rescore=1), .6),
    # tiny-yolo-v1's head: 245 cells, four workgroups of the per-cell pass
    "side7_b5": (5, 7, 2, 20, dict(softmax=0, sqrt=1, rescore=1), .5),
    "forced": (3, 3, 2, 3, dict(softmax=1, sqrt=0, rescore=0, forced=1), .6),
    "empty": (2, 3, 2, 3, dict(softmax=0, sqrt=1, rescore=1), 0.0),
}


def head_inputs(name):
    """inputs of one case whose every decision keeps the 1e-4 margin in the float64 rule; boxes .5 to .9 wide and high"""
    b, side, n, classes, opts, frac = HEAD_CASES[name]
    det = dict(classes=classes, coords=4, side=side, num=n, object_scale=1, noobject_scale=.5, class_scale=1, coord_scale=5, **opts)
    cells = side * side
    for seed in range(50):
        rng = np.random.RandomState(1000 * len(name) + seed)
        size = rng.uniform(.5, .9, (b, cells * n, 2))
        boxes = np.concatenate([rng.uniform(.2, .8, (b, cells * n, 2)), np.sqrt(size) if opts.get("sqrt") else size], axis=2)
        x = np.concatenate([rng.uniform(.1, .9, (b, cells * (classes + n))), boxes.reshape(b, -1)], axis=1).astype(np.float32)
        truth = np.zeros((b, cells, 1 + classes + 4), np.float32)
        obj = rng.uniform(size=(b, cells)) < frac
        truth[..., 0] = obj
        truth[np.arange(b)[:, None], np.arange(cells)[None, :], 1 + rng.randint(classes, size=(b, cells))] = 1
        truth[..., 1 + classes:1 + classes + 2] = rng.uniform(.1, .9, (b, cells, 2))
        truth[..., 1 + classes + 2:] = rng.uniform(.5, .9, (b, cells, 2))
        if opts.get("forced"):
            truth[0, 0, 1 + classes + 2:] = (.2, .3)               # truth.w * truth.h < .1: box 1
            truth[0, 0, 0] = 1
        m = {}
        want = V.detection_train(x, truth, det, m)
        if all(m.get(k, np.inf) >= T.KINK for k in ("iou_gap", "iou_zero", "rmse", "forced")):
            return det, x, truth.reshape(b, -1), want
    raise AssertionError("no inputs keep the margins")


def run_head(dev, det, x, truth, add=0, prev=None):
    L = dev.L
    b = x.shape[0]
    g = darknet.TrainDetection(b, det["side"], det["num"], det["classes"], det.get("softmax", 0), det.get("sqrt", 0), det.get("rescore", 0),
                               det.get("forced", 0), det["coord_scale"], det["object_scale"], det["noobject_scale"], det["class_scale"])
    nbytes = L.y2h_train_detection_scratch_bytes(C.byref(g))
    assert nbytes > 0
    d_out, d_delta = dev.put(np.full(x.shape, np.nan, np.float32)), dev.put(np.full(x.shape, np.nan, np.float32))     # no memset is needed
    d_prev = dev.put(prev) if prev is not None else dev.empty(x.nbytes)
    d_cost, d_stats = dev.empty(16), dev.empty(C.sizeof(darknet.DetectionStats))
    assert L.y2h_train_detection_loss(C.byref(g), dev.put(x), dev.put(truth), d_out, d_delta, d_prev, add, d_cost, d_stats,
                                      dev.empty(nbytes), None) == 0
    st = darknet.DetectionStats.from_buffer_copy(dev.get(d_stats, C.sizeof(darknet.DetectionStats), np.uint8).tobytes())
    return dev.get(d_out, x.shape), dev.get(d_delta, x.shape), dev.get(d_prev, x.shape), float(dev.get(d_cost, 1)[0]), st


@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_detection_head_against_the_rule(dev, name):
    det, x, truth, (out64, delta64, cost64, stats64) = head_inputs(name)
    out, delta, prev, cost, st = run_head(dev, det, x, truth)
    e_out, e_delta = T.err(out, out64), T.err(delta, delta64)
    e_cost = abs(cost - cost64) / cost64
    bound = det_bound(det["classes"])
    cost_bound = 2 * np.sqrt(x.size) * bound + x.size * 2.0 ** -24
    print("%s: err(output) %.3e  err(delta) %.3e  bound %.3e;  cost rule %.9g gpu %.9g err %.3e bound %.3e" % (
        name, e_out, e_delta, bound, cost64, cost, e_cost, cost_bound))
    assert np.abs(delta64).max() >= 1 or name == "empty"          # what the bound's derivation leans on
    assert e_out <= bound and e_delta <= bound
    assert e_cost <= cost_bound
    assert prev.tobytes() == delta.tobytes()                       # the axpy into a zeroed buffer: a store
    assert st.count == stats64["count"]
    for key in STAT_KEYS:
        got, want = getattr(st, key), stats64[key]
        print("%s: %-10s rule %.9g gpu %.9g" % (name, key, want, got))
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= T.bound(0) * abs(want)
    if name == "empty":
        cells, cl, n = det["side"] ** 2, det["classes"], det["num"]
        assert st.count == 0 and all(np.isnan(getattr(st, k)) for k in STAT_KEYS[:4]) and 0 < st.avg_anyobj < 1
        assert np.abs(delta[:, :cells * cl]).max() == 0 and np.abs(delta[:, cells * (cl + n):]).max() == 0
        assert np.abs(delta[:, cells * cl:cells * (cl + n)]).min() > 0
    if name == "side7_b5":
        assert x.shape[0] * det["side"] ** 2 > 3 * 64 and st.count > 64
    if name == "forced":
        assert stats64["count"] > 1


def test_detection_head_adds_to_a_delta_already_written(dev):
    det, x, truth, _ = head_inputs("classes1")
    _, delta, _, _, _ = run_head(dev, det, x, truth)
    had = np.random.RandomState(4).randint(-3, 4, x.shape).astype(np.float32)
    _, delta2, prev, _, _ = run_head(dev, det, x, truth, add=1, prev=had)
    assert delta2.tobytes() == delta.tobytes() and np.array_equal(prev, had + delta)


def test_cells_where_the_reference_leaves_its_arrays_are_skipped(dev):
    """no box wins (every rmse >= 20: the reference goes on with box -1, the cell in front's), and forced names box 1 of a
    one-box head (the reference writes behind the image): the cell keeps its no-object and class deltas, nothing else"""
    for opts, far in ((dict(softmax=0, sqrt=0, rescore=1), 100.), (dict(softmax=0, sqrt=0, rescore=0, forced=1), .5)):
        det = dict(classes=2, coords=4, side=2, num=1, object_scale=1, noobject_scale=.5, class_scale=1, coord_scale=5, **opts)
        x = np.full((1, 4 * (2 + 1 + 4)), .5, np.float32)
        x[0, 4 * 3 + 3 * 4] = far                                   # the last cell's box: x = 100 (rmse 33), or left alone
        truth = np.zeros((1, 4, 7), np.float32)
        truth[0, :, 0] = 1
        truth[0, :, 1] = 1
        truth[0, :, 3:] = (.5, .5, .6, .6)
        truth[0, 3, 5:] = (.2, .3)                                  # forced: .06 < .1 -> box 1 of 1
        out64, delta64, cost64, stats64 = V.detection_train(x, truth, det)
        out, delta, _, cost, st = run_head(dev, det, x, truth.reshape(1, -1))
        assert st.count == stats64["count"] == 3
        assert T.err(delta, delta64) <= det_bound(2) and abs(cost - cost64) / cost64 <= 1e-5
        assert np.all(delta[0, 4 * 3 + 3 * 4:] == 0)                # the last cell: no coordinate delta,
        assert delta[0, 4 * 2 + 3] == np.float32(.5) * (0 - x[0, 4 * 2 + 3])          # the no-object delta,
        assert np.abs(delta[0, 6:8]).max() > 0                      # and its class deltas


def test_detection_head_refuses_bad_arguments(dev):
    L = dev.L
    g = darknet.TrainDetection(0, 3, 2, 3, 0, 0, 0, 0, 5, 1, .5, 1)
    assert L.y2h_train_detection_scratch_bytes(C.byref(g)) == 0
    g = darknet.TrainDetection(1, 3, 2, 3, 0, 0, 0, 0, 5, 1, .5, 1)
    assert L.y2h_train_detection_loss(C.byref(g), None, None, None, None, None, 0, None, None, None, None) != 0
