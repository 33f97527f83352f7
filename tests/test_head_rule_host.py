"""CPU-only checks of the detection head's rule (tests/head_rule.py): it reproduces the compiled reference bit for bit
on the networks of the committed goldens -- the region forward from the layer below, get_region_boxes /
get_detection_boxes at two thresholds with and without only_objectness, the Detector's compaction -- and every case the
GPU test of the head kernels runs (tests/test_gpu_head_kernels.py) keeps the generator's margins: no class score within
1e-3 of its threshold, no hierarchy probability within 1e-3 of .5, something kept and something dropped everywhere.

thresh = 0 has no margin to keep (softmax scores crowd against zero by nature): there the decision is `score > 0`, which
moves only where a score underflows.  Inputs in +-4 keep every exponent above -8 and the +-1e4 rows give exact zeros on
any exp, so the check at thresh 0 is that every non-zero score is a normal float."""
import numpy as np
import pytest

from sr_object_detection_amd import zoo
from tests import head_rule as R
from tests import hier_rule as H
from tests.helpers import load_golden, materialize

F = np.float32
GOLDENS = {"mini_32_b2": "mini", "mini_mfma_64_b2": "mini-mfma", "yolo9000_96_b1": "yolo9000", "yolo9000_96_b1_map": "yolo9000",
           "mini_v1_32_b2": "mini-v1"}


def golden_net(oracle, workdir, name):
    g = load_golden(name)
    size, batch = int(g["size"]), int(g["batch"])
    cfg, wts, x = materialize(workdir, GOLDENS[name], size, batch, int(g["seed"]), float(g["head_gain"]), use_map=bool(g["use_map"]))
    head = [l for l in zoo.resolve(GOLDENS[name], size) if l["type"] in ("region", "detection")][-1]
    return oracle.OracleNet(cfg, wts), x, head, float(g["thresh"]), bool(g["use_map"])


@pytest.mark.parametrize("name", [n for n in GOLDENS if GOLDENS[n] != "mini-v1"])
def test_rule_reproduces_the_reference_region_head(oracle, workdir, name):
    on, x, head, thresh, use_map = golden_net(oracle, workdir, name)
    tree = H.tree("NINE_K") if GOLDENS[name] == "yolo9000" else None
    cmap = R.tree_map("NINE_K") if use_map else None
    num, classes = head["num"], head["classes"]
    on.predict(x)
    below, info = on.layer_info(on.last - 1), on.layer_info(on.last)
    assert (info["n"], info["classes"]) == (num, classes)
    w, h = info["w"], info["h"]
    prev = on.layer_output(on.last - 1).reshape(on.batch, below["out_c"], h, w)
    prev = np.ascontiguousarray(prev.transpose(0, 2, 3, 1)).reshape(on.batch * h * w, -1)             # NHWC
    out = on.layer_output(on.last).reshape(-1, 5 + classes)
    pred = R.region_forward(prev, num, classes, 1, tree)
    assert np.array_equal(pred, out)                                          # forward_region_layer
    if tree is not None:                                                      # the numpy softmax IS the oracle's
        assert np.array_equal(R.softmax_tree_np(prev.reshape(-1, 5 + classes)[:4, 5:], tree, False), out[:4, 5:])
    else:
        assert np.array_equal(np.stack([R.softmax_np(r) for r in prev.reshape(-1, 5 + classes)[:, 5:]]), out[:, 5:])
    total = w * h * num
    kept = dropped = 0
    for th in (thresh, 0.05):
        for oo in (0, 1):
            for img in ((1, 1), (640, 480)):
                boxes, probs, _ = R.region_boxes(pred, w, h, num, classes, head["anchors"], img, th, oo, 0, tree, cmap)
                for b in range(on.batch):
                    if tree is not None:
                        on.predict(x)                                         # the reference edits its output in place
                    ob, op = on.region_boxes(b, th, img[0], img[1], oo, int(use_map))
                    mine = probs[b * total:(b + 1) * total]
                    assert np.array_equal(boxes[b * total:(b + 1) * total], ob)
                    assert np.array_equal(mine, op)
                    kept += int((mine > 0).sum())
                    dropped += int((mine == 0).sum())
                    if img == (1, 1):
                        rec, cnt = R.collect(ob, op, 1, th, total)
                        want = oracle.detector_bboxes(ob, op, th, 640, 480)
                        assert cnt[0] == len(want)
                        r = rec[0, :cnt[0]]
                        assert np.array_equal(r[:, 4], want["prob"]) and np.array_equal(r[:, 5].astype(np.uint32), want["obj_id"])
                        bx = r[:, :4].astype(np.float64)
                        assert np.array_equal(np.maximum(0, (bx[:, 0] - bx[:, 2] / 2.) * 640).astype(np.uint32), want["x"])
                        assert np.array_equal((r[:, 2] * F(640)).astype(np.uint32), want["w"])
    assert kept and dropped
    on.close()


def test_rule_reproduces_the_reference_yolov1_decode(oracle, workdir):
    on, x, head, thresh, _ = golden_net(oracle, workdir, "mini_v1_32_b2")
    on.predict(x)
    out = on.layer_output(on.last).reshape(on.batch, -1)
    side, num, classes = head["side"], head["num"], head["classes"]
    total = side * side * num
    for th in (thresh, 0.05):
        for oo in (0, 1):
            for (w, h) in ((1, 1), (640, 480)):
                boxes, probs = R.detection_boxes(out, side, num, classes, head["sqrt"], w, h, th, oo)
                for b in range(on.batch):
                    ob, op = on.detection_boxes(b, th, w, h, oo)
                    assert np.array_equal(boxes[b * total:(b + 1) * total], ob)
                    assert np.array_equal(probs[b * total:(b + 1) * total], op)
                    rec, cnt = R.collect(ob, op, 1, th, total)
                    want = oracle.detector_bboxes(ob, op, th, 1, 1)
                    assert cnt[0] == len(want) and np.array_equal(rec[0, :cnt[0], 4], want["prob"])
                    assert np.array_equal(rec[0, :cnt[0], 5].astype(np.uint32), want["obj_id"])
    on.close()


def test_collect_keeps_the_first_maximum_and_counts_past_the_cap():
    probs = np.array([[0, .5, .5], [0, 0, 0], [.9, .1, .9], [.3, 0, 0]], F)
    boxes = np.arange(16, dtype=F).reshape(4, 4)
    rec, cnt = R.collect(boxes, probs, 1, 0.2, 2, fill=-7)
    assert cnt.tolist() == [3]
    assert rec[0].tolist() == [[0, 1, 2, 3, .5, 1], [8, 9, 10, 11, F(.9), 0]]
    rec, cnt = R.collect(np.concatenate([boxes, boxes]), np.concatenate([probs, probs[::-1]]), 2, 0.2, 4, fill=-7)
    assert cnt.tolist() == [3, 3] and rec[1, 0].tolist() == [0, 1, 2, 3, F(.3), 0] and (rec[:, 3] == -7).all()


# ---- the cases -------------------------------------------------------------------------------------------------------
def check_margin(scores, thresh, what):
    nz = scores[scores != 0].astype(np.float64)
    if nz.size == 0:
        return
    if thresh > 0:
        assert np.abs(nz - thresh).min() >= R.MARGIN, what
    else:
        assert nz.min() >= np.finfo(F).tiny, what


def test_region_cases_take_the_kernels_they_name():
    by = {c.ident: c for c in R.REGION}
    assert len(by) == len(R.REGION)
    for c in R.REGION:
        assert c.ldx >= c.num * (5 + c.classes)
        assert c.lds_kernel == (c.classes < 250), c.ident
    edge = [c for c in R.REGION if c.classes == 249][0]
    assert (64 * (5 + edge.classes) + 128) * 4 == 64 * 1024                   # exactly 64 KB
    assert [c.boxes for c in R.REGION if c.classes == 250] == [70, 70]
    assert {c.boxes % 64 for c in R.REGION} >= {1, 22, 6}                     # partial last workgroups
    for c in R.REGION:                                                        # the overwritten rows do what they say
        out = R.region_forward(R.region_input(c), c.num, c.classes, c.softmax)
        sp = R.special_boxes(c.boxes)
        assert np.isfinite(out).all()
        if c.softmax:
            assert np.all(out[sp["equal"], 5:] == out[sp["equal"], 5]) and np.allclose(out[:, 5:].sum(1), 1, atol=1e-5)
        if "alt" in sp:
            assert out[sp["obj_hi"], 4] == 1 and out[sp["obj_lo"], 4] == 0 and out[sp["negzero"], 4] == 0.5
            if c.softmax:
                assert set(out[sp["alt"], 5:].tolist()) == {0.0, float(F(1) / F((c.classes + 1) // 2))}


@pytest.mark.parametrize("name", R.TREES)
def test_tree_cases_keep_their_margins(oracle, name):
    t = R.tree(name)
    assert R.tree_lds_ok(t.n) == (t.n <= 16383)
    pred = R.tree_pred(name)
    assert pred.shape == (R.TREE_BOXES, 5 + t.n)
    val, cls, hp = R.tree_best(pred[:, 5:], t)
    assert np.abs(hp.astype(np.float64) - .5).min() >= R.MARGIN               # no hierarchy probability near .5
    assert (val == 0).any(), "a box with no class above .5"
    assert (t.depth[cls[val > 0]] >= min(2, int(t.depth.max()))).any(), "a kept class deeper than level 1"
    scale = pred[:, 4].astype(np.float64)
    assert np.abs(scale - 0.24).min() >= R.MARGIN and np.abs(scale - .5).min() >= R.MARGIN
    for th in R.THRESHES:
        for cf in (0, -1):
            _, probs, edited = R.region_boxes(pred, R.TREE_W, R.TREE_H, R.TREE_NUM, t.n, R.ANCHORS, (1, 1), th, 0, cf, t)
            assert (probs > 0).any() and ((probs == 0).all(axis=1) & (val > 0)).any() == (th > 0 or cf == -1), (th, cf)
            assert ((edited[:, 5:] != 0).sum(axis=1) <= 1).all()
    if t.parents_first:                                                       # the level walk is the same products
        assert np.array_equal(hp, H.hierarchy_predictions(pred[:, 5:], t))
    else:
        assert not np.array_equal(hp, np.stack([[H.get_hierarchy_probability(r, t, c) for c in range(t.n)] for r in pred[:, 5:]]))
    if name in R.MAP_TREES:
        cmap = R.tree_map(name)
        assert len(cmap) == 200 and max(cmap) < t.n
        for th in R.THRESHES:
            _, probs, _ = R.region_boxes(pred, R.TREE_W, R.TREE_H, R.TREE_NUM, t.n, R.ANCHORS, (1, 1), th, 0, 0, t, cmap, fill=-7)
            assert (probs[:, 200:] == -7).all()
            check_margin(probs[:, :200], th, name)
            assert (probs[:, :200] > 0).any() and ((probs[:, :200] == 0).any() or th == 0)


def test_tree_softmax_in_numpy_is_the_oracles(oracle):
    for name in ("MINI", "WIDE", "MANY"):
        t = R.tree(name)
        rows = R.tree_logits(name).reshape(-1, 5 + t.n)[:, 5:]
        assert np.array_equal(R.softmax_tree_np(rows, t, False), H.softmax_tree(rows, t))


def test_fast_exp_distance():
    """D: the rule with a float32 exp against the rule with the double exp, over the tree cases"""
    d = R.fast_exp_distance()
    print("FAST_EXP: D = %.3g" % d)
    # a float32 exp within an ulp moves every term by <= 1.2e-7 relative, the sum by no more, the quotient (<= 1) by the two
    # together and one more rounding
    assert 0 < d <= 3e-7


@pytest.mark.parametrize("c", R.DECODE, ids=[c.ident for c in R.DECODE])
def test_decode_cases_keep_their_margins(oracle, c):
    pred = R.decode_pred(c)
    assert pred.shape == (c.batch * c.total, 5 + c.classes)
    assert c.chain_ok == (c.classes <= 256)
    assert (c.batch * c.total * c.classes > (1 << 20)) == (c == R.DECODE[-1])
    opts = R.decode_options(c)
    if c == R.FULL_CROSS:
        assert len(opts) == 64
    for field in range(6):
        assert len({o[field] for o in opts}) == 2, (c.ident, field)           # both values of every option
    seen, most = set(), 0
    for o in opts:
        key = (o.classfix, o.only_objectness, o.thresh)
        if key in seen:
            continue
        seen.add(key)
        _, probs, _ = R.region_boxes(pred, c.w, c.h, c.num, c.classes, R.ANCHORS, o.img, o.thresh, o.only_objectness, o.classfix)
        check_margin(probs, o.thresh, (c.ident, o.ident))
        if c.total > 1:
            assert (probs > 0).any() and ((probs == 0).any() or (o.thresh == 0 and o.classfix == 0)), (c.ident, o.ident)
        _, cnt = R.collect(np.zeros((len(probs), 4), F), probs, c.batch, o.thresh, 3)
        most = max(most, int(cnt.max()))
        if o.thresh > 0 and c.total > 1:
            assert 0 < cnt.max() < c.total, (c.ident, o.ident)               # a box passes, and not every box
    assert most > 3 or c.total <= 3                                          # max_per_image = 3 cuts
    scale = pred[:, 4].astype(np.float64)
    assert np.abs(scale - .5).min() >= 1e-4 or c.total > 1000                 # classfix = -1 decides at .5


def test_best_class_rows_repeat_their_maximum():
    for classes in R.BEST_CLASS:
        p = R.best_class_rows(classes)
        cls = R.max_index(p)
        assert not p[1].any() and not p[6].any() and cls[1] == 0 and cls[6] == 0
        if classes > 1:
            reps = [(p[r] == p[r].max()).sum() for r in (0, 2, 3, 4, 5, 7)]
            assert max(reps) == 2 and all(p[r, cls[r]] == F(0.75) for r in (0, 2, 3, 4, 5, 7))
            assert all(cls[r] == np.nonzero(p[r] == F(0.75))[0][0] for r in (0, 2, 3, 4, 5, 7))


NMS_COUNTS = {"t4096-c2-k0.5": 2020, "t3000-c3-k0.5-ties": 1500, "t8200-c2-k0.8": 1600, "t16384-c2-k0.5": 8200}


@pytest.mark.parametrize("c", R.NMS_SORT, ids=[c.ident for c in R.NMS_SORT])
def test_nms_cases_reach_the_forms_they_name(oracle, c):
    boxes, probs = R.nms_case(c.total, c.classes, c.seed, c.keep, c.eighths)
    per_class = (probs != 0).sum(axis=0)
    assert np.all(np.abs(per_class - NMS_COUNTS[c.ident]) < 0.08 * NMS_COUNTS[c.ident]), per_class
    assert per_class.min() > 1024                                            # the global-memory loop
    cap = 1 << (c.total - 1).bit_length()
    assert (cap > 8192) == (c.total > 8192) and c.total <= R.NMS_SORT_MAX
    if c.eighths:
        _, runs = np.unique(probs[:, 1][probs[:, 1] != 0], return_counts=True)
        assert runs.max() >= 100
    post = oracle.do_nms_sort(boxes, probs, 0.4)
    assert 0 < (post != 0).sum() < (probs != 0).sum()


def test_v1_cases():
    for c in R.V1_CASES:
        for stride in (c.outputs, c.outputs + 5):
            p = R.v1_pred(c, stride)
            for oo in (0, 1):
                boxes, probs = R.detection_boxes(p, c.side, c.num, c.classes, c.sqrt, 640, 480, R.V1_THRESH, oo)
                assert boxes.shape == (c.batch * c.side * c.side * c.num, 4) and np.isfinite(boxes).all() and np.abs(boxes).max() < 1000
                check_margin(probs[:, 1:] if oo else probs, R.V1_THRESH, c.ident)
                if c.side > 1:
                    assert (probs > 0).any() and (probs == 0).any()
