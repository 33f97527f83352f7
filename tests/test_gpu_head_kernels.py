"""GPU tests of the detection head kernel by kernel, by direct calls of the C-ABI: the region forward of plain and tree
heads in every form (region_lds_kernel, region_kernel in both softmax modes, region_tree_lds_kernel<false/true> with and
without the `best` by-product, region_tree_kernel), the decode of plain and tree heads (level walk, sequential walk with
and without a map), NMS in its LDS, global-memory and lds_boxes = 0 forms, the class-agnostic NMS, the compaction, the
three-launch chain of plain heads, the two-launch chain of tree heads, and the YOLOv1 decode -- against the rule of
tests/head_rule.py (pinned to the compiled reference by tests/test_head_rule_host.py), whose cases these are.

What counts as equal.  Two device forms of one computation: array_equal.  Device against the rule where the value is a
copy or pure fp32 arithmetic (coords, scale * p, thresholds, classes, counts, record order): array_equal.  Behind a double
exp / logistic in [0, 1]: SOFTMAX_BAR.  Box terms: two fp32 spacings of the rule's value (the device's exp and glibc's are
each within an ulp, two or three correctly rounded operations follow); the largest distance seen is printed.  NMS and
compaction: always on the arrays pulled from the device's own decode, so array_equal without a margin.

Y2H_REGION_FAST_EXP (test_region_tree_fast_exp): D = 2.38e-07 is the distance of the rule with a float32 exp from the rule
with the double exp over these cases (tests/test_head_rule_host.py prints it); the device's fast form must stay within
2 * D + SOFTMAX_BAR = 5.97e-07 of the rule.  Measured on the device: 1.79e-07 at worst (the 16383-node tree)."""
import ctypes as C

import numpy as np
import pytest

from tests import head_rule as R
from tests import hier_rule as H
from tests.test_gpu_hier import SOFTMAX_BAR
from tests.test_gpu_kernels import Dev

pytestmark = pytest.mark.gpu

F = np.float32
SWITCHES = ("Y2_REGION_TREE_SIMPLE", "Y2_REGION_EXP_DOUBLE", "Y2_NO_TREE_BEST", "Y2_DTS_THREADS", "Y2_DETECT_SEPARATE")
EINVAL = -2
FAST_EXP = 1
GUARD, FILL = 64, -7


class y2h_decode(C.Structure):
    """include/y2_hip.h"""
    _fields_ = [("batch", C.c_int), ("w", C.c_int), ("h", C.c_int), ("num", C.c_int), ("classes", C.c_int), ("img_w", C.c_int),
                ("img_h", C.c_int), ("thresh", C.c_float), ("only_objectness", C.c_int), ("classfix", C.c_int),
                ("anchors", C.c_void_p), ("tree_parent", C.c_void_p), ("tree_order", C.c_void_p), ("tree_level_off", C.c_void_p),
                ("tree_levels", C.c_int), ("map", C.c_void_p), ("pred", C.c_void_p), ("boxes", C.c_void_p), ("probs", C.c_void_p)]


def bind(L):
    vp, i, f, ln, q = C.c_void_p, C.c_int, C.c_float, C.c_long, C.POINTER(y2h_decode)
    L.y2h_region_forward.argtypes = [vp, i, vp, i, i, i, i, i, i, i, vp, vp, vp]
    L.y2h_region_forward_tree.argtypes = [vp, i, vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, i, vp, i, vp]
    L.y2h_region_tree_best_ok.argtypes = [i, i]
    L.y2h_region_boxes.argtypes = [q, vp]
    L.y2h_nms_sort.argtypes = [vp, vp, vp, i, i, i, i, f, vp, vp]
    L.y2h_nms.argtypes = [vp, vp, i, i, i, i, f, vp]
    L.y2h_collect.argtypes = [vp, vp, i, i, i, i, f, vp, vp, i, vp, vp]
    L.y2h_detect_chain_ok.argtypes = [q]
    L.y2h_detect_chain.argtypes = [q, f, vp, vp, vp, vp, i, vp, vp]
    L.y2h_detect_tree_chain_ok.argtypes = [q]
    L.y2h_detect_tree_chain.argtypes = [q, f, vp, vp, i, vp, vp, vp]
    L.y2h_detection_boxes.argtypes = [vp, ln, i, i, i, i, i, i, i, f, i, vp, vp, vp]
    L.y2h_softmax_rows.argtypes = [vp, vp, ln, i, f, vp]
    return L


@pytest.fixture()
def dev(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    d = Dev()
    bind(d.L)
    d.L.y2h_set_device(0)
    yield d
    d.close()


class Out:
    """an output buffer with a guard tail: data and tail pre-filled with -7 (`init`: the data part holds that instead)"""

    def __init__(self, dev, shape, dtype=F, init=None):
        self.dev, self.shape, self.dtype = dev, tuple(np.atleast_1d(shape)), dtype
        self.size = int(np.prod(self.shape))
        host = np.full(self.size + GUARD, FILL, dtype)
        if init is not None:
            host[:self.size] = np.asarray(init, dtype).reshape(-1)
        self.p = dev.put(host)

    def at(self, elements):
        return C.c_void_p(self.p.value + elements * np.dtype(self.dtype).itemsize)

    def pull(self):
        a = self.dev.get(self.p, (self.size + GUARD,), self.dtype)
        assert (a[self.size:] == FILL).all(), "guard tail written"
        return a[:self.size].reshape(self.shape)


def at(p, floats):
    return C.c_void_p(p.value + 4 * floats)


def ulps(got, want):
    """the distance in fp32 spacings of the rule's value"""
    want = np.asarray(want, F)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


def check_boxes(got, want, what):
    u = ulps(got, want)
    print("%s: box terms within %.2f fp32 spacings of the rule" % (what, u))
    assert u <= 2, what


# =====================================================================================================================
# A. region forward, plain heads
# =====================================================================================================================
@pytest.mark.parametrize("c", R.REGION, ids=[c.ident for c in R.REGION])
def test_region_forward_plain(dev, oracle, c):
    """region_lds_kernel up to 249 classes, region_kernel (softmax modes 1 and 0) from 250"""
    L = dev.L
    size = 5 + c.classes
    x = R.region_input(c)
    dx = dev.put(x)
    y = Out(dev, (c.boxes, size))
    assert L.y2h_region_forward(dx, c.ldx, y.p, c.batch, c.hw, c.num, c.classes, 4, c.softmax, 0, None, None, None) == 0
    got = y.pull()
    rule = R.region_forward(x, c.num, c.classes, c.softmax)
    assert np.array_equal(got[:, :4], rule[:, :4])
    assert np.abs(got[:, 4] - rule[:, 4]).max() <= SOFTMAX_BAR
    sp = R.special_boxes(c.boxes)
    if "alt" in sp:
        assert got[sp["obj_hi"], 4] == 1 and got[sp["obj_lo"], 4] == 0 and got[sp["negzero"], 4] == 0.5
    if not c.softmax:
        assert np.array_equal(got[:, 5:], rule[:, 5:])
        return
    ref = Out(dev, (c.boxes, c.classes))                          # y2h_softmax_rows on the same device slices
    for i in range(c.boxes):
        assert L.y2h_softmax_rows(at(dx, (i // c.num) * c.ldx + (i % c.num) * size + 5), ref.at(i * c.classes), 1, c.classes, 1.0, None) == 0
    assert np.array_equal(got[:, 5:], ref.pull())
    err = float(np.abs(got[:, 5:] - rule[:, 5:]).max())
    print("%s: max |kernel - rule| = %.3g" % (c.ident, err))
    assert err <= SOFTMAX_BAR
    assert np.all(got[sp["equal"], 5:] == got[sp["equal"], 5])


def test_region_forward_refuses_bad_arguments(dev):
    L = dev.L
    dx = dev.put(np.zeros(64, F))
    y = Out(dev, (64,))
    for args in ((dx, 12, y.p, 0, 1, 2, 1, 4, 1), (dx, 12, y.p, 1, 0, 2, 1, 4, 1), (dx, 12, y.p, 1, 1, 2, 0, 4, 1),
                 (dx, 12, y.p, 1, 1, 2, 1, 3, 1), (dx, 11, y.p, 1, 1, 2, 1, 4, 1)):
        assert L.y2h_region_forward(*args, 0, None, None, None) == EINVAL
    assert (y.pull() == FILL).all()


# =====================================================================================================================
# B. region forward, tree heads
# =====================================================================================================================
class TreeDev:
    """a tree's tables on the device"""

    def __init__(self, dev, t):
        self.t = t
        self.gs, self.go, self.par = dev.put(t.group_size), dev.put(t.group_offset), dev.put(t.parent)
        self.order = self.off = None
        self.levels = 0
        if t.parents_first:
            order, off = t.levels()
            self.order, self.off, self.levels = dev.put(order), dev.put(off), len(off) - 1


def forward_tree(dev, td, dx, flags=0, best=False, expect=0):
    """y2h_region_forward_tree on TREE_BATCH x (TREE_W * TREE_H) cells of TREE_NUM boxes -> (y, best val, best cls)"""
    t = td.t
    boxes = R.TREE_BOXES
    y = Out(dev, (boxes, 5 + t.n))
    b = Out(dev, (2 * boxes,)) if best else None
    rc = dev.L.y2h_region_forward_tree(dx, R.TREE_NUM * (5 + t.n), y.p, R.TREE_BATCH, R.TREE_W * R.TREE_H, R.TREE_NUM, t.n, 4, t.groups,
                                       td.gs, td.go, td.par, td.order, td.off, td.levels, b.p if best else None, flags, None)
    assert rc == expect, rc
    if rc != 0:
        assert (y.pull() == FILL).all()
        return None, None, None
    got = y.pull()
    if not best:
        return got, None, None
    raw = b.pull()
    return got, raw[:boxes].copy(), raw[boxes:].view(np.int32).copy()


def depth_bar(t, cls, per_factor):
    """a product of depth + 1 factors <= 1, each within `per_factor` of the rule's, and as many roundings of <= 6e-8"""
    return (t.depth[cls].astype(np.float64) + 1) * (per_factor + 6e-8)


@pytest.mark.parametrize("name", R.TREES)
def test_region_forward_tree(dev, oracle, monkeypatch, name):
    """region_tree_lds_kernel<false> up to 16383 classes, region_tree_kernel from 16384 (N16384, BIG) and under
    Y2_REGION_TREE_SIMPLE; <false> again under FAST_EXP with Y2_REGION_EXP_DOUBLE; the `best` by-product and its refusals"""
    L = dev.L
    t = R.tree(name)
    td = TreeDev(dev, t)
    x = R.tree_logits(name)
    dx = dev.put(x)
    size = 5 + t.n
    rule = R.tree_pred(name)
    y0, _, _ = forward_tree(dev, td, dx)
    assert np.array_equal(y0[:, :4], rule[:, :4])
    assert np.abs(y0[:, 4] - rule[:, 4]).max() <= SOFTMAX_BAR
    err = float(np.abs(y0[:, 5:] - rule[:, 5:]).max())
    print("%s: max |kernel - rule| = %.3g" % (name, err))
    assert err <= SOFTMAX_BAR
    # the device-side reference: the tree softmax of tests/test_gpu_hier.py (held there to y2h_softmax_rows group by group)
    gof = dev.put(t.group)
    ref = Out(dev, (R.TREE_BOXES, t.n))
    for i in range(R.TREE_BOXES):
        assert L.y2h_softmax_tree_rows(at(dx, i * size + 5), ref.at(i * t.n), 1, t.n, 1.0, t.groups, td.gs, td.go, gof, None) == 0
    assert np.array_equal(y0[:, 5:], ref.pull())
    monkeypatch.setenv("Y2_REGION_TREE_SIMPLE", "1")
    simple, _, _ = forward_tree(dev, td, dx)
    assert np.array_equal(simple, y0)
    monkeypatch.delenv("Y2_REGION_TREE_SIMPLE")
    monkeypatch.setenv("Y2_REGION_EXP_DOUBLE", "1")
    forced, _, _ = forward_tree(dev, td, dx, flags=FAST_EXP)
    assert np.array_equal(forced, y0)
    monkeypatch.delenv("Y2_REGION_EXP_DOUBLE")
    # the `best` by-product
    assert L.y2h_region_tree_best_ok(t.n, max(td.levels, 1)) == int(R.tree_lds_ok(t.n))
    assert L.y2h_region_tree_best_ok(t.n, 0) == 0
    if not t.parents_first or not R.tree_lds_ok(t.n):
        forward_tree(dev, td, dx, best=True, expect=EINVAL)       # BACK: no level order; BIG, N16384: no LDS row
        return
    val, cls, _ = R.tree_best(rule[:, 5:], t)
    yb, bval, bcls = forward_tree(dev, td, dx, best=True)
    assert np.array_equal(yb, y0)
    assert np.array_equal(bcls, cls)
    assert np.all(np.abs(bval.astype(np.float64) - val) <= depth_bar(t, cls, SOFTMAX_BAR)) and np.array_equal(bval == 0, val == 0)
    monkeypatch.setenv("Y2_NO_TREE_BEST", "1")
    assert L.y2h_region_tree_best_ok(t.n, td.levels) == 0
    forward_tree(dev, td, dx, best=True, expect=EINVAL)


@pytest.mark.parametrize("name", [n for n in R.TREES if n != "BACK"])
def test_region_tree_fast_exp(dev, oracle, name):
    """region_tree_lds_kernel<true>.  D = 2.38e-07 (the rule with a float32 exp against the rule with the double exp, over
    these cases); the bound is 2 * D + SOFTMAX_BAR = 5.97e-07.  Measured on the device: 1.79e-07 on the 16383-node tree,
    1.19e-07 on MINI, MANY and the yolo9000 tree, 1.9e-09 on WIDE; BIG and the 16384-node tree run region_tree_kernel, which
    has the double form only (0)."""
    t = R.tree(name)
    td = TreeDev(dev, t)
    dx = dev.put(R.tree_logits(name))
    rule = R.tree_pred(name)
    bar = 2 * R.fast_exp_distance() + SOFTMAX_BAR
    y0, _, _ = forward_tree(dev, td, dx)
    yf, _, _ = forward_tree(dev, td, dx, flags=FAST_EXP)
    assert np.array_equal(yf[:, :5], y0[:, :5])
    err = float(np.abs(yf[:, 5:].astype(np.float64) - rule[:, 5:]).max())
    print("%s: FAST_EXP max |kernel - rule| = %.3g (bound %.3g, D = %.3g)" % (name, err, bar, R.fast_exp_distance()))
    assert err <= bar
    if not R.tree_lds_ok(t.n):
        assert np.array_equal(yf, y0)                                  # region_tree_kernel has one form
        return
    assert not np.array_equal(yf, y0)                                  # the fast form did run
    val, cls, _ = R.tree_best(rule[:, 5:], t)
    yb, bval, bcls = forward_tree(dev, td, dx, flags=FAST_EXP, best=True)
    assert np.array_equal(yb, yf)
    assert np.array_equal(bcls, cls)
    assert np.all(np.abs(bval.astype(np.float64) - val) <= depth_bar(t, cls, bar)) and np.array_equal(bval == 0, val == 0)


def test_region_tree_sums_run_in_index_order(dev, monkeypatch):
    """a group whose terms span 1 .. 2^-30 in descending order, and a group of 1 followed by 4096 terms below half an ulp
    of 1: added in index order the small terms are lost one by one (sum 1, the first output exactly 1); the same groups
    reversed add the small terms up first (sum 1.0001).  Both forms of the LDS kernel and the global-memory kernel."""
    L = dev.L
    t = H.Tree([-1] * 31 + [0] * 4097)
    assert t.group_size.tolist() == [31, 4097]
    down = np.concatenate([-np.arange(31) * np.log(2), [0], np.full(4096, -17.5)]).astype(F)
    up = np.concatenate([down[:31][::-1], down[31:][::-1]])
    size = 5 + t.n
    x = np.zeros((1, 2 * size), F)
    x[0, 5:size], x[0, size + 5:] = down, up
    gs, go, par = dev.put(t.group_size), dev.put(t.group_offset), dev.put(t.parent)
    dx = dev.put(x)
    outs = {}
    for form, flags, env in (("double", 0, None), ("fast", FAST_EXP, None), ("global", 0, "Y2_REGION_TREE_SIMPLE")):
        y = Out(dev, (2, size))
        if env:
            monkeypatch.setenv(env, "1")
        assert L.y2h_region_forward_tree(dx, 2 * size, y.p, 1, 1, 2, t.n, 4, t.groups, gs, go, par, None, None, 0, None, flags, None) == 0
        if env:
            monkeypatch.delenv(env)
        got = y.pull()[:, 5:]
        outs[form] = got
        rule = R.softmax_tree_np(np.stack([down, up]), t, form == "fast")
        assert rule[0, 31] == 1 and rule[1, -1] < 0.99995
        assert got[0, 31] == 1 and got[1, -1] < 0.99995, form
        assert np.abs(got.astype(np.float64) - rule).max() <= (2 * R.fast_exp_distance() if form == "fast" else 0) + SOFTMAX_BAR, form
    assert np.array_equal(outs["global"], outs["double"])


# =====================================================================================================================
# C. decode, plain heads
# =====================================================================================================================
def decode_struct(dev, batch, w, h, num, classes, o, dpred, boxes, probs, td=None, order=True, cmap=None, anchors=None):
    q = y2h_decode()
    q.batch, q.w, q.h, q.num, q.classes = batch, w, h, num, classes
    q.img_w, q.img_h = o.img
    q.thresh, q.only_objectness, q.classfix = o.thresh, o.only_objectness, o.classfix
    q.anchors = (anchors if anchors is not None else dev.put(R.ANCHORS[:2 * num])).value
    if td is not None:
        q.tree_parent = td.par.value
        if order and td.order is not None:
            q.tree_order, q.tree_level_off, q.tree_levels = td.order.value, td.off.value, td.levels
    q.map = cmap.value if cmap is not None else None
    q.pred = dpred.value
    q.boxes = boxes.p.value if boxes is not None else None
    q.probs = probs.p.value if probs is not None else None
    return q


def dense_chain(dev, oracle, q, nb, total, classes, o, max_per, check_oracle=True):
    """y2h_region_boxes (done by the caller into q.boxes / q.probs, pulled here) + y2h_nms_sort + y2h_collect, each held to
    the oracle / the rule on the arrays pulled from the device -> (final probs on the device, records, counts)"""
    L = dev.L
    batch = nb // total
    n = nb * classes
    dboxes, dprobs = C.c_void_p(q.boxes), C.c_void_p(q.probs)
    boxes = dev.get(dboxes, (nb, 4))
    probs = dev.get(dprobs, (nb, classes))
    final, dfinal, nms_out = probs, dprobs, None
    if o.nms > 0:
        nms_out = Out(dev, (nb, classes))
        assert L.y2h_memcpy_d2d(nms_out.p, dprobs, n * 4, None) == 0
        cc = Out(dev, (batch * classes,), np.int32)
        assert L.y2h_nms_sort(dboxes, dprobs, nms_out.p, batch, total, classes, classes, o.nms, cc.p, None) == 0
        final, dfinal = nms_out.pull(), nms_out.p
        cc.pull()
        if check_oracle:
            for b in range(batch):
                s = slice(b * total, (b + 1) * total)
                assert np.array_equal(final[s], oracle.do_nms_sort(boxes[s], probs[s], o.nms)), "image %d" % b
        assert np.array_equal(dev.get(dprobs, (nb, classes)), probs)              # the input scores are not written
    rec, cnt, scratch = Out(dev, (batch, max_per, 6)), Out(dev, (batch,), np.int32), Out(dev, (2 * nb,))
    assert L.y2h_collect(dboxes, dfinal, batch, total, classes, classes, o.thresh, rec.p, cnt.p, max_per, scratch.p, None) == 0
    records, counts = rec.pull(), cnt.pull()
    scratch.pull()
    want_rec, want_cnt = R.collect(boxes, final, batch, o.thresh, max_per, fill=FILL)
    assert np.array_equal(counts, want_cnt) and np.array_equal(records, want_rec)
    return boxes, probs, final, records, counts


DECODE_PARAMS = [pytest.param(c, o, id=c.ident + "-" + o.ident) for c in R.DECODE for o in R.decode_options(c)]


@pytest.mark.parametrize("c,o", DECODE_PARAMS)
def test_decode_plain(dev, oracle, c, o):
    """decode_boxes_kernel + decode_probs_kernel, nms_sort_kernel (LDS form), best_class_kernel + collect_kernel, and the
    chain: decode_all_kernel, nms_sort_kernel with the count reset, best_collect_kernel (vec4 where classes % 4 == 0, scalar
    otherwise) or, past 2^20 scores, best_class_kernel + collect_kernel"""
    L = dev.L
    nb, total = c.batch * c.total, c.total
    max_per = total if o.max_all else 3
    pred = R.decode_pred(c)
    dpred = dev.put(pred)
    boxes, probs = Out(dev, (nb, 4)), Out(dev, (nb, c.classes))
    q = decode_struct(dev, c.batch, c.w, c.h, c.num, c.classes, o, dpred, boxes, probs)
    assert L.y2h_region_boxes(C.byref(q), None) == 0
    rb, rp, _ = R.region_boxes(pred, c.w, c.h, c.num, c.classes, R.ANCHORS, o.img, o.thresh, o.only_objectness, o.classfix)
    assert np.array_equal(probs.pull(), rp)
    check_boxes(boxes.pull(), rb, c.ident)
    assert np.array_equal(dev.get(dpred, pred.shape), pred)                       # a plain head's rows are not edited
    b1, p1, f1, rec1, cnt1 = dense_chain(dev, oracle, q, nb, total, c.classes, o, max_per)
    assert L.y2h_detect_chain_ok(C.byref(q)) == int(c.chain_ok)
    boxes2, probs2, nms2 = Out(dev, (nb, 4)), Out(dev, (nb, c.classes)), Out(dev, (nb, c.classes))
    cc = Out(dev, (c.batch * c.classes,), np.int32, init=0)
    rec, cnt, scratch = Out(dev, (c.batch, max_per, 6)), Out(dev, (c.batch,), np.int32), Out(dev, (2 * nb,))
    q2 = decode_struct(dev, c.batch, c.w, c.h, c.num, c.classes, o, dpred, boxes2, probs2)
    if not c.chain_ok:
        assert L.y2h_detect_chain(C.byref(q2), o.nms, nms2.p, cc.p, rec.p, cnt.p, max_per, scratch.p, None) == EINVAL
        assert (boxes2.pull() == FILL).all() and (rec.pull() == FILL).all()
        return
    for frame in range(3):                                                        # the same buffers, frame after frame
        assert L.y2h_detect_chain(C.byref(q2), o.nms, nms2.p, cc.p, rec.p, cnt.p, max_per, scratch.p, None) == 0
        assert np.array_equal(boxes2.pull(), b1) and np.array_equal(probs2.pull(), p1), frame
        if o.nms > 0:
            assert np.array_equal(nms2.pull(), f1), frame
        else:
            assert (nms2.pull() == FILL).all()
        assert np.array_equal(cnt.pull(), cnt1) and np.array_equal(rec.pull(), rec1), frame
        assert not cc.pull().any(), frame                                         # class_counts are zero again
        scratch.pull()


@pytest.mark.parametrize("stride_pad", [0, 3])
@pytest.mark.parametrize("classes", R.BEST_CLASS)
def test_best_class_kernel(dev, classes, stride_pad):
    """one wavefront per box: fewer classes than lanes, one pass, one more than a pass, two passes and a rest; a repeated
    maximum (the first one wins) and all-zero rows (class 0, score 0)"""
    L = dev.L
    p = R.best_class_rows(classes)
    stride = classes + stride_pad
    padded = np.full((8, stride), 0.99, F)
    padded[:, :classes] = p
    boxes = np.arange(32, dtype=F).reshape(8, 4)
    rec, cnt, scratch = Out(dev, (2, 4, 6)), Out(dev, (2,), np.int32), Out(dev, (16,))
    assert L.y2h_collect(dev.put(boxes), dev.put(padded), 2, 4, classes, stride, 0.2, rec.p, cnt.p, 4, scratch.p, None) == 0
    raw = scratch.pull()
    cls = R.max_index(p)
    assert np.array_equal(raw[8:].view(np.int32), cls) and np.array_equal(raw[:8], p[np.arange(8), cls])
    want_rec, want_cnt = R.collect(boxes, p, 2, 0.2, 4, fill=FILL)
    assert np.array_equal(cnt.pull(), want_cnt) and np.array_equal(rec.pull(), want_rec)


def test_chain_limits(dev):
    """y2h_detect_chain_ok: 256 classes and 16384 boxes per image; y2h_detect_tree_chain_ok: 4096 boxes, a 150 KB row"""
    L = dev.L
    o = R.SUBSET[0]
    d = dev.put(np.zeros(4, F))
    box = Out(dev, (4,))
    for classes, w, num, ok in ((256, 128, 128, 1), (257, 128, 128, 0), (256, 16385, 1, 0), (1, 16384, 1, 1)):
        q = decode_struct(dev, 1, w, 1, num, classes, o, d, box, box, anchors=d)
        assert L.y2h_detect_chain_ok(C.byref(q)) == ok, (classes, w, num)
    td = TreeDev(dev, R.tree("MINI"))
    for classes, w, num, ok in ((38400, 1, 1, 1), (38401, 1, 1, 0), (24, 1024, 4, 1), (24, 241, 17, 0)):
        q = decode_struct(dev, 1, w, 1, num, classes, o, d, box, box, td=td, anchors=d)
        assert L.y2h_detect_tree_chain_ok(C.byref(q)) == ok, (classes, w, num)
    q = decode_struct(dev, 1, 1, 1, 1, 24, o._replace(only_objectness=1), d, box, box, td=td, anchors=d)
    assert L.y2h_detect_tree_chain_ok(C.byref(q)) == 0
    q = decode_struct(dev, 1, 1, 1, 1, 24, o, d, box, box, td=td, order=False, anchors=d)
    assert L.y2h_detect_tree_chain_ok(C.byref(q)) == 0
    assert (box.pull() == FILL).all()


# =====================================================================================================================
# D. decode, tree heads
# =====================================================================================================================
TREE_OPTS = [R.Opt((1, 1), 0, 0, 0.24, 0.4, True), R.Opt((640, 480), -1, 0, 0.0, 0.0, True), R.Opt((1, 1), 0, 1, 0.24, 0.4, True)]


def tree_boxes(dev, td, pred, o, order, cmap=None):
    """y2h_region_boxes on a fresh copy of pred -> (boxes, probs, the edited pred)"""
    n = td.t.n
    dpred = Out(dev, pred.shape, init=pred)
    boxes, probs = Out(dev, (len(pred), 4)), Out(dev, (len(pred), n))
    q = decode_struct(dev, R.TREE_BATCH, R.TREE_W, R.TREE_H, R.TREE_NUM, n, o, dpred.p, boxes, probs, td=td, order=order, cmap=cmap)
    assert dev.L.y2h_region_boxes(C.byref(q), None) == 0
    return boxes.pull(), probs.pull(), dpred.pull()


@pytest.mark.parametrize("name", R.TREES)
def test_decode_tree(dev, oracle, name):
    """decode_tree_kernel (level walk) and decode_boxes_kernel's sequential walk, without and with a map: each against the
    rule, the two against each other; BACK has the sequential walk only"""
    t = R.tree(name)
    td = TreeDev(dev, t)
    pred = R.tree_pred(name)
    for o in TREE_OPTS:
        rb, rp, redit = R.region_boxes(pred, R.TREE_W, R.TREE_H, R.TREE_NUM, t.n, R.ANCHORS, o.img, o.thresh, o.only_objectness,
                                       o.classfix, t)
        seq = tree_boxes(dev, td, pred, o, order=False)
        check_boxes(seq[0], rb, name)
        assert np.array_equal(seq[1], rp) and np.array_equal(seq[2], redit), o.ident
        if t.parents_first:
            lev = tree_boxes(dev, td, pred, o, order=True)
            assert all(np.array_equal(a, b) for a, b in zip(lev, seq)), o.ident
    if name in R.MAP_TREES:
        cmap = dev.put(np.asarray(R.tree_map(name), np.int32))
        for o in TREE_OPTS:
            rb, rp, redit = R.region_boxes(pred, R.TREE_W, R.TREE_H, R.TREE_NUM, t.n, R.ANCHORS, o.img, o.thresh, o.only_objectness,
                                           o.classfix, t, R.tree_map(name), fill=FILL)
            seq = tree_boxes(dev, td, pred, o, order=False, cmap=cmap)
            lev = tree_boxes(dev, td, pred, o, order=True, cmap=cmap)
            assert np.array_equal(seq[1], rp) and np.array_equal(seq[2], redit), o.ident
            assert all(np.array_equal(a, b) for a, b in zip(lev, seq)), o.ident


def tree_chain(dev, td, dpred, batch, w, h, num, o, max_per, best=None, expect=0):
    nb = batch * w * h * num
    boxes = Out(dev, (nb, 4))
    rec, cnt, scratch = Out(dev, (batch, max_per, 6)), Out(dev, (batch,), np.int32), Out(dev, (2 * nb,))
    q = decode_struct(dev, batch, w, h, num, td.t.n, o, dpred, boxes, None, td=td)
    rc = dev.L.y2h_detect_tree_chain(C.byref(q), o.nms, rec.p, cnt.p, max_per, scratch.p, best, None)
    assert rc == expect, rc
    scratch.pull()
    return boxes.pull(), rec.pull(), cnt.pull()


def dense_tree(dev, oracle, td, pred, batch, w, h, num, o, max_per):
    nb, n = len(pred), td.t.n
    dpred = Out(dev, pred.shape, init=pred)
    boxes, probs = Out(dev, (nb, 4)), Out(dev, (nb, n))
    q = decode_struct(dev, batch, w, h, num, n, o, dpred.p, boxes, probs, td=td)
    assert dev.L.y2h_region_boxes(C.byref(q), None) == 0
    boxes.pull(), probs.pull()
    b, _, _, rec, cnt = dense_chain(dev, oracle, q, nb, w * h * num, n, o, max_per)
    return b, rec, cnt


@pytest.mark.parametrize("name", [n for n in R.TREES if n != "BACK"])
def test_detect_tree_chain(dev, oracle, monkeypatch, name):
    """decode_tree_sparse_kernel at 512 and 256 threads, decode_tree_cand_kernel on the region layer's `best`, and
    nms_collect_sparse_kernel, against y2h_region_boxes + y2h_nms_sort + y2h_collect on the device"""
    t = R.tree(name)
    td = TreeDev(dev, t)
    rule = R.tree_pred(name)
    dx = dev.put(R.tree_logits(name))
    y_dev = best = None
    if R.tree_lds_ok(t.n):                                                        # the device's own region output, with `best`
        y = Out(dev, rule.shape)
        best = Out(dev, (2 * R.TREE_BOXES,))
        assert dev.L.y2h_region_forward_tree(dx, R.TREE_NUM * (5 + t.n), y.p, R.TREE_BATCH, R.TREE_W * R.TREE_H, R.TREE_NUM, t.n, 4, t.groups,
                                             td.gs, td.go, td.par, td.order, td.off, td.levels, best.p, 0, None) == 0
        y_dev = y.pull()
    shape = (R.TREE_BATCH, R.TREE_W, R.TREE_H, R.TREE_NUM)
    seen = 0
    for nms in (0.0, 0.4, 1e-6):
        for max_per in (R.TREE_W * R.TREE_H * R.TREE_NUM, 1):
            o = R.Opt((1, 1), 0, 0, 0.24, nms, True)
            want = dense_tree(dev, oracle, td, rule, *shape, o, max_per)
            seen = max(seen, int(want[2].max()))
            dpred = Out(dev, rule.shape, init=rule)
            got = tree_chain(dev, td, dpred.p, *shape, o, max_per)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (nms, max_per)
            assert np.array_equal(dpred.pull(), rule)                            # the chain does not edit the rows
            monkeypatch.setenv("Y2_DTS_THREADS", "256")
            got = tree_chain(dev, td, dpred.p, *shape, o, max_per)
            monkeypatch.delenv("Y2_DTS_THREADS")
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (nms, max_per, 256)
            if y_dev is not None:
                want = dense_tree(dev, oracle, td, y_dev, *shape, o, max_per)
                dpred = Out(dev, y_dev.shape, init=y_dev)
                got = tree_chain(dev, td, dpred.p, *shape, o, max_per, best=best.p)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (nms, max_per, "best")
                own = tree_chain(dev, td, dpred.p, *shape, o, max_per)
                assert all(np.array_equal(a, b) for a, b in zip(own, want)), (nms, max_per, "own sweep on the device's rows")
    assert seen > 1                                                               # max_per_image = 1 cut something


def limit_pred(total=4096):
    """MINI rows written by hand: objectness .1 and flat conditionals everywhere, and candidates -- objectness .9, .95 down
    one path, the leaf a little lower from candidate to candidate -- at box 0, at the last box, 80 of class 17, three of
    each of six more classes, and two of class 23 with exactly equal scores"""
    t = R.tree("MINI")
    pred = np.zeros((total, 5 + t.n), F)
    pred[:, :4] = R.synth.uniform(41, total * 4, -1.5, 1.5).reshape(total, 4)
    pred[:, 2:4] *= F(0.5)
    pred[:, 4] = 0.1
    pred[:, 5:] = 0.01
    spots = np.unique((R.synth.uniform01(42, 400).astype(np.float64) * (total - 2)).astype(np.int64) + 1)[:100]
    where = [0, total - 1] + spots.tolist()
    classes = [17, 17] + [17] * 78 + [c for c in (11, 12, 13, 19, 20, 21) for _ in range(3)] + [23, 23]
    for k, (box, c) in enumerate(zip(where, classes)):
        path = R.path_to(t, c)
        pred[box, 4] = 0.9
        pred[box, 5 + np.asarray(path)] = 0.95
        pred[box, 5 + c] = F(0.95) - F(0.001) * F(0 if c == 23 else k % 40)
    return pred, len(classes)


def test_detect_tree_chain_at_its_box_limit(dev, oracle):
    """4096 boxes per image qualify and match the dense chain; 4097 do not"""
    L = dev.L
    t = R.tree("MINI")
    td = TreeDev(dev, t)
    pred, cands = limit_pred()
    val, cls, _ = R.tree_best(pred[:, 5:], t)
    assert (val > 0).sum() == cands and val[0] > 0 and val[-1] > 0
    per_class = np.bincount(cls[val > 0], minlength=t.n)
    assert per_class[17] > 64 and (per_class >= 2).sum() > 4
    v23 = val[(cls == 23) & (val > 0)]
    assert len(v23) == 2 and v23[0] == v23[1]
    anchors = dev.put(R.ANCHORS[:8])
    for nms in (0.4, 0.0, 1e-6):
        for max_per in (4096, 1):
            o = R.Opt((1, 1), 0, 0, 0.24, nms, True)
            want = dense_tree(dev, oracle, td, pred, 1, 32, 32, 4, o, max_per)
            assert want[2][0] == cands if nms == 0 else 1 < want[2][0] < cands
            got = tree_chain(dev, td, dev.put(pred), 1, 32, 32, 4, o, max_per)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (nms, max_per)
    over = np.zeros((4097, 5 + t.n), F)
    o = R.Opt((1, 1), 0, 0, 0.24, 0.4, True)
    boxes = Out(dev, (4097, 4))
    q = decode_struct(dev, 1, 241, 1, 17, t.n, o, dev.put(over), boxes, None, td=td)
    assert L.y2h_detect_tree_chain_ok(C.byref(q)) == 0
    rec, cnt, scratch = Out(dev, (1, 8, 6)), Out(dev, (1,), np.int32), Out(dev, (2 * 4097,))
    assert L.y2h_detect_tree_chain(C.byref(q), 0.4, rec.p, cnt.p, 8, scratch.p, None, None) == EINVAL
    assert (boxes.pull() == FILL).all() and (rec.pull() == FILL).all() and (cnt.pull() == FILL).all()
    del anchors


# =====================================================================================================================
# E. NMS at scale
# =====================================================================================================================
def nms_sort(dev, boxes, probs, batch, total, classes, stride, thresh, expect=0):
    L = dev.L
    dboxes, din = dev.put(boxes), dev.put(probs)
    out = Out(dev, probs.shape, init=probs)
    cc = Out(dev, (batch * classes,), np.int32)
    assert L.y2h_nms_sort(dboxes, din, out.p, batch, total, classes, stride, thresh, cc.p, None) == expect
    if expect == 0:
        counts = cc.pull().reshape(batch, classes)
        assert np.array_equal(counts, (probs.reshape(batch, total, stride)[:, :, :classes] != 0).sum(axis=1))   # class_count_kernel
    return out.pull()


@pytest.mark.parametrize("c", R.NMS_SORT, ids=[c.ident for c in R.NMS_SORT])
def test_nms_sort_at_scale(dev, oracle, c):
    """nms_sort_kernel past NMS_LDS_BOXES candidates per class (the global-memory loop), with tie runs behind it, with
    lds_boxes = 0 (more than 8192 boxes), and at y2h_nms_sort's limit"""
    boxes, probs = R.nms_case(c.total, c.classes, c.seed, c.keep, c.eighths)
    per_class = (probs != 0).sum(axis=0)
    print("%s: candidates per class %s" % (c.ident, per_class.tolist()))
    assert per_class.min() > 1024
    got = nms_sort(dev, boxes, probs, 1, c.total, c.classes, c.classes, 0.4)
    want = oracle.do_nms_sort(boxes, probs, 0.4)
    assert 0 < (want != 0).sum() < (probs != 0).sum()
    assert np.array_equal(got, want)


def test_nms_sort_past_its_limit(dev):
    boxes, probs = R.nms_case(R.NMS_SORT_MAX + 1, 1, 77, 0.5)
    assert np.array_equal(nms_sort(dev, boxes, probs, 1, R.NMS_SORT_MAX + 1, 1, 1, 0.4, expect=EINVAL), probs)


def test_nms_sort_batch_and_padded_rows(dev, oracle):
    """two images, rows of classes + 3 floats (the padding is neither read nor written), a class with exactly one candidate
    and a class with none; classes 0 and 1 of each image take the global-memory loop"""
    total, classes, stride = 2100, 4, 7
    boxes = np.zeros((2, total, 4), F)
    probs = np.full((2, total, stride), 0.99, F)
    for b in range(2):
        boxes[b], p = R.nms_case(total, classes, 77 + 10 * b, 0.45, eighths=(b == 1))
        p[:, 2:] = 0
        p[1234 + b, 2] = 0.7
        probs[b, :, :classes] = p
    assert ((probs[:, :, :2] != 0).sum(axis=1) > 1024).all()
    got = nms_sort(dev, boxes, probs, 2, total, classes, stride, 0.4).reshape(2, total, stride)
    assert (got[:, :, classes:] == F(0.99)).all()
    for b in range(2):
        assert np.array_equal(got[b, :, :classes], oracle.do_nms_sort(boxes[b], probs[b, :, :classes], 0.4)), b


@pytest.mark.parametrize("total,classes,keep", [(17, 3, 0.6), (845, 300, 0.6), (4096, 2, 0.6), (R.NMS_PLAIN_MAX, 2, 0.985)])
def test_nms_plain(dev, oracle, total, classes, keep):
    """nms_plain_kernel: a box count that is no multiple of 16, more classes than the 256 lanes, and y2h_nms's limit (with
    few scores: the walk is sequential in the box index by construction)"""
    L = dev.L
    boxes, probs = R.nms_case(total, classes, 77, keep)
    stride = classes + 1
    padded = np.full((total, stride), 0.99, F)
    padded[:, :classes] = probs
    out = Out(dev, padded.shape, init=padded)
    assert L.y2h_nms(dev.put(boxes), out.p, 1, total, classes, stride, 0.4, None) == 0
    got = out.pull()
    want = oracle.do_nms(boxes, probs, 0.4)
    assert 0 < (want != 0).sum() < (probs != 0).sum() or total < 100
    assert np.array_equal(got[:, :classes], want) and (got[:, classes:] == F(0.99)).all()


def test_nms_plain_past_its_limit(dev):
    boxes, probs = R.nms_case(R.NMS_PLAIN_MAX + 1, 1, 77, 0.9)
    out = Out(dev, probs.shape, init=probs)
    assert dev.L.y2h_nms(dev.put(boxes), out.p, 1, R.NMS_PLAIN_MAX + 1, 1, 1, 0.4, None) == EINVAL
    assert np.array_equal(out.pull(), probs)


# =====================================================================================================================
# F. the YOLOv1 decode
# =====================================================================================================================
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("c", R.V1_CASES, ids=[c.ident for c in R.V1_CASES])
def test_detection_boxes(dev, c, pad):
    """detection_boxes_kernel: no libm call in it, so array_equal throughout"""
    L = dev.L
    stride = c.outputs + pad
    pred = R.v1_pred(c, stride)
    dpred = dev.put(pred)
    n = c.batch * c.side * c.side * c.num
    for oo in (0, 1):
        for (w, h) in ((1, 1), (640, 480)):
            boxes, probs = Out(dev, (n, 4)), Out(dev, (n, c.classes))
            assert L.y2h_detection_boxes(dpred, stride, c.batch, c.side, c.num, c.classes, c.sqrt, w, h, R.V1_THRESH, oo, boxes.p, probs.p, None) == 0
            rb, rp = R.detection_boxes(pred, c.side, c.num, c.classes, c.sqrt, w, h, R.V1_THRESH, oo)
            assert np.array_equal(boxes.pull(), rb) and np.array_equal(probs.pull(), rp), (oo, w, h)
    assert L.y2h_detection_boxes(dpred, stride, 0, c.side, c.num, c.classes, c.sqrt, 1, 1, R.V1_THRESH, 0, boxes.p, probs.p, None) == EINVAL
