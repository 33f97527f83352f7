"""The classifier loader on the device: y2h_augment_cls_to_input through the C-ABI, fed by the product's own packer, against
tests/aug_cls_rule.py on the WHOLE frame, by np.array_equal -- every value is formed by single IEEE operations in a fixed
order, so a tolerance would only hide a reordering -- and the trainer entries end to end on a small classifier.

Provenance: the pixel chain is held to a restatement of the reference's image.c (tests/aug_cls_rule.py: parity with a run of
the reference unpinned); the draws and the label rows are pinned to the compiled reference by tests/test_aug_cls_host.py."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import aug_cls_rule as R
from tests import aug_rule
from tests import train_det_rule as D
from tests import train_rule as T
from tests.test_aug_cls_host import REFUSALS, SMALL, good_items, raw_items, region_cfg
from tests.test_gpu_aug import batch_items, colour_frame, frame, padded, params

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 5, 8, 33)       # a single pixel; an odd row tail with rows of odd alignment; whole groups; more than one block, tail and odd alignment
IDENTITY = dict(rad=0., aspect=1., scale=1., dx=0., dy=0., flip=0, dhue=0., dsat=1., dexp=1.)


def rad(deg):
    return float(F(deg * 2 * math.pi / 360))


def launch(items, size, swap_rb):
    """items: dicts of frame + draws -> float32 [n][size][size][3] of one y2h_augment_cls_to_input launch over what
    y2_aug_cls_pack sends up for them"""
    L = darknet.lib()
    n = len(items)
    arr, keep = darknet.aug_cls_items(items)
    nbytes = L.y2_aug_cls_pack_bytes(arr, n, size)
    desc = (darknet.AugCls * n)()
    pixels = np.zeros(max(nbytes, 1), np.uint8)
    L.y2_aug_cls_pack(arr, n, size, desc, pixels.ctypes.data)
    table = np.frombuffer(bytes(desc), np.uint8)
    d_desc, d_pix, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    out = np.full((n, size, size, 3), np.nan, F)
    assert L.y2h_malloc(C.byref(d_desc), table.size) == 0 and L.y2h_malloc(C.byref(d_pix), pixels.size) == 0
    assert L.y2h_malloc(C.byref(d_out), out.nbytes) == 0
    try:
        assert L.y2h_memcpy_h2d(d_desc, table.ctypes.data, table.size, None) == 0
        assert L.y2h_memcpy_h2d(d_pix, pixels.ctypes.data, pixels.size, None) == 0
        assert L.y2h_memcpy_h2d(d_out, out.ctypes.data, out.nbytes, None) == 0
        assert L.y2h_augment_cls_to_input(d_desc, n, d_pix, int(swap_rb), size, d_out, None) == 0
        assert L.y2h_memcpy_d2h(out.ctypes.data, d_out, out.nbytes, None) == 0
    finally:
        L.y2h_free(d_desc); L.y2h_free(d_pix); L.y2h_free(d_out)
    return out


def rule(it, size, swap_rb):
    d = dict(IDENTITY, **{k: v for k, v in it.items() if k != "frame"})
    return R.augment(it["frame"], size, d["rad"], d["scale"], d["dx"], d["dy"], d["aspect"], d["flip"], d["dhue"], d["dsat"], d["dexp"], swap_rb)


def limits(f, size, scale, aspect):
    """the bounds random_augment_image draws dx and dy between (image.c:1695-1698)"""
    oh, ow = f.shape[:2]
    return max((ow * scale / aspect - size) / 2., 0.), max((oh * scale - size) / 2., 0.)


def geometry_items(size):
    """frames 1x1, 37x53 with a padded pitch, 64x48 with three and four bytes per pixel; 0, +7, -7, 90 and 180 degrees;
    aspect .75, 1 and 4/3; scale below and above 1; dx, dy at 0 and at either limit; both flips; the distortion either way"""
    one, a, b3, b4 = frame(1, 1, 3, 2), padded(frame(53, 37, 3, 3), 5), frame(48, 64, 3, 4), frame(48, 64, 4, 5)
    items = [dict(frame=a), dict(frame=b4, flip=1), dict(frame=one, rad=rad(7), scale=.5, dhue=.1, dsat=1.5)]
    for f, deg, aspect, scale, sx, sy, flip in ((a, 7, .75, 1.6, 1, -1, 1), (b4, -7, 4 / 3., .6, -1, 1, 0), (b3, 90, 1., .8, 1, 1, 1),
                                                (b3, 180, .75, 2.5, -1, -1, 0), (a, -7, 4 / 3., 3., 0, 1, 1), (b4, 7, 1., 1.25, 1, 0, 0)):
        lx, ly = limits(f, size, scale, aspect)
        items.append(dict(frame=f, rad=rad(deg), aspect=aspect, scale=scale, dx=sx * lx, dy=sy * ly, flip=flip, dhue=.1 * (sx or 1),
                          dsat=1.5 if flip else 1 / 1.5, dexp=1 / 1.5 if flip else 1.5))
    items.append(dict(frame=a, rad=rad(45), scale=.04, flip=1, dhue=-.1, dsat=1.5, dexp=1.5))          # over all four edges
    items.append(dict(frame=b3, rad=rad(180), scale=1., dx=500., dy=-400.))                              # wholly beside the frame
    return items


@pytest.mark.parametrize("swap_rb", (0, 1))
@pytest.mark.parametrize("size", SIZES)
def test_kernel_is_the_rule_on_every_geometry(size, swap_rb):
    items = geometry_items(size)
    got = launch(items, size, swap_rb)
    for i, it in enumerate(items):
        assert np.array_equal(got[i], rule(it, size, swap_rb)), "item %d of size %d swap %d" % (i, size, swap_rb)
    assert not np.isnan(got).any()


@pytest.mark.parametrize("size", (8, 16))
def test_integer_landing_is_the_plane_value(size):
    """angle 0, aspect 1, scale 1, an even size and even frame sides, whole dx and dy: every rx, ry is a whole number, floorf
    returns it, the weights are 1, 0, 0, 0 and a grey pixel comes back from the identity distortion as it went in"""
    grey = np.repeat(frame(48, 64, 1, 8), 3, axis=2)
    shifts = ((0, 0), (3, -2), (size // 2 - 32, 24 - size // 2), (32 - size // 2, size // 2 - 24))       # the last two reach opposite corners of the frame
    items = [dict(frame=grey, dx=float(dx), dy=float(dy), flip=k & 1) for k, (dx, dy) in enumerate(shifts)]
    got = launch(items, size, 0)
    plane = aug_rule.planes(grey)
    for k, (dx, dy) in enumerate(shifts):
        x0, y0 = 32 - size // 2 + dx, 24 - size // 2 + dy
        assert 0 <= x0 and x0 + size <= 64 and 0 <= y0 and y0 + size <= 48
        want = plane[y0:y0 + size, x0:x0 + size]
        assert np.array_equal(got[k], want[:, ::-1] if k & 1 else want), k
        assert np.array_equal(got[k], rule(items[k], size, 0)), k


def test_taps_outside_the_frame_repeat_the_edge():
    a = padded(frame(53, 37, 3, 3), 5)
    it = dict(frame=a, scale=.1, rad=rad(7), aspect=.75)
    rx, ry = R.coords(37, 53, 33, it["rad"], it["scale"], 0., 0., it["aspect"])
    assert rx.min() < -1 and rx.max() > 38 and ry.min() < -1 and ry.max() > 54         # the crop hangs over all four edges
    one = frame(1, 1, 4, 6)
    items = [it, dict(frame=one, rad=rad(30), scale=.7, aspect=4 / 3., dx=2., dy=-1.), dict(frame=one, scale=3., flip=1, dhue=.2, dsat=1.5, dexp=.8)]
    got = launch(items, 33, 0)
    for i, item in enumerate(items):
        assert np.array_equal(got[i], rule(item, 33, 0)), i
    # a 1 x 1 frame: every tap is the one pixel.  The four weights of a pixel sum to 1 within a few ulps, not exactly, so the
    # blend is the pixel within 4 * 2^-24 and the distortion (scales <= 1.5, six hue sectors) carries that to well under 1e-5;
    # the yardstick is the rule above, this only says what the rule amounts to
    for i in (1, 2):
        pixel = aug_rule.distort(aug_rule.planes(one), it_d(items[i], "dhue"), it_d(items[i], "dsat"), it_d(items[i], "dexp"))[0, 0]
        assert np.abs(got[i] - pixel).max() < 1e-5, i


@pytest.mark.parametrize("size", (8, 12))
def test_kernel_is_the_rule_on_every_colour_branch(size):
    """the frame of tests/test_gpu_aug.py's colour test, landed on pixel for pixel (even sides, angle 0, scale 1)"""
    f = colour_frame(size, size)
    grey = np.zeros((size, size, 3), np.uint8)
    grey[...] = (np.arange(size * size) % 256).astype(np.uint8).reshape(size, size, 1)
    grey[0, 0] = 0
    items = [dict(frame=f, dhue=d, dsat=s, dexp=e) for d, s, e in ((.1, 1.5, 1 / 1.5), (-.1, 1 / 1.5, 1.5), (.5, 1.5, 1.5), (-.5, 1 / 1.5, 1 / 1.5))]
    items += [dict(frame=grey, dhue=.5, dsat=1.5, dexp=1.5), dict(frame=grey, flip=1, dhue=-.1, dsat=1 / 1.5, dexp=1 / 1.5)]
    items += [dict(frame=f, rad=rad(7), scale=1.3, aspect=.75, dhue=.1, dsat=1.5, dexp=1.5)]          # the same colours, blended
    hh, s, v = aug_rule.rgb_to_hsv(aug_rule.planes(f))
    coloured = s > 0
    seen, up, down, clamped = set(), False, False, False
    for it in items[:4]:
        moved = (hh + F(it["dhue"])).astype(F)
        up |= bool((moved[coloured] > 1).any())
        down |= bool((moved[coloured] < 0).any())
        seen |= set(np.floor(6 * aug_rule.shift_hue(hh, it["dhue"])[coloured].astype(np.float64)).astype(int).tolist())
        clamped |= bool(((v * F(it["dexp"])) > 1).any())
    assert up and down and clamped and {0, 1, 2, 3, 4, 5} <= seen, (up, down, clamped, seen)
    got = launch(items, size, 0)
    for i, it in enumerate(items):
        assert np.array_equal(got[i], rule(it, size, 0)), "item %d of size %d" % (i, size)
    for i in range(4):                                  # landed on whole pixels: the crop is the frame
        assert np.array_equal(got[i], aug_rule.distort(aug_rule.planes(f), it_d(items[i], "dhue"), it_d(items[i], "dsat"), it_d(items[i], "dexp"))), i
    assert not np.isnan(got).any()                      # a grey pixel's 0/0 hue is carried and never read
    assert (got[:4] == 1).any() and (got[:4] == 0).any()


def it_d(it, key):
    return it.get(key, IDENTITY[key])


# ---- the trainer entries, end to end on a small classifier (16 x 16, four images a call, two calls an update) ----
FRAMES = (frame(53, 37, 3, 21), frame(16, 20, 4, 22), padded(frame(10, 12, 3, 23), 3), frame(48, 64, 3, 24))
LABELS = ("tabby", "siamese", "dog", "car", "bus")
PATHS = ("set/tabby_a.jpg", "set/dog_c.jpg", "set/bus_b.jpg", "set/siamese_d.jpg")


def cls_batch(step, size=16):
    """four frames of four sizes with the draws the reference would make after srand(900 + step), tiny.cfg's values"""
    darknet.srand(900 + step)
    items = [dict(darknet.aug_draw_classification(f.shape[1], f.shape[0], size, size * 2, size, 7., .75, .1, .75, .75), frame=f) for f in FRAMES]
    truth = np.stack([darknet.aug_labels(p, LABELS)[0] for p in PATHS])
    return items, np.roll(truth, step, axis=0)


def test_loaded_steps_are_train_network_datum_on_the_pulled_batch(workdir):
    cfg, wts, _ = T.materialize(workdir, "S", 7203, spec=SMALL)
    a = darknet.Network.parse_network_cfg(cfg)
    b = darknet.Network.parse_network_cfg(cfg)
    a.load_weights(wts)
    b.load_weights(wts)
    assert a.net.batch == 4 and a.net.subdivisions == 2 and a.truth_floats() == len(LABELS)
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        a.train_step_loaded()
    L = darknet.lib()
    for step in (1, 2, 3):
        items, truth = cls_batch(step)
        a.train_load_classification(items, truth, swap_rb=bool(step == 2))
        x, y = a.train_pull_input()
        for i, it in enumerate(items):                  # the input is the rule's, the truth the caller's
            assert np.array_equal(x[i], rule(it, 16, step == 2).transpose(2, 0, 1)), (step, i)
        assert np.array_equal(y.view(np.uint32), truth.view(np.uint32)), step
        la = a.train_step_loaded()
        lb = L.train_network_datum(b.net, x.ctypes.data, y.ctypes.data)
        assert np.isfinite(la) and F(la).tobytes() == F(lb).tobytes(), (step, la, lb)
    assert a.net.seen[0] == b.net.seen[0] == 12
    pa, pb = params(a), params(b)
    assert pa.keys() == pb.keys() and len(pa) > 0
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert np.isfinite(a.train_step_loaded())           # a second step on the same load
    assert all(t >= 0 for t in a.train_load_times())
    a.free()
    b.free()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_a_refused_load_leaves_nothing_loaded(workdir, what):
    cfg, wts, _ = T.materialize(workdir, "S", 7203, spec=SMALL)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    items, truth = cls_batch(1)
    net.train_load_classification(items, truth)
    assert np.isfinite(net.train_step_loaded())
    seen = net.net.seen[0]
    change, pattern = REFUSALS[what]
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_load_classification(change(good_items(4)), truth)
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        net.train_step_loaded()
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        net.train_pull_input()
    assert net.net.seen[0] == seen == 4
    net.train_load_classification(items, truth)         # and the next good load steps
    assert np.isfinite(net.train_step_loaded()) and net.net.seen[0] == 8
    net.free()


@pytest.mark.parametrize("kw, pattern", [(dict(data=None), r"item 1: data is NULL"), (dict(step=20), r"item 1: step 20 is less than w\*c = 21"),
                                         (dict(h=0), r"item 1: bad frame geometry 0 x 7"), (dict(w=0), r"item 1: bad frame geometry 9 x 0"),
                                         (dict(c=2), r"item 1: the frame has 2 channels")])
def test_a_refused_item_leaves_nothing_loaded(workdir, kw, pattern):
    """what darknet.aug_cls_items cannot express -- NULL data, a short step, a frame without pixels --, field by field"""
    cfg, wts, _ = T.materialize(workdir, "S", 7203, spec=SMALL)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    items, truth = cls_batch(1)
    net.train_load_classification(items, truth)
    assert np.isfinite(net.train_step_loaded())
    seen = net.net.seen[0]
    arr, keep = raw_items(4, **kw)
    assert darknet.lib().y2_train_load_classification(C.byref(net.net), arr, truth.ctypes.data, 4, 0) == -1
    assert re.search(pattern, darknet._check())
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        net.train_step_loaded()
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        net.train_pull_input()
    assert net.net.seen[0] == seen == 4
    net.train_load_classification(items, truth)         # and the next good load steps
    assert np.isfinite(net.train_step_loaded()) and net.net.seen[0] == 8
    net.free()


def test_refusals_that_name_the_network_or_the_truth(workdir):
    cfg, wts, _ = T.materialize(workdir, "S", 7203, spec=SMALL)
    net = darknet.Network.parse_network_cfg(cfg)
    items, truth = cls_batch(1)
    net.train_load_classification(items, truth)
    arr, keep = darknet.aug_cls_items(items)
    assert darknet.lib().y2_train_load_classification(C.byref(net.net), arr, None, 4, 0) == -1
    assert "truth is NULL" in darknet._check()
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        net.train_step_loaded()
    assert net.net.seen[0] == 0
    net.free()
    big = np.zeros(4096, F)
    nets = [(T.materialize(workdir, "R%d" % k, 1, spec=spec)[0], pattern) for k, (spec, pattern) in enumerate((
        (dict(SMALL, w=20), r"the network is 20 x 16"), (dict(SMALL, c=1), r"reads 1 channels"),
        (dict(SMALL, layers=[("conv", 6, 3, 1, 1, "leaky"), ("softmax", 1.0), ("cost",)]), r"put an \[avgpool\] in front")))]
    nets.append((region_cfg(workdir), r"ends in \[region\]"))
    for cfg, pattern in nets:
        net = darknet.Network.parse_network_cfg(cfg)
        arr, keep = darknet.aug_cls_items(good_items(net.net.batch))
        assert darknet.lib().y2_train_load_classification(C.byref(net.net), arr, big.ctypes.data, net.net.batch, 0) == -1
        assert re.search(pattern, darknet._check()), pattern
        with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
            net.train_step_loaded()
        assert net.net.seen[0] == 0
        net.free()


def detection_run(workdir):
    cfg, wts, _ = D.materialize(workdir, "E", 7103)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.train_load_detection(batch_items(1))
    x, y = net.train_pull_input()
    loss = net.train_step_loaded()
    out = (x.copy(), y.copy(), F(loss).tobytes(), params(net))
    net.free()
    return out


def test_detection_loader_is_unchanged_by_a_classification_load(workdir):
    before = detection_run(workdir)
    cfg, wts, _ = T.materialize(workdir, "S", 7203, spec=SMALL)
    cls = darknet.Network.parse_network_cfg(cfg)
    cls.load_weights(wts)
    cls.train_load_classification(*cls_batch(2))
    assert np.isfinite(cls.train_step_loaded())
    after = detection_run(workdir)                      # with the classifier's trainer and its load still alive
    cls.free()
    assert np.isfinite(np.frombuffer(before[2], F)[0])
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
    assert before[3].keys() == after[3].keys()
    for k in before[3]:
        assert before[3][k].tobytes() == after[3][k].tobytes(), k
