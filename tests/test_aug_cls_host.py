"""The classifier loader's host half, without a device: the draws and the label rows against tests/golden/aug_cls.npz (the
COMPILED reference's load_data_augment, run whole: tests/golden/gen_aug_cls_golden.py), y2_net_augment_classifier against the
cfg text, the packer against the taps tests/aug_cls_rule.py computes on the whole frame, every refusal of
y2_train_load_classification, the exports, and csrc/host/y2_aug.c as a stand-alone program under
-fsanitize=address,undefined."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import aug_cls_rule as R
from tests import train_rule as T
from tests.helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CASES = range(3)
# conv + maxpool + conv + avgpool + softmax + cost on 16 x 16, four images a call, two calls an update
SMALL = dict(w=16, h=16, c=3, batch=4, subdivisions=2, learning_rate=0.01, momentum=0.9, decay=0.0005, policy="constant",
             layers=[("conv", 6, 3, 1, 1, "leaky"), ("max", 2, 2), ("conv", 5, 3, 1, 0, "linear"), ("avg",), ("softmax", 1.0), ("cost",)])


@pytest.fixture(scope="module")
def fix():
    return load_golden("aug_cls")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tree_of(parent):
    """a darknet.Tree over `parent` as read_tree lays it out (a new group wherever the parent changes) -> (Tree, kept arrays)"""
    parent = np.ascontiguousarray(parent, np.int32)
    sizes = []
    for i, p in enumerate(parent):
        if i == 0 or p != parent[i - 1]:
            sizes.append(0)
        sizes[-1] += 1
    sizes = np.array(sizes, np.int32)
    t = darknet.Tree()
    t.n = len(parent)
    t.parent = parent.ctypes.data_as(type(t.parent))
    t.groups = len(sizes)
    t.group_size = sizes.ctypes.data_as(type(t.group_size))
    return t, (parent, sizes)


def test_fixture_holds_the_cases_it_is_about(fix):
    aspect, angle, sat, exp = (set(fix["cases"][:, k].tolist()) for k in (1, 2, 3, 4))
    assert aspect == {.75, 1.} and angle == {0., 7.} and sat == {.75, 1.5} and exp == {.75, 1.5}
    assert {tuple(s) for s in fix["sizes"].tolist()} == {(37, 53), (64, 48), (500, 375)}
    flips, zero, free, secret = set(), 0, 0, 0
    for k in CASES:
        flips |= set(fix["c%d_flip" % k].tolist())
        zero += int((fix["c%d_crop" % k][:, 3] == 0).sum())
        free += int((fix["c%d_crop" % k][:, 3] != 0).sum())
        secret += int((fix["c%d_truth" % k] == -1234).sum())
    assert flips == {0, 1} and zero > 0 and free > 0 and secret > 0
    matches = {sum(l in p for l in fix["labels"].tolist()) for p in fix["paths"].tolist()}
    assert {0, 1, 2} <= matches
    assert len(tree_of(fix["parent"])[1][1]) >= 3


@pytest.mark.parametrize("k", CASES)
def test_draws_follow_the_reference_rand_order(fix, k):
    """srand(seed), the batch's paths, then image by image the draws: what the reference's single thread does"""
    seed, aspect, angle, sat, exp = (float(v) for v in fix["cases"][k])
    lo, hi, size, _ = (int(v) for v in fix["crop"][k])
    darknet.srand(int(seed))
    n = len(fix["c%d_path" % k])
    paths = darknet.aug_random_paths(n, len(fix["sizes"]))
    assert np.array_equal(paths, fix["c%d_path" % k])
    for i, p in enumerate(paths):
        ow, oh = (int(v) for v in fix["sizes"][p])
        d = darknet.aug_draw_classification(ow, oh, lo, hi, size, angle, aspect, float(fix["hue"]), sat, exp)
        assert np.array_equal(bits([d[key] for key in ("aspect", "scale", "rad", "dx", "dy")]), bits(fix["c%d_crop" % k][i])), (k, i, d)
        assert d["flip"] == fix["c%d_flip" % k][i], (k, i)
        assert np.array_equal(bits([d["dhue"], d["dsat"], d["dexp"]]), bits(fix["c%d_distort" % k][i])), (k, i)


@pytest.mark.parametrize("k", CASES)
def test_label_rows_are_the_reference_bit_for_bit(fix, k):
    labels = fix["labels"].tolist()
    tree, keep = tree_of(fix["parent"]) if fix["crop"][k][3] else (None, None)
    for i, p in enumerate(fix["c%d_path" % k]):
        path = str(fix["paths"][p])
        got, count = darknet.aug_labels(path, labels, tree)
        assert np.array_equal(bits(got), bits(fix["c%d_truth" % k][i])), (k, i, path)
        assert count == sum(l in path for l in labels), (k, i, path)


@pytest.mark.parametrize("name, extra, want", [
    ("tiny.cfg", None, dict(min_crop=224, max_crop=320, angle=7, aspect=.75, hue=.1, saturation=.75, exposure=.75)),
    (None, None, dict(min_crop=16, max_crop=32, angle=0, aspect=1, hue=0, saturation=1, exposure=1)),
    (None, dict(min_crop=20, max_crop=48, angle=30, aspect=.5, hue=.2), dict(min_crop=20, max_crop=48, angle=30, aspect=.5, hue=.2, saturation=1, exposure=1)),
])
def test_net_augment_classifier_reports_the_cfg(tmp_path, name, extra, want):
    if name:
        path = os.path.join(GOLDEN, "ref_cfg", name)
        text = open(path).read().replace(" ", "")
        for key in ("angle", "aspect", "hue", "saturation", "exposure", "max_crop"):     # the expectation is what the cfg text says
            assert "\n%s=%s" % (key, ("%g" % want[key]).lstrip("0")) in text, (name, key)
        assert "min_crop" not in text and "\nwidth=224" in text
    else:
        path, _, _ = T.materialize(str(tmp_path), "S", 1, spec=SMALL, extra=extra)
    net = darknet.Network.parse_network_cfg(path)
    got = net.net_augment_classifier()
    null_ok = darknet.lib().y2_net_augment_classifier(net.net, *[None] * 7)
    net.free()
    assert null_ok == 0
    assert (got["min_crop"], got["max_crop"]) == (want["min_crop"], want["max_crop"])
    for key in ("angle", "aspect", "hue", "saturation", "exposure"):
        assert F(got[key]) == F(want[key]), (name, key, got)


def test_net_augment_classifier_needs_an_engine():
    assert darknet.lib().y2_net_augment_classifier(darknet.CNetwork(), *[None] * 7) == -1
    assert "no engine" in darknet._check()


def test_draw_refuses_a_side_that_truncates_to_0():
    with pytest.raises(darknet.Y2Error, match="truncates to 0"):
        darknet.aug_draw_classification(37, 0, 16, 32, 16, 0., 1., 0., 1., 1.)          # oh
    with pytest.raises(darknet.Y2Error, match="truncates to 0"):
        darknet.aug_draw_classification(0, 53, 16, 32, 16, 0., 1., 0., 1., 1.)          # (int)(ow * aspect)
    below, other = 0, 0
    for seed in range(12):                  # 1 * aspect truncates to 0 exactly when the drawn aspect is below 1
        darknet.srand(seed)
        try:
            d = darknet.aug_draw_classification(1, 53, 16, 32, 16, 0., .4, 0., 1., 1.)
            assert d["aspect"] >= 1
            other += 1
        except darknet.Y2Error:
            below += 1
    assert below > 0 and other > 0
    # a refused draw made every draw: the sequence behind it is the one behind an accepted draw
    libc_rand = darknet.C.CDLL(None).rand
    darknet.srand(3)
    darknet.aug_draw_classification(37, 53, 16, 32, 16, 0., 1., 0., 1., 1.)
    want = libc_rand()
    darknet.srand(3)
    with pytest.raises(darknet.Y2Error):
        darknet.aug_draw_classification(37, 0, 16, 32, 16, 0., 1., 0., 1., 1.)
    assert libc_rand() == want


# ---- the packer against the rule's taps ----
def sweep():
    """240 seeded items: every angle in [-180, 180], aspect .5 - 2, scale .2 - 4, shifts that push the window over every edge
    (and, every eighth item, wholly out of the frame), frames from 1 x 1 to 500 x 375, output sizes 1 to 33"""
    rng = np.random.RandomState(20260)
    frames = ((53, 37), (48, 64), (375, 500), (5, 7), (9, 1), (1, 9), (1, 1))
    out = []
    for i in range(240):
        oh, ow = frames[i % len(frames)]
        size = (1, 5, 8, 33, 16)[i % 5]
        deg = (-180., 180., 0., 90., -90., 7., -7.)[i % 7] if i < 28 else rng.uniform(-180, 180)
        far = 4. if i % 8 == 7 else .75
        out.append(dict(oh=oh, ow=ow, size=size, rad=F(deg * 2 * math.pi / 360), aspect=F(rng.uniform(.5, 2)), scale=F(rng.uniform(.2, 4)),
                        dx=F(rng.uniform(-far, far) * ow), dy=F(rng.uniform(-far, far) * oh), flip=i & 1))
    return out


def draws_of(it):
    return {k: float(it[k]) for k in ("rad", "aspect", "scale", "dx", "dy")}


def test_packed_rectangle_holds_every_tap_of_the_rule():
    edges = dict(left=0, right=0, top=0, bottom=0)
    for i, it in enumerate(sweep()):
        frame = np.zeros((it["oh"], it["ow"], 3), np.uint8)
        x0, y0, rw, rh = darknet.aug_cls_rect(dict(draws_of(it), frame=frame), it["size"])
        assert 0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= it["ow"] and y0 + rh <= it["oh"], (i, it)
        rx, ry = R.coords(it["ow"], it["oh"], it["size"], it["rad"], it["scale"], it["dx"], it["dy"], it["aspect"])
        (tx0, tx1, ty0, ty1), _, _ = R.taps(it["ow"], it["oh"], rx, ry)
        assert x0 <= tx0.min() and tx1.max() < x0 + rw and y0 <= ty0.min() and ty1.max() < y0 + rh, (i, it, (x0, y0, rw, rh))
        edges["left"] += int(rx.min() < 0); edges["right"] += int(rx.max() > it["ow"])
        edges["top"] += int(ry.min() < 0); edges["bottom"] += int(ry.max() > it["oh"])
    assert all(v > 20 for v in edges.values()), edges           # the sweep does hang over every edge


@pytest.mark.parametrize("scale", (2., 3., 4.))
@pytest.mark.parametrize("deg", (0., 7., 45., 90.))
def test_a_centred_zoomed_crop_sends_less_than_the_frame(scale, deg):
    frame = np.zeros((375, 500, 3), np.uint8)
    x0, y0, rw, rh = darknet.aug_cls_rect(dict(frame=frame, scale=scale, rad=deg * 2 * math.pi / 360), 224)
    assert rw < 500 and rh < 375 and rw * rh <= (224 / scale * 1.42 + 5) ** 2, (x0, y0, rw, rh)
    items, keep = darknet.aug_cls_items([dict(frame=frame, scale=scale, rad=deg * 2 * math.pi / 360)])
    assert darknet.lib().y2_aug_cls_pack_bytes(items, 1, 224) == rw * rh * 3


def test_pack_copies_the_rectangle_and_fills_the_table():
    rng = np.random.default_rng(4)
    wide = rng.integers(0, 256, size=(53, 37 * 4 + 5), dtype=np.uint8)
    frame = np.lib.stride_tricks.as_strided(wide, shape=(53, 37, 4), strides=(wide.strides[0], 4, 1))      # four bytes a pixel, padded rows
    its = [dict(frame=frame, scale=1.5, rad=.3, aspect=.75, dx=3., dy=-2., flip=1, dhue=.1, dsat=1.5, dexp=.8),
           dict(frame=frame, scale=.1)]
    items, keep = darknet.aug_cls_items(its)
    nbytes = darknet.lib().y2_aug_cls_pack_bytes(items, 2, 8)
    desc = (darknet.AugCls * 2)()
    pixels = np.full(nbytes + 16, 0xEE, np.uint8)
    darknet.lib().y2_aug_cls_pack(items, 2, 8, desc, pixels.ctypes.data)
    assert (pixels[nbytes:] == 0xEE).all()
    off = 0
    for d, it in zip(desc, its):
        assert (d.src, d.pitch, d.c, d.ow, d.oh) == (off, d.rw * 4, 4, 37, 53)
        assert np.array_equal(pixels[off:off + d.pitch * d.rh].reshape(d.rh, d.rw, 4), frame[d.y0:d.y0 + d.rh, d.x0:d.x0 + d.rw])
        off += d.pitch * d.rh
        rad, s, a = F(it.get("rad", 0.)), F(it["scale"]), F(it.get("aspect", 1.))
        assert d.cosr == R._libm.cos(float(rad)) and d.sinr == R._libm.sin(float(rad)) and d.s == float(s) and d.aspect == float(a)
        assert d.ax == float(F(F(F(it.get("dx", 0.)) / s) * a)) and d.ay == float(F(F(it.get("dy", 0.)) / s))
        assert (d.cx, d.cy) == (18.5, 26.5) and d.flip == int(it.get("flip", 0))
    assert off == nbytes
    assert (desc[1].x0, desc[1].y0, desc[1].rw, desc[1].rh) == (0, 0, 37, 53)          # a crop that hangs over every edge reads the whole frame


# ---- refusals, without a device ----
def good_items(batch, h=9, w=7):
    return [dict(frame=np.full((h, w, 3), 40 + i, np.uint8)) for i in range(batch)]


def small_net(tmp, spec=SMALL):
    cfg, _, _ = T.materialize(str(tmp), "S", 1, spec=spec)
    return darknet.Network.parse_network_cfg(cfg)


REFUSALS = {
    "too_few_items": (lambda it: it[:-1], r"3 items for a batch-4 network"),
    "too_many_items": (lambda it: it + it[:1], r"5 items for a batch-4 network"),
    "two_channels": (lambda it: it[:1] + [dict(it[1], frame=np.zeros((9, 7, 2), np.uint8))] + it[2:], r"item 1: the frame has 2 channels"),
    "scale_zero": (lambda it: it[:2] + [dict(it[2], scale=0.)] + it[3:], r"item 2: scale 0 is not finite and positive"),
    "scale_negative": (lambda it: [dict(it[0], scale=-1.)] + it[1:], r"item 0: scale -1 is not finite and positive"),
    "scale_inf": (lambda it: it[:3] + [dict(it[3], scale=float("inf"))], r"item 3: scale inf is not finite and positive"),
    "scale_nan": (lambda it: it[:3] + [dict(it[3], scale=float("nan"))], r"item 3: scale -?nan is not finite and positive"),
    "aspect_zero": (lambda it: it[:1] + [dict(it[1], aspect=0.)] + it[2:], r"item 1: aspect 0 is not finite and positive"),
    "aspect_inf": (lambda it: it[:1] + [dict(it[1], aspect=float("inf"))] + it[2:], r"item 1: aspect inf is not finite and positive"),
    "rad_nan": (lambda it: it[:1] + [dict(it[1], rad=float("nan"))] + it[2:], r"item 1: rad -?nan is not finite"),
    "dx_inf": (lambda it: it[:1] + [dict(it[1], dx=float("inf"))] + it[2:], r"item 1: dx inf is not finite"),
    "dy_inf": (lambda it: it[:1] + [dict(it[1], dy=float("-inf"))] + it[2:], r"item 1: dy -inf is not finite"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_load_refuses_before_the_device(tmp_path, what):
    """without a device a refusal that came after a device call would carry HIP's message instead; with one, preparing the
    trainer would have waited for its uploads (the wait counter stands still)"""
    net = small_net(tmp_path)
    change, pattern = REFUSALS[what]
    truth = np.zeros((4, net.truth_floats()), F)
    waits = darknet.stream_syncs()
    seen = net.net.seen[0]
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_load_classification(change(good_items(4)), truth)
    with pytest.raises(darknet.Y2Error, match=r"nothing is loaded"):
        net.train_step_loaded()
    with pytest.raises(darknet.Y2Error, match=r"nothing is loaded"):
        net.train_pull_input()
    assert darknet.stream_syncs() == waits and net.net.seen[0] == seen
    net.free()


def raw_items(n, **kw):
    """AugClsItems built field by field, item 1 changed, for what darknet.aug_cls_items cannot express"""
    arr, keep = (darknet.AugClsItem * n)(), []
    for i in range(n):
        frame = np.zeros((9, 7, 3), np.uint8)
        f = dict(data=frame.ctypes.data, h=9, w=7, c=3, step=21, aspect=1., scale=1., rad=0., dx=0., dy=0., flip=0, dhue=0., dsat=1., dexp=1.)
        f.update(kw if i == 1 else {})
        arr[i] = darknet.AugClsItem(**f)
        keep.append(frame)
    return arr, keep


@pytest.mark.parametrize("kw, pattern", [(dict(data=None), r"item 1: data is NULL"), (dict(step=20), r"item 1: step 20 is less than w\*c = 21"),
                                         (dict(h=0), r"item 1: bad frame geometry"), (dict(w=-3), r"item 1: bad frame geometry")])
def test_load_refuses_a_bad_item_by_number(tmp_path, kw, pattern):
    net = small_net(tmp_path)
    arr, keep = raw_items(4, **kw)
    truth = np.zeros((4, net.truth_floats()), F)
    assert darknet.lib().y2_train_load_classification(darknet.C.byref(net.net), arr, truth.ctypes.data, 4, 0) == -1
    assert re.search(pattern, darknet._check())
    net.free()


def test_load_refuses_null_truth_and_null_items(tmp_path):
    net = small_net(tmp_path)
    arr, keep = raw_items(4)
    assert darknet.lib().y2_train_load_classification(darknet.C.byref(net.net), arr, None, 4, 0) == -1
    assert "truth is NULL" in darknet._check()
    truth = np.zeros((4, net.truth_floats()), F)
    assert darknet.lib().y2_train_load_classification(darknet.C.byref(net.net), None, truth.ctypes.data, 4, 0) == -1
    assert "no items" in darknet._check()
    net.free()


def region_cfg(tmp):
    path = os.path.join(tmp, "region.cfg")
    with open(path, "w") as f:
        f.write("[net]\nbatch=2\nwidth=6\nheight=6\nchannels=3\n[convolutional]\nfilters=12\nsize=1\nstride=1\npad=1\nactivation=linear\n"
                "[region]\nanchors=1,1,2,2\nclasses=1\ncoords=4\nnum=2\nsoftmax=1\n")
    return path


NOT_FED = {
    "detector": (lambda tmp: region_cfg(tmp), None, r"ends in \[region\]"),
    "one_channel": (None, dict(SMALL, c=1), r"reads 1 channels"),
    "not_square": (None, dict(SMALL, w=20), r"the network is 20 x 16"),
    "trainer_refuses": (None, dict(SMALL, layers=[("conv", 6, 3, 1, 1, "leaky"), ("softmax", 1.0), ("cost",)]), r"put an \[avgpool\] in front"),
}


@pytest.mark.parametrize("what", sorted(NOT_FED))
def test_load_refuses_a_network_it_cannot_feed(tmp_path, what):
    make, spec, pattern = NOT_FED[what]
    net = darknet.Network.parse_network_cfg(make(str(tmp_path))) if make else small_net(tmp_path, spec)
    arr, keep = raw_items(net.net.batch)
    truth = np.zeros(4096, F)
    waits = darknet.stream_syncs()
    assert darknet.lib().y2_train_load_classification(darknet.C.byref(net.net), arr, truth.ctypes.data, net.net.batch, 0) == -1
    assert re.search(pattern, darknet._check())
    assert darknet.stream_syncs() == waits
    net.free()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"y2h_augment_cls_to_input", "y2_aug_draw_classification", "y2_aug_labels", "y2_net_augment_classifier",
            "y2_train_load_classification"}
    assert want <= have, sorted(want - have)


def test_host_half_stand_alone_under_sanitizers(tmp_path):
    """csrc/host/y2_aug.c + tests/native/aug_cls_host_main.c as one program with its own main, nothing preloaded: the packer over
    crops that hang over every edge of exactly-sized heap frames, the label rows and the draws"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "aug_cls_host")
    src = os.path.join(ROOT, "sr_object_detection_amd", "csrc", "host")
    # the sanitizers' runtimes are linked into the program itself, so they come first whatever else a host loads
    build = subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + src,
                            os.path.join(src, "y2_aug.c"), os.path.join(ROOT, "tests", "native", "aug_cls_host_main.c"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler cannot link the sanitizers here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "aug_cls_host ok" in run.stdout, run.stdout + run.stderr
