"""The depth stage of the Kinect loop on the device (y2_depth_upload / y2_depth_boxes / y2_ingest_regions_depth /
y2_detect_regions_depth / test_detector_regions_depth) against the numpy restatement in tests/depth_rule.py.  The core
is integer and the float steps are single IEEE operations, so every comparison is array_equal: no tolerance anywhere
(NaN == NaN for the fields the reference itself leaves NaN)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import depth_rule
from tests.test_gpu_regions import _mini
from tests.test_native_callers import build

pytestmark = pytest.mark.gpu

H, W, DH, DW = 64, 96, 24, 32                 # colour 96 x 64, depth 32 x 24


def _same(a, b):
    """array_equal over every field of two DET3D_DTYPE arrays, NaN equal to NaN"""
    assert a.shape == b.shape
    for k in depth_rule.FIELDS:
        x, y = a[k], b[k]
        ok = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert ok, (k, x, y)


def _map(h, w, seed):
    """a colour -> depth map with every case the alignment rule names"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    m = np.stack([xs * np.float32(DW / w) + rng.uniform(-0.6, 0.6, (h, w)).astype(np.float32),
                  ys * np.float32(DH / h) + rng.uniform(-0.6, 0.6, (h, w)).astype(np.float32)], axis=-1).astype(np.float32)
    special = [3.5, 0.5, DW - 0.5, DW - 1.5,                  # exactly k + 0.5
               -0.5, -0.7, -1.0, -1.49, -1.5,                 # (-1.5, -0.5]: truncation toward zero lands on 0; -1.5 does not
               float(DW), DW + 0.2, 1e6,                      # >= dw
               np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483520.0, -2147483648.0]
    k = 0
    for r in range(2, h, 5):                                  # each special value in X, in Y and in both
        for c in range(1, w, 7):
            v = np.float32(special[k % len(special)])
            if k % 3 != 1:
                m[r, c, 0] = v
            if k % 3 != 0:
                m[r, c, 1] = v if v < DH or not np.isfinite(v) else np.float32(DH + (k % 2) * 0.3)
            k += 1
    return m


def _depth(seed):
    rng = np.random.default_rng(seed)
    # the values the filter and the thresholds turn on (depth8 = 15, 16, 24, 25, 26, 40, 41, 0) and ordinary ones
    pool = np.array([0, 15 * 32, 15 * 32 + 31, 16 * 32, 24 * 32 + 31, 25 * 32, 25 * 32 + 7, 26 * 32, 40 * 32 + 31, 41 * 32,
                     600, 900, 1200, 2500, 4000, 8191], np.uint16)
    depth = pool[rng.integers(0, len(pool), (DH, DW))]
    body = rng.choice(np.array([0, 1, 2, 3, 6, 7, 255], np.uint8), (DH, DW))
    return depth, body


@pytest.fixture(scope="module")
def net3(workdir):
    net, _, _ = _mini(workdir, 3, tag="depth")
    yield net
    net.free()


@pytest.mark.parametrize("h,w,with_body", [(64, 96, True), (64, 96, False), (64, 97, True), (63, 97, True)])
def test_alignment_equals_the_rule(net3, h, w, with_body):
    """63 x 97 is no multiple of 4: the kernel's scalar tail runs with a map"""
    depth, body = _depth(1)
    m = _map(h, w, 2)
    assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and (m == np.float32(3e9)).any()
    assert ((m > -1.5) & (m <= -0.5)).any() and (m >= DW).any() and (m == 3.5).any()
    net3.depth_upload(depth, body if with_body else None, m)
    want = depth_rule.align(depth, body if with_body else None, m)
    got = net3.depth_aligned()
    for g, x in zip(got, want[:3]):
        assert g.shape == (h, w) and np.array_equal(g, x)
    unmapped = want[3][..., 0] < 0
    assert unmapped.any() and (~unmapped).any() and (got[2][unmapped] == 255).all()
    # x86's INT_MIN for NaN is "unmapped"; the GPU's convert gives 0, which would read depth[.., 0]
    assert unmapped[np.isnan(m).any(axis=-1)].all()
    # X = -0.7 lands on column 0 (truncation toward zero)
    hit = (m[..., 0] == np.float32(-0.7)) & ~unmapped
    assert hit.any() and (want[3][hit][:, 0] == 0).all()


def test_alignment_identity_form(net3):
    rng = np.random.default_rng(3)
    depth = rng.integers(0, 65536, (37, 53)).astype(np.uint16)            # 37 * 53 is odd: a scalar tail
    body = rng.integers(0, 8, (37, 53)).astype(np.uint8)
    net3.depth_upload(depth, body, None)
    d16, d8, per = net3.depth_aligned()
    assert np.array_equal(d16, depth) and np.array_equal(d8, (depth >> 5).astype(np.uint8)) and np.array_equal(per, body)
    net3.depth_upload(depth, None, None)
    assert (net3.depth_aligned()[2] == 255).all()
    with pytest.raises(darknet.Y2Error, match="map"):
        net3.depth_upload(depth, None, None, color_hw=(64, 96))


# ---------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------
FRAME = np.random.default_rng(7).integers(0, 255, size=(H, W, 4), dtype=np.uint8)      # BGRA, no 255 of its own
RECTS = [None, (5, 3, 40, 44), (50, 10, 37, 53)]
FAR = [0.0, 0.8, 1.3]                         # limits 25.0 and 40.625: depth8 25 / 41 are whitened, 24 / 40 are not


def _layers(net):
    assert darknet.lib().y2_forward_device(net.net, None) == 0
    return [net.pull_layer_output(i) for i in range(net.n)]


@pytest.fixture(scope="module")
def plain(workdir):
    net, _, _ = _mini(workdir, 3, tag="depthplain")
    net.set_fusion(False)                                     # every layer's output is stored
    yield net
    net.free()


@pytest.mark.parametrize("letterbox", [False, True])
def test_filter_off_is_ingest_regions(plain, letterbox):
    items = [(FRAME, r) for r in RECTS]
    plain.ingest_regions(items, swap_rb=True, letterbox=letterbox)
    want = _layers(plain)
    plain.ingest_regions_depth(items, [0.0, -1.0, 0.0], swap_rb=True, letterbox=letterbox)      # needs no depth frame
    got = _layers(plain)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "layer %d" % i


@pytest.mark.parametrize("letterbox", [False, True])
def test_filter_equals_host_whitened_crops(plain, letterbox):
    depth, body = _depth(4)
    m = _map(H, W, 5)
    plain.depth_upload(depth, body, m)
    d8 = depth_rule.align(depth, body, m)[1]
    assert all((d8 == v).any() for v in (0, 15, 16, 24, 25, 26, 40, 41))
    items = [(FRAME, r) for r in RECTS]
    white = [(depth_rule.whiten(FRAME, r, d8, f), r) for r, f in zip(RECTS, FAR)]
    for (a, _), (b, r), f in zip(items, white, FAR):
        x, y, rw, rh = r or (0, 0, W, H)
        changed = (a != b).any(axis=-1)
        crop8 = d8[y:y + rh, x:x + rw]
        if f > 0:
            lim = 25 if f == 0.8 else 41
            assert np.array_equal(changed[y:y + rh, x:x + rw], (crop8 <= 15) | (crop8 >= lim))
            assert changed.sum() == changed[y:y + rh, x:x + rw].sum() > 0
        else:
            assert not changed.any()
    plain.ingest_regions(white, swap_rb=True, letterbox=letterbox)
    want = _layers(plain)
    plain.ingest_regions_depth(items, FAR, swap_rb=True, letterbox=letterbox)
    got = _layers(plain)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "layer %d" % i
    plain.ingest_regions(items, swap_rb=True, letterbox=letterbox)
    assert not np.array_equal(_layers(plain)[0], want[0])                 # the filter did change the input
    # a filtered item of another frame size is refused, and nothing ran
    other = np.zeros((H, W + 1, 3), np.uint8)
    with pytest.raises(darknet.Y2Error, match="item 1"):
        plain.ingest_regions_depth([items[0], (other, (0, 0, 20, 20))], [0.0, 0.9])


# ---------------------------------------------------------------------------
# per-box statistics
# ---------------------------------------------------------------------------
def _box(left, top, right, bot, w, h):
    """a frame-relative box whose ROI in a w x h frame is exactly [left, right) x [top, bot)"""
    l, r, t, b = (left + 0.25) / w, (right + 0.25) / w, (top + 0.25) / h, (bot + 0.25) / h
    return np.array([(l + r) / 2, (t + b) / 2, r - l, b - t], np.float32)


def _check_boxes(net, boxes, planes, table, expect_rois=None):
    d16, d8, per, dxy = planes
    want = depth_rule.as_records([depth_rule.box_stats(b, d16, d8, per, dxy, table) for b in boxes], darknet.DET3D_DTYPE)
    if expect_rois is not None:
        for s, e in zip(want, expect_rois):
            if e is not None:
                assert (s["left"], s["top"], s["right"], s["bot"]) == e, (s, e)
    got = net.depth_boxes(boxes)
    _same(got, want)
    return want


def test_depth_boxes_small_frame(net3):
    """colour 96 x 64 through a map: the degenerate ROIs, clamping, an invalid box, no depth, nothing mapped"""
    depth, body = _depth(8)
    depth[0:6, 0:8] = 0                                       # a block without depth ...
    m = _map(H, W, 9)
    ys, xs = np.mgrid[0:16, 0:24].astype(np.float32)
    m[0:16, 0:24, 0] = xs * np.float32(7.0 / 24)              # ... that the colour block [0,16) x [0,24) maps into
    m[0:16, 0:24, 1] = ys * np.float32(5.0 / 16)
    m[40:52, 60:82] = np.float32(-7.0)                        # a colour block that maps nowhere
    m[44, 70] = (np.nan, 3.0)
    table = np.random.default_rng(10).uniform(-0.8, 0.8, (DH, DW, 2)).astype(np.float32)
    net3.depth_upload(depth, body, m)
    net3.depth_set_camera_table(table)
    planes = depth_rule.align(depth, body, m)
    rois = [(10, 20, 11, 21), (30, 5, 31, 60), (3, 33, 90, 34), (0, 0, W, H), (17, 9, 80, 50), (20, 30, 83, 31),
            (1, 1, 23, 15), (61, 41, 81, 51)]
    boxes = [_box(*r, W, H) for r in rois]
    boxes.append(np.array([0.95, 0.1, 0.3, 0.5], np.float32))              # partly outside: clamped
    boxes.append(np.array([-0.05, 0.9, 0.4, 0.4], np.float32))
    boxes.append(np.array([1.4, 0.5, 0.2, 0.2], np.float32))               # entirely outside: invalid
    boxes.append(np.array([0.5, -0.6, 0.2, 0.2], np.float32))
    boxes.append(np.array([0.5, 0.5, 0.0, 0.3], np.float32))               # no width
    want = _check_boxes(net3, np.array(boxes), planes, table, rois + [None] * 5)
    assert want["valid"].tolist() == [1] * 10 + [0] * 3
    assert want[8]["right"] == W and want[9]["left"] == 0 and want[9]["bot"] == H
    assert (want["cam_z"][10:] == -1).all() and not want["left"][10:].any()
    zero, nowhere = want[6], want[7]
    assert zero["otsu"] == 0 and zero["mean_all_mm"] == 0 and zero["avg_mm"] == -16          # Otsu 0, the fallback mean
    assert nowhere["valid"] == 1 and not nowhere["pts"].any()                                 # point counts 0
    assert (want["otsu"][:6] > 0).any()
    net3.depth_set_camera_table(None)                        # without a table: (0, 0, -1, 0, 0)
    _check_boxes(net3, np.array(boxes), planes, None)


def test_depth_boxes_large_frame(net3):
    """a registered 640 x 480 frame with depth near 65535: 64-bit sums, several workgroups per box, every width around
    the wave and block sizes, the owner rule and a camera table with -inf entries under two points"""
    h, w = 480, 640
    rng = np.random.default_rng(12)
    depth = rng.integers(64000, 65536, (h, w)).astype(np.uint16)
    depth[100:260, 300:500] = rng.integers(500, 4000, (160, 200)).astype(np.uint16)          # an object in front
    depth[400:440, 20:120] = 0
    body = np.full((h, w), 255, np.uint8)
    body[10:20, 10:15] = 3                                    # ROI A [10,20) x [10,20): label 3 on exactly 50 of 100
    body[10:20, 30:35] = 4; body[10, 35] = 4                  # ROI B [10,20) x [30,40): 51 of 100
    body[30:40, 10:16] = 2; body[30:40, 16:19] = 5            # ROI C: 60 x label 2, 30 x label 5
    body[30:40, 30:34] = 6; body[30:35, 34:39] = 1; body[35:39, 34:39] = 1                   # ROI D: 40 x 6, 45 x 1
    body[50:60, 10:15] = 5; body[50:60, 15:20] = 2            # ROI E: a tie of 50 : 50 (lower label, not belonging)
    rois = [(10, 10, 20, 20), (30, 10, 40, 20), (10, 30, 20, 40), (30, 30, 40, 40), (10, 50, 20, 60),
            (0, 0, w, h),                                     # the whole frame: sum > 2^31
            (5, 7, 68, 50), (100, 90, 164, 130), (200, 3, 265, 44), (250, 80, 507, 300),      # widths 63, 64, 65, 257
            (0, 200, w, 201), (639, 0, 640, h), (30, 405, 100, 430)]
    boxes = np.array([_box(*r, w, h) for r in rois])
    net3.depth_upload(depth, body, None)
    planes = depth_rule.align(depth, body, None)
    free = depth_rule.as_records([depth_rule.box_stats(b, *planes, None) for b in boxes], darknet.DET3D_DTYPE)
    assert int(planes[0].astype(np.int64).sum()) > 2 ** 31 and free[5]["mean_all_mm"] > 50000
    assert free["belongs"][:5].tolist() == [0, 1, 1, 0, 0] and free["body_id"][:5].tolist() == [255, 4, 2, 255, 255]
    assert free[12]["otsu"] == 0 and (free["otsu"][[5, 9]] > 0).all()
    table = rng.uniform(-0.7, 0.7, (h, w, 2)).astype(np.float32)
    cx, cy = (int(np.float32(v) + np.float32(0.5)) for v in free[7]["pts"][0])
    lx, ly = (int(np.float32(v) + np.float32(0.5)) for v in free[8]["pts"][3])
    table[cy, cx, 1] = -np.inf                                # under box 7's centre: the (0, 0, -1) branch
    table[ly, lx, 0] = -np.inf                                # under box 8's left point: an infinite width, as the reference
    net3.depth_set_camera_table(table)
    want = _check_boxes(net3, boxes, planes, table, rois)
    assert (want[7]["cam_x"], want[7]["cam_y"], want[7]["cam_z"]) == (0, 0, -1)
    assert np.isinf(want[8]["cam_w"]) and np.isfinite(want[9]["cam_w"]) and want[9]["cam_z"] > 0
    net3.depth_set_camera_table(None)


# ---------------------------------------------------------------------------
# behind the detect chain
# ---------------------------------------------------------------------------
def _scene(seed):
    depth, body = _depth(seed)
    m = _map(H, W, seed + 1)
    table = np.random.default_rng(seed + 2).uniform(-0.8, 0.8, (DH, DW, 2)).astype(np.float32)
    return depth, body, m, table


@pytest.mark.parametrize("letterbox", [False, True])
def test_detect_regions_depth(net3, letterbox):
    thresh, nms = 0.05, 0.4
    depth, body, m, table = _scene(20)
    net3.depth_upload(depth, body, m)
    net3.depth_set_camera_table(table)
    d8 = depth_rule.align(depth, body, m)[1]
    items = [(FRAME, r) for r in RECTS]
    white = [(depth_rule.whiten(FRAME, r, d8, f), r) for r, f in zip(RECTS, FAR)]
    want, wc = net3.detect_regions(white, thresh, nms, swap_rb=True, letterbox=letterbox)
    got, d3, gc = net3.detect_regions_depth(items, FAR, thresh, nms, swap_rb=True, letterbox=letterbox)
    assert np.array_equal(gc, wc) and int(gc.sum()) > 0
    for i in range(3):
        assert got[i].tobytes() == want[i].tobytes(), "item %d" % i
        # the statistics of the boxes as returned: the device mapped them into the frame itself, and used the same ROI
        if len(got[i]):
            host = net3.depth_boxes(np.stack([got[i][k] for k in ("x", "y", "w", "h")], axis=-1))
            _same(d3[i], host)
            for b, s in zip(got[i], d3[i]):
                v, left, top, right, bot = depth_rule.roi((b["x"], b["y"], b["w"], b["h"]), W, H)
                assert s["valid"] == v
                if v:
                    assert (s["left"], s["top"], s["right"], s["bot"]) == (left, top, right, bot)
    assert sum(int(s["valid"].sum()) for s in d3) > 0
    # without a filter it is y2_detect_regions
    plain_d, plain_c = net3.detect_regions(items, thresh, nms, swap_rb=True, letterbox=letterbox)
    nd, _, nc = net3.detect_regions_depth(items, None, thresh, nms, swap_rb=True, letterbox=letterbox)
    assert np.array_equal(nc, plain_c) and all(a.tobytes() == b.tobytes() for a, b in zip(nd, plain_d))
    net3.depth_set_camera_table(None)


def test_detect_regions_depth_many_boxes(net3):
    """more detections than the prefix of records that is fetched before the counts are known: the second copy"""
    depth, body, m, table = _scene(40)
    net3.depth_upload(depth, body, m)
    net3.depth_set_camera_table(table)
    items = [(FRAME, r) for r in RECTS]
    got, d3, gc = net3.detect_regions_depth(items, FAR, 0.0005, 0.9)
    assert int(gc.sum()) > 300 and [len(g) for g in got] == gc.tolist()
    for i in range(3):
        _same(d3[i], net3.depth_boxes(np.stack([got[i][k] for k in ("x", "y", "w", "h")], axis=-1)))
    # a capacity below the count: the first max_per_item records of every item
    few, f3, fc = net3.detect_regions_depth(items, FAR, 0.0005, 0.9, max_per_item=5)
    assert np.array_equal(fc, gc)
    for i in range(3):
        assert few[i].tobytes() == got[i][:5].tobytes()
        _same(f3[i], d3[i][:5])
    net3.depth_set_camera_table(None)


def _native_scene(workdir):
    from tests.helpers import load_golden, materialize
    g = load_golden("mini_64_b3")
    cfg, wts, _ = materialize(workdir, "mini", 64, 3, int(g["seed"]), float(g["head_gain"]), tag="depthc")
    depth, body, m, table = _scene(30)
    frame = np.ascontiguousarray(FRAME[:, :, :3])
    fpath, dpath = os.path.join(workdir, "depth_frame.u8"), os.path.join(workdir, "depth_scene.bin")
    with open(fpath, "wb") as f:
        np.array(frame.shape, dtype=np.int32).tofile(f)
        frame.tofile(f)
    with open(dpath, "wb") as f:
        np.array(depth.shape, dtype=np.int32).tofile(f)
        for a in (depth, body, m, table):
            np.ascontiguousarray(a).tofile(f)
    args = []
    for r, far in zip(RECTS[1:], FAR[1:]):
        args += [str(v) for v in r] + [repr(far)]
    return cfg, wts, frame, (depth, body, m, table), [fpath, dpath], args


def test_detector_detect_regions_depth_cpp_caller(workdir):
    """Detector::upload_depth / set_camera_table / detect_regions_depth: the depth fields equal the C API's for the same
    call (strict mode), the pixel boxes are the C API's boxes through the class's own truncation (cpp:229-235), and
    without far_m the boxes are detect_regions'"""
    cfg, wts, frame, (depth, body, m, table), paths, args = _native_scene(workdir)
    thresh = 0.05
    exe = build(workdir, "detector_depth", "g++", "detector_depth.cpp", ["-std=c++11"])
    out = subprocess.run([exe, cfg, wts] + paths + [repr(thresh)] + args, capture_output=True, text=True, timeout=600, check=True,
                         env=dict(os.environ, Y2_STRICT="1")).stdout.splitlines()
    boxes = [l.split()[1:] for l in out if l.startswith("BOX ")]
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    net.depth_set_camera_table(table)
    net.depth_upload(depth, body, m)
    dets, d3, counts = net.detect_regions_depth([(frame, r) for r in RECTS], FAR, thresh, 0.1, swap_rb=True, letterbox=False)
    want = [(i, d, s) for i in range(3) for d, s in zip(dets[i], d3[i])]
    assert len(boxes) == len(want) > 0 and "UNFILTERED_EQUALS_DETECT_REGIONS 1" in out
    for o, (i, d, s) in zip(boxes, want):
        x, y, w, h = (np.float64(d[k]) for k in ("x", "y", "w", "h"))
        px = [int(max(0.0, (x - w / 2.) * W)), int(max(0.0, (y - h / 2.) * H)), int(np.float32(d["w"]) * np.float32(W)),
              int(np.float32(d["h"]) * np.float32(H))]
        assert [int(o[0]), int(o[1])] == [i, int(d["obj_id"])] and np.float32(float(o[2])) == d["prob"]
        assert [int(v) for v in o[3:7]] == px, (o, px)
        assert [int(o[7]), int(o[14]), int(o[15]), int(o[16])] == [int(s["valid"]), int(s["otsu"]), int(s["belongs"]), int(s["body_id"])]
        assert np.array_equal(np.array([float(v) for v in o[8:14]], np.float32),
                              np.array([s[k] for k in ("cam_x", "cam_y", "cam_z", "cam_w", "cam_h", "avg_mm")], np.float32), equal_nan=True)
    net.free()


def test_test_detector_regions_depth_c_caller(workdir):
    """test_detector_regions_depth from a C program written like the Kinect application: the objects' box, class and
    eight depth fields equal the Python path's"""
    cfg, wts, frame, (depth, body, m, table), paths, args = _native_scene(workdir)
    thresh = 0.05
    exe = build(workdir, "kinect_depth_like", "gcc", "kinect_depth_like.c")
    out = subprocess.run([exe, cfg, wts] + paths + [repr(thresh)] + args, capture_output=True, text=True, timeout=600,
                         check=True, env=dict(os.environ, Y2_STRICT="1")).stdout.splitlines()
    objs = [l.split()[1:] for l in out if l.startswith("OBJ ")]
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    net.depth_set_camera_table(table)
    net.depth_upload(depth, body, m)
    dets, d3, counts = net.detect_regions_depth([(frame, r) for r in RECTS], FAR, thresh, 0.1, swap_rb=True, letterbox=False)
    want = []
    for i in range(3):
        for d, s in zip(dets[i], d3[i]):
            want.append((i, int(d["obj_id"]), "class%d" % d["obj_id"]) +
                        tuple(np.float32(v) for v in (d["prob"], d["x"], d["y"], d["w"], d["h"], s["cam_x"], s["cam_y"], s["cam_z"],
                                                      s["cam_w"], s["cam_h"])) + (int(s["belongs"]), int(s["body_id"])))
    assert ("COUNTS %d %d %d" % tuple(counts)) in out and len(objs) == len(want) > 0
    for o, wv in zip(objs, want):
        assert (int(o[0]), int(o[1]), o[2]) == wv[:3] and (int(o[13]), int(o[14])) == wv[13:]
        assert np.array_equal(np.array([float(v) for v in o[3:13]], np.float32), np.array(wv[3:13], np.float32), equal_nan=True), (o, wv)
    net.free()
