"""CPU-only checks of the depth stage (y2_depth_* / y2_ingest_regions_depth / y2_detect_regions_depth /
test_detector_regions_depth): the library exports it, the Python mirrors have the C layouts, the Otsu threshold and the
ROI arithmetic -- the very code the kernels compile, include/y2_depth_rule.h -- equal the numpy restatement in
tests/depth_rule.py, and every refusal that needs no device comes before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import depth_rule
from tests.helpers import materialize

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_library_exports_the_depth_entries():
    L = darknet.lib()
    for name in ("y2_depth_upload", "y2_depth_set_camera_table", "y2_depth_aligned", "y2_depth_boxes", "y2_otsu_threshold",
                 "y2_depth_roi", "y2_ingest_regions_depth", "y2_detect_regions_depth", "test_detector_regions_depth",
                 "y2h_depth_align", "y2h_depth_boxes", "y2h_regions_to_input_filtered"):
        assert hasattr(L, name), name


def test_struct_layouts_match_c(workdir):
    src = os.path.join(workdir, "depth_layout.c")
    exe = os.path.join(workdir, "depth_layout")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sr_yolo2.h"\n#include "y2_hip.h"\nint main(void) {\n')
        for cname, cls in (("y2_det3d", darknet.Det3d), ("y2_depth_frame", darknet.DepthFrame)):
            f.write('    printf("%%zu\\n", sizeof(%s));\n' % cname)
            for name, _ in cls._fields_:
                f.write('    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, name))
        f.write('    printf("%zu\\n", sizeof(y2h_det3d));\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    want = []
    for cls in (darknet.Det3d, darknet.DepthFrame):
        want += [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
    assert got[:-1] == want
    assert got[-1] == C.sizeof(darknet.Det3d) == darknet.DET3D_DTYPE.itemsize
    assert [darknet.DET3D_DTYPE.fields[n][1] for n, _ in darknet.Det3d._fields_] == [getattr(darknet.Det3d, n).offset
                                                                                      for n, _ in darknet.Det3d._fields_]


def _hist(**bins):
    h = np.zeros(256, np.int64)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def _otsu_cases():
    rng = np.random.default_rng(5)
    cases = []
    for k in range(24):                                       # random: dense, sparse, with and without a bin-0 share
        h = rng.integers(0, 400, 256)
        if k % 3 == 1:
            h[rng.random(256) < 0.9] = 0
        if k % 2:
            h[0] = int(h[1:].sum() * rng.uniform(0, 5))
        cases.append(("random%d" % k, h))
    for k in range(6):                                        # smooth two-mode depth histograms, as a box over an object gives
        x = np.arange(256)
        a, b = rng.integers(20, 110), rng.integers(130, 250)
        h = (900 * np.exp(-((x - a) / 6.) ** 2) + 500 * np.exp(-((x - b) / 11.) ** 2)).astype(np.int64)
        h[0] = rng.integers(0, 3000)
        cases.append(("modes%d" % k, h))
    cases.append(("all in bin 0", _hist(b0=1000)))
    cases.append(("empty", np.zeros(256, np.int64)))
    # hist[0] against 0.85 * n, n = 2000: 1700 is not above, 1701 is
    cases.append(("bin 0 at 85%", _hist(b0=1700, b40=200, b90=100)))
    cases.append(("bin 0 just above 85%", _hist(b0=1701, b40=199, b90=100)))
    cases.append(("bin 0 just below 85%", _hist(b0=1699, b40=201, b90=100)))
    # one occupied bin: one class is empty on one side for every i (0/0 = NaN, the comparison is false)
    cases.append(("single bin", _hist(b77=500)))
    cases.append(("single bin 255", _hist(b255=3)))
    cases.append(("single bin 1", _hist(b0=10, b1=90)))
    # two equal peaks: every i between them gives the same variance, the strict > keeps the lowest
    cases.append(("two equal peaks", _hist(b50=300, b180=300)))
    cases.append(("two equal peaks, adjacent", _hist(b50=300, b51=300)))
    cases.append(("three equal peaks", _hist(b10=128, b100=128, b200=128)))
    return cases


@pytest.mark.parametrize("name,hist", _otsu_cases(), ids=[c[0] for c in _otsu_cases()])
def test_otsu_threshold_equals_the_rule(name, hist):
    assert darknet.otsu_threshold(hist) == depth_rule.otsu(hist)


def test_otsu_threshold_known_answers():
    """the rule itself, on cases whose answer follows from the reference's text"""
    assert depth_rule.otsu(_hist(b0=1000)) == 0               # :1588
    assert depth_rule.otsu(_hist(b0=1701, b40=199, b90=100)) == 0
    assert depth_rule.otsu(_hist(b0=1700, b40=200, b90=100)) == 40      # first i that separates the two bins
    assert depth_rule.otsu(_hist(b50=300, b180=300)) == 50
    assert depth_rule.otsu(_hist(b77=500)) == 0               # NaN for every i: deltaMax is never exceeded


def test_roi_equals_the_rule():
    rng = np.random.default_rng(11)
    boxes = [tuple(b) for b in rng.random((200, 4), dtype=np.float32)]
    boxes += [tuple(b) for b in (rng.random((100, 4), dtype=np.float32) * 3 - 1)]       # partly and wholly outside
    boxes += [(0.5, 0.5, 1.0, 1.0), (0.5, 0.5, 0.0, 0.0), (-0.2, 0.5, 0.1, 0.1), (1.3, 0.5, 0.1, 0.1), (0.5, 0.5, -0.3, 0.2),
              (0.25, 0.25, 1 / 96, 1 / 64), (np.nan, 0.5, 0.1, 0.1), (0.5, 0.5, np.inf, 0.1), (1e30, 0.5, 0.1, 0.1),
              (-1e30, 0.5, 0.1, 0.1)]
    valid = 0
    for W, H in ((96, 64), (97, 64), (640, 480), (1920, 1080)):
        for b in boxes:
            got = darknet.depth_roi(b, W, H)
            assert got == depth_rule.roi(b, W, H), (b, W, H)
            valid += got[0]
    assert 0 < valid < 4 * len(boxes)
    assert darknet.depth_roi((0.5, 0.5, 1.0, 1.0), 96, 64) == (1, 0, 0, 96, 64)
    assert darknet.depth_roi((1.3, 0.5, 0.1, 0.1), 96, 64)[0] == 0


def _frame(h, w, c, seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


def test_refusals_come_before_device_work(workdir):
    cfg, _, _ = materialize(workdir, "mini", 64, 3, 3)
    net = darknet.Network.parse_network_cfg(cfg)
    L = darknet.lib()
    frame = _frame(64, 96, 3)
    items = [(frame, None), (frame, (10, 8, 40, 30)), (frame, (50, 20, 30, 30))]
    arr, keep = darknet.regions(items)
    far = np.array([0, 0.9, 1.1], np.float32)
    dets = np.zeros((3, 8), dtype=darknet.DET_DTYPE)
    d3 = np.zeros((3, 8), dtype=darknet.DET3D_DTYPE)
    counts = np.zeros(3, np.int32)

    def ingest(a, f):
        assert L.y2_ingest_regions_depth(net.net, a, 3, darknet._ptr(f), 1, 0) != 0
        return darknet._check()

    def detect(a, f):
        assert L.y2_detect_regions_depth(net.net, a, 3, darknet._ptr(f) if f is not None else None, 1, 0, 0.2, 0.4,
                                         darknet._ptr(dets), darknet._ptr(d3), darknet._ptr(counts), 8) != 0
        return darknet._check()

    # no depth frame has been uploaded: a filtered ingest, and any depth detect, are refused
    for msg in (ingest(arr, far), detect(arr, far), detect(arr, None)):
        assert "depth" in msg and "upload" in msg, msg
    # what y2_ingest_regions refuses is refused here too, naming the item
    bad, keep2 = darknet.regions([items[0], (frame, (90, 0, 30, 10)), items[2]])
    for msg in (ingest(bad, far), detect(bad, far)):
        assert "item 1" in msg, msg
    # missing outputs
    assert L.y2_detect_regions_depth(net.net, arr, 3, darknet._ptr(far), 1, 0, 0.2, 0.4, darknet._ptr(dets), None,
                                     darknet._ptr(counts), 8) != 0
    assert "d3" in darknet._check()
    # the depth entries themselves: geometry that cannot be right
    depth = np.zeros((24, 32), np.uint16)
    f = darknet.DepthFrame(depth.ctypes.data, None, None, 24, 32, 64, 96)       # no map, yet another size
    assert L.y2_depth_upload(net.net, C.byref(f)) != 0
    assert "map" in darknet._check()
    f = darknet.DepthFrame(None, None, None, 24, 32, 24, 32)
    assert L.y2_depth_upload(net.net, C.byref(f)) != 0
    assert "depth" in darknet._check()
    boxes = np.zeros((1, 4), np.float32)
    out = np.zeros(1, darknet.DET3D_DTYPE)
    assert L.y2_depth_boxes(net.net, darknet._ptr(boxes), 1, darknet._ptr(out)) != 0
    assert "upload" in darknet._check()
    assert L.y2_depth_aligned(net.net, None, None, None) != 0
    assert "upload" in darknet._check()
    net.free()


def test_filter_refuses_a_frame_without_colour(workdir):
    """c < 3 on a filtered item (reachable on a one-channel network; a 3-channel one refuses c < net.c first)"""
    cfg, _, _ = materialize(workdir, "mini", 64, 2, 3)
    gray = os.path.join(workdir, "mini_gray.cfg")
    with open(cfg) as src, open(gray, "w") as dst:
        text = src.read()
        assert "channels=3" in text
        dst.write(text.replace("channels=3", "channels=1"))
    net = darknet.Network.parse_network_cfg(gray)
    arr, keep = darknet.regions([(_frame(64, 96, 3), None), (_frame(64, 96, 1), (4, 4, 20, 20))])
    far = np.array([0, 0.8], np.float32)
    assert darknet.lib().y2_ingest_regions_depth(net.net, arr, 2, darknet._ptr(far), 1, 0) != 0
    msg = darknet._check()
    assert "item 1" in msg and "channel" in msg, msg
    net.free()


def test_depth_callers_compile_and_link(workdir):
    """No GPU needed: the C caller of test_detector_regions_depth and the C++ caller of Detector::detect_regions_depth
    build against include/ and resolve every symbol."""
    from tests.test_native_callers import build
    build(workdir, "kinect_depth_like", "gcc", "kinect_depth_like.c")
    build(workdir, "detector_depth", "g++", "detector_depth.cpp", ["-std=c++11"])
