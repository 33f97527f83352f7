"""CPU-only checks of the batched-regions entry (y2_ingest_regions / y2_detect_regions / test_detector_regions): the
library exports it, the Python mirror of y2_region has the C layout, every refusal happens before any device work
(so it is seen here, without a GPU) and names the item, and the box mapping back into each item's frame follows the
formulas of include/sr_yolo2.h step by step in fp32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests.conftest import has_gpu
from tests.helpers import materialize

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_library_exports_the_region_entries():
    L = darknet.lib()
    for name in ("y2_ingest_regions", "y2_detect_regions", "test_detector_regions", "y2_region_box_to_frame",
                 "y2h_regions_to_input"):
        assert hasattr(L, name), name


def test_region_struct_layout_matches_c(workdir):
    src = os.path.join(workdir, "region_layout.c")
    exe = os.path.join(workdir, "region_layout")
    fields = [f for f, _ in darknet.Region._fields_]
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sr_yolo2.h"\nint main(void) {\n')
        f.write('    printf("%zu\\n", sizeof(y2_region));\n')
        for name in fields:
            f.write('    printf("%%zu\\n", offsetof(y2_region, %s));\n' % name)
        f.write("    return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", INCLUDE, src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(darknet.Region)
    assert got[1:] == [getattr(darknet.Region, name).offset for name in fields]


def _net(workdir, batch=3):
    cfg, wts, _ = materialize(workdir, "mini", 64, batch, 3)
    net = darknet.Network.parse_network_cfg(cfg)
    return net


def _frame(h, w, c, seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


GOOD = [(_frame(90, 120, 3), (10, 20, 37, 53)), (_frame(64, 64, 3, 2), None), (_frame(50, 40, 4, 3), (0, 0, 40, 50))]


def _refuse(net, items, n=None, letterbox=False, detect=False):
    arr, keep = darknet.regions(items)
    n = len(items) if n is None else n
    L = darknet.lib()
    if detect:
        dets = np.zeros((4, 8), dtype=darknet.DET_DTYPE)
        counts = np.zeros(4, np.int32)
        rc = L.y2_detect_regions(net.net, arr, n, 1, int(letterbox), 0.2, 0.4, darknet._ptr(dets), darknet._ptr(counts), 8)
    else:
        rc = L.y2_ingest_regions(net.net, arr, n, 1, int(letterbox))
    assert rc != 0
    return darknet._check()


@pytest.mark.parametrize("detect", [False, True])
def test_refusals_name_the_item_and_come_before_device_work(workdir, detect):
    net = _net(workdir)
    cases = []                                                  # (items, letterbox, what the message names)
    cases.append(([GOOD[0], GOOD[1], (_frame(10, 10, 2), None)], False, "item 2"))                  # c < net.c
    cases.append(([GOOD[0], (_frame(90, 120, 3), (100, 0, 30, 10))], False, "item 1"))              # x + rw > w
    cases.append(([(_frame(90, 120, 3), (0, 85, 10, 10))], False, "item 0"))                        # y + rh > h
    cases.append(([GOOD[1], (_frame(90, 120, 3), (-1, 0, 10, 10))], False, "item 1"))               # x < 0
    cases.append(([GOOD[1], GOOD[0], (_frame(90, 120, 3), (0, 0, 0, 5))], False, "item 2"))         # rw < 1
    cases.append(([GOOD[1], (_frame(90, 120, 3), (3, 0, 0, 0))], False, "item 1"))                  # whole frame with x != 0
    cases.append(([GOOD[0], (_frame(1, 900, 3), None)], True, "item 1"))                             # degenerate letterbox
    for items, lb, frag in cases:
        msg = _refuse(net, items, letterbox=lb, detect=detect)
        assert frag in msg, msg
        assert "regions" in msg
    # n outside [1, net.batch]
    for n in (0, 4):
        msg = _refuse(net, GOOD + [GOOD[0]], n=n, detect=detect)
        assert "batch-3" in msg, msg
    # NULL data and step < w*c, written straight into the C structs
    L = darknet.lib()
    arr, keep = darknet.regions(GOOD)
    arr[1].data = None
    fn = L.y2_ingest_regions
    assert fn(net.net, arr, 3, 1, 0) != 0
    msg = darknet._check()
    assert "item 1" in msg and "NULL" in msg, msg
    arr, keep = darknet.regions(GOOD)
    arr[2].step = arr[2].w * arr[2].c - 1
    assert fn(net.net, arr, 3, 1, 0) != 0
    msg = darknet._check()
    assert "item 2" in msg and "step" in msg, msg
    # the network is still usable: the same valid call is refused by nothing but the absence of a device
    if not has_gpu():
        arr, keep = darknet.regions(GOOD)
        assert fn(net.net, arr, 3, 1, 0) != 0
        msg = darknet._check()
        assert "item" not in msg and "device" in msg.lower(), msg
    net.free()


def test_detect_regions_refuses_missing_outputs(workdir):
    net = _net(workdir)
    arr, keep = darknet.regions(GOOD)
    counts = np.zeros(3, np.int32)
    assert darknet.lib().y2_detect_regions(net.net, arr, 3, 1, 0, 0.2, 0.4, None, darknet._ptr(counts), 8) != 0
    assert "y2_detect_regions" in darknet._check()
    with pytest.raises(darknet.Y2Error, match="item 0"):
        net.detect_regions([(_frame(8, 8, 3), (4, 4, 8, 8))], 0.2, 0.4)
    with pytest.raises(darknet.Y2Error, match="item 0"):
        net.ingest_regions([(_frame(8, 8, 1), None)])
    net.free()


def letterbox_dims(iw, ih, w, h):
    """image.c:1607-1618 (float comparison, integer sizes)"""
    if np.float32(w) / np.float32(iw) < np.float32(h) / np.float32(ih):
        return w, (ih * w) // iw
    return (iw * h) // ih, h


def map_box(frame_hw, rect, net_w, net_h, letterbox, box):
    """numpy float32 restatement of y2_region_box_to_frame (include/sr_yolo2.h)"""
    f32 = np.float32
    H, W = frame_hw
    rx, ry, rw, rh = rect if rect is not None and (rect[2] or rect[3]) else (0, 0, W, H)
    x, y, w, h = (f32(v) for v in box)
    if letterbox:
        nw, nh = letterbox_dims(rw, rh, net_w, net_h)
        x = (x * f32(net_w) - f32((net_w - nw) // 2)) / f32(nw)
        y = (y * f32(net_h) - f32((net_h - nh) // 2)) / f32(nh)
        w = w * f32(net_w) / f32(nw)
        h = h * f32(net_h) / f32(nh)
    if (rx, ry, rw, rh) != (0, 0, W, H):
        x = (x * f32(rw) + f32(rx)) / f32(W)
        y = (y * f32(rh) + f32(ry)) / f32(H)
        w = w * f32(rw) / f32(W)
        h = h * f32(rh) / f32(H)
    return np.array([x, y, w, h], dtype=np.float32)


@pytest.mark.parametrize("frame_hw,rect,letterbox", [
    ((480, 640), (400, 120, 200, 210), False),        # a hand crop
    ((480, 640), (13, 7, 1, 90), False),              # one pixel wide
    ((480, 640), (100, 50, 60, 200), True),           # letterboxed tall region
    ((480, 640), (100, 50, 300, 90), True),           # letterboxed wide region
    ((480, 640), None, False),                        # whole frame: unchanged
    ((480, 640), (0, 0, 640, 480), False),            # the same, spelled out
    ((480, 640), None, True),                         # whole frame, letterboxed
])
def test_box_mapping_matches_numpy(frame_hw, rect, letterbox):
    rng = np.random.default_rng(17)
    frame = np.zeros(frame_hw + (3,), np.uint8)
    for net_w, net_h in ((416, 416), (64, 64), (608, 320)):
        for box in rng.random((64, 4), dtype=np.float32):
            got = darknet.region_box_to_frame((frame, rect), net_w, net_h, letterbox, box)
            want = map_box(frame_hw, rect, net_w, net_h, letterbox, box)
            assert got.tobytes() == want.tobytes(), (box, got, want)
            if rect is None and not letterbox:
                assert got.tobytes() == np.asarray(box, np.float32).tobytes()


def test_region_callers_compile_and_link(workdir):
    """No GPU needed: the C caller of test_detector_regions and the C++ caller of Detector::detect_regions build against
    include/ (with the reference's header names) and resolve every symbol."""
    from tests.test_native_callers import build
    build(workdir, "regions_like", "gcc", "regions_like.c")
    build(workdir, "detector_regions", "g++", "detector_regions.cpp", ["-std=c++11"])
