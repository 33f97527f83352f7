#!/usr/bin/env python3
"""What the depth stage of the Kinect loop costs on the device (y2_depth_upload, and y2_detect_regions_depth over
y2_detect_regions), at the Kinect's shapes: colour 1920x1080 BGRA, depth 512x424, three items (the whole frame and two
hand crops, KinectUtil_with_cam.cpp:1003-1118), about 20 boxes from a synthetic-weights tiny-yolo-voc.

Every time is measured between two events on the engine's stream (y2h_event_elapsed_ms), p50 / p90 of --iters calls after
--warmup.  Per kernel, the bytes it must stream and the GB/s that gives:
  align     8 B of map in + 8 B of planes out per colour pixel (the depth / body gathers hit a 0.65 MB frame in L2)
  clear     the accumulators of every box slot
  pass 1    4 B per ROI pixel (depth16, depth8, person)
  pass 2    7 B per ROI pixel (depth16, depth8, dx/dy)
  filter    the fused ingest, timed against the plain one: 1 B of depth8 per source tap of a filtered item

usage: depth_latency.py [--net tiny-yolo-voc] [--size 416] [--iters 200] [--warmup 20] [--boxes 20]"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

H, W, DH, DW = 1080, 1920, 424, 512
CROPS = [(300, 400, 544, 544), (1100, 380, 520, 560)]      # the two hand crops (544 / distance pixels on a side)
FAR = [0.0, 1.3, 1.4]                                      # jointDistance + 0.3


class Planes(C.Structure):     # include/y2_hip.h y2h_depth_planes
    _fields_ = [("depth16", C.c_void_p), ("depth8", C.c_void_p), ("person", C.c_void_p), ("dxy", C.c_void_p),
                ("cam_table", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("dh", C.c_int), ("dw", C.c_int),
                ("grasp16", C.c_void_p)]                   # NULL: the Demo_what statistics


class Timer:
    def __init__(self, L, stream):
        self.L, self.stream = L, stream
        self.a, self.b = C.c_void_p(), C.c_void_p()
        L.y2h_event_create(C.byref(self.a))
        L.y2h_event_create(C.byref(self.b))

    def ms(self, fn):
        self.L.y2h_event_record(self.a, self.stream)
        fn()
        self.L.y2h_event_record(self.b, self.stream)
        out = C.c_float()
        self.L.y2h_event_elapsed_ms(self.a, self.b, C.byref(out))
        return out.value

    def stats(self, fn, iters, warmup):
        for _ in range(warmup):
            fn()
        t = np.array([self.ms(fn) for _ in range(iters)])
        return {"p50_ms": round(float(np.percentile(t, 50)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4)}


    def stats_turns(self, fns, iters, warmup):
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        t = {k: [] for k in fns}
        for _ in range(iters):
            for k, fn in fns.items():
                t[k].append(self.ms(fn))
        return {k: {"p50_ms": round(float(np.percentile(v, 50)), 4), "p90_ms": round(float(np.percentile(v, 90)), 4)}
                for k, v in t.items()}


def dev_array(L, a):
    p = C.c_void_p()
    assert L.y2h_malloc(C.byref(p), a.nbytes) == 0
    assert L.y2h_memcpy_h2d(p, darknet._ptr(a), a.nbytes, None) == 0 and L.y2h_stream_sync(None) == 0
    return p


def scene():
    """a room: a far wall, a table, two people in front of it; the colour camera sees a little more than the depth one"""
    rng = np.random.default_rng(3)
    depth = (3200 + 300 * rng.random((DH, DW))).astype(np.uint16)
    depth[260:, :] = np.linspace(2400, 900, DH - 260).astype(np.uint16)[:, None]
    body = np.full((DH, DW), 255, np.uint8)
    for k, (x0, x1) in enumerate(((110, 190), (330, 400))):
        depth[90:380, x0:x1] = 1000 + 100 * k + (20 * rng.random((290, x1 - x0))).astype(np.uint16)
        body[90:380, x0:x1] = k + 1
    depth[rng.random((DH, DW)) < 0.03] = 0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.stack([(xs - 210) * np.float32(DW / 1500.), ys * np.float32(DH / H) + np.float32(0.3)], axis=-1).astype(np.float32)
    yy, xx = np.mgrid[0:DH, 0:DW].astype(np.float32)
    table = np.stack([(xx - DW / 2) / 365., (DH / 2 - yy) / 365.], axis=-1).astype(np.float32)
    return depth, body, m, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="tiny-yolo-voc")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=20)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    L = darknet.lib()
    L.y2h_depth_align.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 5
    L.y2h_depth_boxes.argtypes = [C.POINTER(Planes), C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.y2h_depth_acc_bytes.restype = C.c_ulong
    tmp = tempfile.mkdtemp()
    cfg, wts = os.path.join(tmp, "n.cfg"), os.path.join(tmp, "n.weights")
    open(cfg, "w").write(zoo.cfg_text(a.net, a.size, a.size, 1))
    synth.write_weights(wts, zoo.resolve(a.net, a.size), 7)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_batch_network(3)
    frame = np.random.default_rng(5).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    items = [(frame, None)] + [(frame, r) for r in CROPS]
    depth, body, m, table = scene()
    net.depth_set_camera_table(table)
    net.depth_upload(depth, body, m)
    # every call goes through the default capacity (max_per_item = l.w*l.h*l.n, what test_detector_regions_depth and
    # Detector::detect_regions_depth pass); the threshold is what brings the synthetic head down to about --boxes detections
    nms, cap = 0.1, None
    lo, hi = 0.01, 0.999999
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if int(net.detect_regions(items, mid, nms)[1].sum()) > a.boxes:
            lo = mid
        else:
            hi = mid
    thresh = hi
    dets, d3, counts = net.detect_regions_depth(items, FAR, thresh, nms)
    per_item = net.last.w * net.last.h * net.last.n
    roi_px = int(sum(int(((s["right"] - s["left"]) * (s["bot"] - s["top"])).sum()) for s in d3))
    tm = Timer(L, L.y2_stream(net.net))
    res = {}
    res["depth_upload"] = tm.stats(lambda: net.depth_upload(depth, body, m), a.iters, a.warmup)
    # the calls that are compared with each other take turns inside one loop, so that a drift of the host's pace (the
    # packing of the region rows into pinned memory lies between the two events) hits them alike
    res.update(tm.stats_turns({
        "detect_regions": lambda: net.detect_regions(items, thresh, nms),
        "detect_regions_depth_no_filter": lambda: net.detect_regions_depth(items, None, thresh, nms),
        "detect_regions_depth": lambda: net.detect_regions_depth(items, FAR, thresh, nms)}, a.iters, a.warmup))
    res.update(tm.stats_turns({"ingest_regions": lambda: net.ingest_regions(items),
                               "ingest_regions_depth": lambda: net.ingest_regions_depth(items, FAR)}, a.iters, a.warmup))
    # the kernels alone, on buffers of this tool's own
    npix = H * W
    d_depth, d_body, d_map, d_tab = (dev_array(L, x) for x in (depth, body, m, table))
    d16, d8, dper, dxy = (dev_array(L, np.zeros(npix * k, np.uint8)) for k in (2, 1, 1, 4))
    res["kernel_align"] = tm.stats(lambda: L.y2h_depth_align(d_depth, d_body, d_map, DH, DW, H, W, d16, d8, dper, dxy, tm.stream),
                                   a.iters, a.warmup)
    nb = int(sum(len(d) for d in dets))
    if nb:
        # the launch y2_detect_regions_depth makes: 3 x per_item slots, the boxes as the detect chain's records, counts on the device
        rec = np.zeros((3, per_item, 6), np.float32)
        for i, d in enumerate(dets):
            for k, f in enumerate(("x", "y", "w", "h")):
                rec[i, :len(d), k] = d[f]
        planes = Planes(d16, d8, dper, dxy, d_tab, H, W, DH, DW)
        d_rec, d_cnt = dev_array(L, rec), dev_array(L, np.array([len(d) for d in dets], np.int32))
        d_acc = dev_array(L, np.zeros(3 * per_item * L.y2h_depth_acc_bytes(), np.uint8))
        d_out = dev_array(L, np.zeros(3 * per_item, darknet.DET3D_DTYPE))
        for name, stages in (("kernels_boxes_all", 15), ("boxes_clear", 1), ("boxes_pass1", 2), ("boxes_pass2", 4), ("boxes_finalise", 8)):
            res[name] = tm.stats(lambda: L.y2h_depth_boxes(C.byref(planes), d_rec, 6, per_item, d_cnt, None, 3, per_item, d_acc, d_out,
                                                           stages, tm.stream), a.iters, a.warmup)
    extra = res["detect_regions_depth"]["p50_ms"] - res["detect_regions"]["p50_ms"]
    print("%s %dx%d, colour %dx%d BGRA, depth %dx%d, 3 items x %d box slots (the default max_per_item), %d boxes (thresh %.6f) covering"
          " %d ROI pixels; %d timed calls after %d warm-up (event ms on the engine's stream):"
          % (a.net, a.size, a.size, W, H, DW, DH, per_item, nb, thresh, roi_px, a.iters, a.warmup))
    for k, v in res.items():
        print("  %-32s p50 %8.4f   p90 %8.4f" % (k, v["p50_ms"], v["p90_ms"]))
    print("  detect_regions_depth over detect_regions at the same inputs: %+.4f ms p50 (of which the filter in the ingest %+.4f)"
          % (extra, res["ingest_regions_depth"]["p50_ms"] - res["ingest_regions"]["p50_ms"]))
    align_b = npix * 16
    print("  align kernel: %.1f MB streamed -> %.0f GB/s (the same buffers every call: the 256 MB Infinity Cache serves part of it)"
          % (align_b / 1e6, align_b / 1e6 / res["kernel_align"]["p50_ms"]))
    up_b = depth.nbytes + body.nbytes + m.nbytes
    print("  y2_depth_upload: %.1f MB host -> device, then the align kernel -> %.1f GB/s end to end" %
          (up_b / 1e6, up_b / 1e6 / res["depth_upload"]["p50_ms"]))
    if nb:
        acc_b = 3 * per_item * L.y2h_depth_acc_bytes()
        print("  clear: %.2f MB of accumulators -> %.0f GB/s" % (acc_b / 1e6, acc_b / 1e6 / res["boxes_clear"]["p50_ms"]))
        for name, per_px in (("boxes_pass1", 4), ("boxes_pass2", 7)):
            print("  %s: %.2f MB streamed (%d B per ROI pixel) -> %.0f GB/s" % (name[6:], roi_px * per_px / 1e6, per_px,
                                                                                roi_px * per_px / 1e6 / res[name]["p50_ms"]))
    print(json.dumps({"net": a.net, "size": a.size, "iters": a.iters, "device": darknet.device_name(), "boxes": nb, "roi_pixels": roi_px,
                      "extra_p50_ms": round(extra, 4), **res}))
    net.free()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
