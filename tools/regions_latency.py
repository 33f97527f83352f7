#!/usr/bin/env python3
"""What batching the Kinect loop's three detector calls saves (whole 640x480 colour frame + two hand crops of about
200x200 per camera frame, KinectUtil_with_cam.cpp:1029-1110).

  (a) three sequential batch-1 y2_detect_u8 calls, the crops copied on the host first (as the application does)
  (b) one y2_detect_regions call with the same three items on a batch-3 network
  (c) one y2_detect_regions call with ONE item (the whole frame) on the same batch-3 network: the full planned batch
      still runs, so this is the price of the padded slots, next to (d)
  (d) one batch-1 y2_detect_u8 call on the whole frame

usage: regions_latency.py [--net tiny-yolo-voc] [--size 416] [--iters 200] [--warmup 20] [--graph]
Prints p50 / p90 wall-clock ms per case (timed with gc disabled, as bench.py does) and one JSON line."""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

CROPS = [(60, 200, 200, 200), (410, 180, 190, 210)]        # (x, y, w, h) of the two hand crops in the 640x480 frame


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    gc.collect()
    gc.disable()
    try:
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    finally:
        gc.enable()
    ms = 1e3 * np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ms, 50)), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="tiny-yolo-voc")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--graph", action="store_true", help="replay each forward pass from a hipGraph (y2_set_graph)")
    ap.add_argument("--thresh", type=float, default=0.24)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    tmp = tempfile.mkdtemp()
    cfg = os.path.join(tmp, "n.cfg")
    open(cfg, "w").write(zoo.cfg_text(a.net, a.size, a.size, 1))
    wts = os.path.join(tmp, "n.weights")
    synth.write_weights(wts, zoo.resolve(a.net, a.size), 7)
    nets = {}
    for b in (1, 3):
        n = darknet.Network.parse_network_cfg(cfg)
        n.load_weights(wts)
        n.set_batch_network(b)
        n.set_graph(a.graph)
        nets[b] = n
    frame = np.random.default_rng(5).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    items = [(frame, None)] + [(frame, r) for r in CROPS]
    nms = 0.1

    def sequential():
        nets[1].detect_u8(frame[None], a.thresh, nms)
        for x, y, w, h in CROPS:
            crop = np.ascontiguousarray(frame[y:y + h, x:x + w])[None]
            nets[1].detect_u8(crop, a.thresh, nms)

    res = {
        "a_three_batch1_detect_u8": timed(sequential, a.iters, a.warmup),
        "b_one_detect_regions_b3": timed(lambda: nets[3].detect_regions(items, a.thresh, nms), a.iters, a.warmup),
        "c_detect_regions_n1_on_b3": timed(lambda: nets[3].detect_regions(items[:1], a.thresh, nms), a.iters, a.warmup),
        "d_one_batch1_detect_u8": timed(lambda: nets[1].detect_u8(frame[None], a.thresh, nms), a.iters, a.warmup),
    }
    print("%s %dx%d, %d timed calls after %d warm-up%s (wall-clock ms):" % (a.net, a.size, a.size, a.iters, a.warmup,
                                                                             ", forward replayed from a hipGraph" if a.graph else ""))
    for k, v in res.items():
        print("  %-28s p50 %8.3f   p90 %8.3f" % (k, v["p50_ms"], v["p90_ms"]))
    sa, sb = res["a_three_batch1_detect_u8"]["p50_ms"], res["b_one_detect_regions_b3"]["p50_ms"]
    print(json.dumps({"net": a.net, "size": a.size, "graph": a.graph, "iters": a.iters, "device": darknet.device_name(),
                      "speedup_p50_a_over_b": round(sa / sb, 3), **res}))
    for n in nets.values():
        n.free()


if __name__ == "__main__":
    main()
