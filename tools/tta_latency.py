#!/usr/bin/env python3
"""What building the classifier's evaluation views on the device saves (validate_classifier_10 / _multi,
classifier.c:336-406, :531-593).

Per image, on the same frames and weights:
  new     y2_classifier_view_sums over all frames at once: one upload per block, device resizes, one launch fills each
          forward's views, one launch adds its rows, one copy down per block; MULTI resizes the network once per
          distinct size
  loop    what a caller could write before: the views built in numpy (resize_image, slicing with clamped indices,
          [::-1]), network_predict at batch 1 per view, resize_network per image and scale, the sum on the host.  It
          uses only calls the library had before, so Y2_LIB=<an older build> runs it against that build (--loop-only).

Rows: darknet19 at 224, CROP10 on a batch-10 and on a batch-1 network, MULTI with the reference's five scales, fp32
and fp16, 64 synthetic frames of two aspect ratios.  `loop` is timed per image and reported as the p50 over the frames
after a warm-up pass over all of them; `new` is one call over all frames, repeated, p50 of (call time / frames).  Every
timed span ends in a host-visible result, i.e. behind a device synchronise.  Also printed: the plan rebuilds of each
path, the largest difference between the two paths' sums, and the bytes one y2h_views_to_input launch moves (for a
bandwidth figure from a kernel trace of --rows crop10_b10).

usage: tta_latency.py [--frames 64] [--repeats 5] [--rows crop10_b10,crop10_b1,multi] [--modes fp32,fp16] [--loop-only]"""
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

SIZE = 224
SCALES = (224, 288, 320, 352, 384)
SHIFTS = ((-32, -32), (32, -32), (0, 0), (-32, 32), (32, 32))
FRAME_SIZES = ((400, 300), (320, 480))                 # (w, h): 4:3 landscape and 2:3 portrait
CROP10, MULTI = 0, 1


def crop(im, dx, dy, w, h):
    r = np.clip(np.arange(h) + dy, 0, im.shape[1] - 1)
    c = np.clip(np.arange(w) + dx, 0, im.shape[2] - 1)
    return im[:, r[:, None], c[None, :]]


def resize_min_dims(w, h, m):
    return (m, (h * m) // w) if w < h else ((w * m) // h, m)


def loop_crop10(net, frame):
    im = frame if frame.shape[1:] == (SIZE + 32, SIZE + 32) else darknet.resize_image(frame, SIZE + 32, SIZE + 32)
    pred = np.zeros(net.output_size, np.float32)
    for src in (im, im[:, :, ::-1]):
        for dx, dy in SHIFTS:
            pred += net.network_predict(crop(src, dx, dy, SIZE, SIZE))
    return pred


def loop_multi(net, frame):
    pred = np.zeros(net.output_size, np.float32)
    for s in SCALES:
        rw, rh = resize_min_dims(frame.shape[2], frame.shape[1], s)
        r = frame if (rw, rh) == (frame.shape[2], frame.shape[1]) else darknet.resize_image(frame, rw, rh)
        net.resize_network(rw, rh)
        pred += net.network_predict(r)
        pred += net.network_predict(r[:, :, ::-1])
    return pred


def time_loop(fn, net, frames):
    for f in frames:                                   # the warm-up pass
        fn(net, f)
    ts, sums = [], []
    gc.collect()
    gc.disable()
    try:
        for f in frames:
            t0 = time.perf_counter()
            sums.append(fn(net, f))
            ts.append(time.perf_counter() - t0)
    finally:
        gc.enable()
    return 1e3 * np.asarray(ts), np.stack(sums)


def time_new(net, mode, frames, scales, repeats):
    net.classifier_view_sums(mode, frames, scales)     # the warm-up pass
    ts = []
    before = darknet.view_resizes()
    gc.collect()
    gc.disable()
    try:
        for _ in range(repeats):
            t0 = time.perf_counter()
            sums = net.classifier_view_sums(mode, frames, scales)
            ts.append((time.perf_counter() - t0) / len(frames))
    finally:
        gc.enable()
    return 1e3 * np.asarray(ts), sums, (darknet.view_resizes() - before) // repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", default="crop10_b10,crop10_b1,multi")
    ap.add_argument("--modes", default="fp32,fp16")
    ap.add_argument("--loop-only", action="store_true", help="time only the loop (for an older build named by Y2_LIB)")
    ap.add_argument("--new-only", action="store_true", help="time only the new path (for a kernel trace)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    wts = os.path.join(tmp, "d19.weights")
    synth.write_weights(wts, zoo.resolve("darknet19", SIZE), 41, 1.0)
    frames = [synth.uniform01(900 + i, 3 * h * w).reshape(3, h, w)
              for i, (w, h) in ((i, FRAME_SIZES[i % 2]) for i in range(a.frames))]
    print("darknet19 at %d, %d frames (%s), device %s" % (SIZE, a.frames, " / ".join("%dx%d" % s for s in FRAME_SIZES),
                                                          darknet.device_name()))
    print("one y2h_views_to_input launch at batch 10 moves %d bytes (4 read + 4 written per value)" % (10 * 3 * SIZE * SIZE * 8))
    out = []
    for half in [m == "fp16" for m in a.modes.split(",")]:
        for row in a.rows.split(","):
            mode = MULTI if row == "multi" else CROP10
            batch = {"crop10_b10": 10, "crop10_b1": 1, "multi": 2}[row]
            scales = SCALES if mode == MULTI else None
            res = {"row": row, "mode": "fp16" if half else "fp32", "batch": batch}
            nets = {}
            for b in {1, batch}:
                cfg = os.path.join(tmp, "d19_b%d.cfg" % b)
                open(cfg, "w").write(zoo.cfg_text("darknet19", SIZE, SIZE, b))
                n = darknet.Network.parse_network_cfg(cfg)
                n.load_weights(wts)
                n.set_half(half)
                nets[b] = n
            if not a.new_only:
                ms, loop_sums = time_loop(loop_multi if mode == MULTI else loop_crop10, nets[1], frames)
                if mode == MULTI:
                    nets[1].resize_network(SIZE, SIZE)
                res.update(loop_p50_ms=round(float(np.percentile(ms, 50)), 4), loop_p90_ms=round(float(np.percentile(ms, 90)), 4),
                           loop_rebuilds=a.frames * len(SCALES) if mode == MULTI else 0)
            if not a.loop_only:
                ms, new_sums, rebuilds = time_new(nets[batch], mode, frames, scales, a.repeats)
                res.update(new_p50_ms=round(float(np.percentile(ms, 50)), 4), new_max_ms=round(float(ms.max()), 4),
                           new_rebuilds=int(rebuilds))
                if not a.new_only:
                    res["max_abs_diff_of_sums"] = float(np.abs(new_sums - loop_sums).max())
                    res["same_top1"] = bool((new_sums.argmax(1) == loop_sums.argmax(1)).all())
                    res["speedup_p50"] = round(res["loop_p50_ms"] / res["new_p50_ms"], 2)
            for n in nets.values():
                n.free()
            print("  " + json.dumps(res))
            out.append(res)
    print(json.dumps({"tool": "tta_latency", "device": darknet.device_name(), "frames": a.frames, "rows": out}))


if __name__ == "__main__":
    main()
