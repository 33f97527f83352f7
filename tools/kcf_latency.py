#!/usr/bin/env python3
"""Latency of the batched KCF tracker (y2_kcf_init / y2_kcf_track) on a 1920 x 1080 BGRA frame, for 1, 5 and 27 trackers
with 80 x 80 and 200 x 300 boxes, beside test_detector_img's batch-1 latency from the same process as context.

    python tools/kcf_latency.py --out profiles/kcf_stage.txt
        host wall time per call (every call ends in a device synchronise), median and spread of --repeats calls after a
        warm-up of every shape
    rocprofv3 --kernel-trace --stats -d DIR -o kcf -- python tools/kcf_latency.py --loop 27 200x300 --repeats 20
    python tools/kcf_latency.py --stats DIR/.../kcf_kernel_stats.csv --calls 20 --out profiles/kcf_stage.txt --append
        device time per call and each stage's share of it (patch, fHOG, DFTs, element-wise), from a kernel trace taken in a
        run of its own: the loop makes one init and then `repeats` track(update=0) and `repeats` track(update=1) calls

Nothing here is a pass/fail number.  A run without a GPU fails; it does not fall back."""
import argparse
import csv
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920
STAGES = (("patch", ("kcf_patch",)), ("fHOG", ("kcf_grad", "kcf_hist", "kcf_norm", "kcf_chan")), ("DFTs", ("kcf_dft",)),
          ("element-wise", ("kcf_cross", "kcf_gauss", "kcf_train", "kcf_apply", "kcf_argmax")))


def frames():
    rng = np.random.default_rng(3)
    base = np.kron(rng.integers(0, 256, (H // 8, W // 8, 1)), np.ones((8, 8, 4), np.int64))
    f0 = (base + rng.integers(0, 24, (H, W, 4))).clip(0, 255).astype(np.uint8)
    return f0, np.roll(f0, (4, -8), axis=(0, 1))


def boxes(n, bw, bh):
    cols = 9
    return [(160.0 + 200 * (i % cols), 200.0 + 330 * (i // cols), float(bw), float(bh)) for i in range(n)]


def timed(fn, repeats):
    t = []
    for _ in range(repeats):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t), max(t)


def network(tmp, name="mini", size=32):
    from sr_object_detection_amd import darknet
    from tests.helpers import materialize
    cfg, wts, x = materialize(tmp, name, size, 1, 3)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    return net, x


def measure(args, out):
    from sr_object_detection_amd import darknet
    if darknet.device_count() < 1:
        sys.exit("kcf_latency: no HIP device visible")
    f0, f1 = frames()
    with tempfile.TemporaryDirectory() as tmp:
        net, _ = network(tmp)
        out.write("KCF tracker stage on %s: host wall time per call in ms (median, min .. max of %d calls after warm-up);\n"
                  "every call ends in a device synchronise.  Frame %d x %d BGRA.\n\n" % (darknet.device_name(), args.repeats, W, H))
        out.write("%-9s %-9s %-24s %-24s %-24s\n" % ("trackers", "box", "init", "track update=0", "track update=1"))
        for bw, bh in ((80, 80), (200, 300)):
            for n in (1, 5, 27):
                b = boxes(n, bw, bh)
                net.kcf_init(f0, b); net.kcf_track(f1, False); net.kcf_track(f1, True)          # warm-up of the shape
                row = [timed(lambda: net.kcf_init(f0, b), args.repeats)]
                net.kcf_init(f0, b)
                row.append(timed(lambda: net.kcf_track(f1, False), args.repeats))
                row.append(timed(lambda: net.kcf_track(f1, True), args.repeats))
                out.write("%-9d %-9s %s\n" % (n, "%dx%d" % (bw, bh), " ".join("%7.3f (%6.3f..%7.3f)" % r for r in row)))
        net.kcf_free()
        net.free()
        det, x = network(tmp, "tiny-yolo-voc", 416)
        det.detect(x, 0.24, 0.1)
        m = timed(lambda: det.detect(x, 0.24, 0.1), args.repeats)
        out.write("\ncontext, same process: tiny-yolo-voc 416 batch 1, forward + decode + NMS: %.3f ms (%.3f..%.3f)\n" % m)
        det.free()


def loop(args):
    from sr_object_detection_amd import darknet
    if darknet.device_count() < 1:
        sys.exit("kcf_latency: no HIP device visible")
    n, (bw, bh) = int(args.loop[0]), (int(v) for v in args.loop[1].split("x"))
    f0, f1 = frames()
    with tempfile.TemporaryDirectory() as tmp:
        net, _ = network(tmp)
        net.kcf_init(f0, boxes(n, bw, bh))
        for _ in range(args.repeats):
            net.kcf_track(f1, False)
        for _ in range(args.repeats):
            net.kcf_track(f1, True)
        net.kcf_free()
        net.free()


def stats(args, out):
    total, per = 0.0, {name: 0.0 for name, _ in STAGES}
    for row in csv.DictReader(open(args.stats)):
        for name, keys in STAGES:
            if any(k in row["Name"] for k in keys):
                per[name] += float(row["TotalDurationNs"])
                total += float(row["TotalDurationNs"])
    if total <= 0:
        sys.exit("kcf_latency: no tracker kernels in %s" % args.stats)
    # a loop of r calls with update = 0 and r with update = 1 runs the feature chain 1 + r + 2r times
    out.write("\nkernel trace (rocprofv3 --kernel-trace --stats, a run of its own): %s\n" % args.note)
    out.write("device time of the tracker's kernels: %.3f ms over 1 init + %d track(update=0) + %d track(update=1) calls\n"
              % (total / 1e6, args.calls, args.calls))
    for name, _ in STAGES:
        out.write("  %-13s %6.1f %%\n" % (name, 100 * per[name] / total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--loop", nargs=2, metavar=("TRACKERS", "WxH"))
    ap.add_argument("--stats")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    if args.loop:
        return loop(args)
    out = open(args.out, "a" if args.append else "w") if args.out else sys.stdout
    stats(args, out) if args.stats else measure(args, out)


if __name__ == "__main__":
    main()
