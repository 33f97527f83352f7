#!/usr/bin/env python3
"""Dense heads in fp16 storage mode against the same library's fp32 path, in one process.
usage: dense_f16_times.py [out=profiles/dense_f16.txt] [forwards=50] [repeats=3]

Networks: tiny-yolo-v1 448 b1, vgg-16 256 b1 / b16 / b128, yolo-v1 448 b1, alexnet 227 b1.  Each is built once in fp32 and
once in fp16 (y2_set_half); forwards alternate between the two, the first two of each are warm-up, and the per-layer times
are the median of `forwards` forwards per mode from the engine's per-layer events (y2_layer_times_ms).  The whole run is
repeated `repeats` times.  Per [connected] / [local] layer the file holds the kernel and the time in both modes and the
layer's weight bytes over its time, beside the 6.3 TB/s HBM streaming ceiling of an MI355X; per network the images/s of
both modes (batch over the sum of the layer times).  The weight-bound layers (vgg-16's first dense layer at b1 and b16,
tiny-yolo-v1's dense layer, yolo-v1's [local]) are marked: there the fp16 time has to be below the fp32 time."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

CASES = [("tiny-yolo-v1", 448, (1,)), ("vgg-16", 256, (1, 16, 128)), ("yolo-v1", 448, (1,)), ("alexnet", 227, (1,))]
CEILING_TBS = 6.3
WARMUP = 2


def weight_bound(name, batch, layers, i):
    """the layers the fp16 mode has to win on: they stream their weights"""
    kind = layers[i]["type"]
    first_dense = kind == "connected" and not any(l["type"] == "connected" for l in layers[:i])
    return (name == "vgg-16" and batch in (1, 16) and first_dense) or (name == "tiny-yolo-v1" and first_dense) or \
           (name == "yolo-v1" and kind == "local")


def weights_of(l):
    if l["type"] == "connected":
        return l["inputs"] * l["outputs"]
    return l["out_w"] * l["out_h"] * l["filters"] * l["size"] * l["size"] * l["c"]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dense_f16.txt")
    forwards = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    tmp = tempfile.mkdtemp()
    lines = ["# tools/dense_f16_times.py on %s: median of %d forwards per mode, modes alternating, %d warm-up forwards, %d repeats" %
             (darknet.device_name(), forwards, WARMUP, repeats),
             "# GB/s = the layer's weight bytes (fp32: 4 per weight, fp16: 2) over its time; HBM streaming ceiling %.1f TB/s" % CEILING_TBS]
    missed = []
    for name, size, batches in CASES:
        spec = zoo.SPECS[name]
        layers = zoo.resolve(spec, size)
        cfg = os.path.join(tmp, name + ".cfg")
        open(cfg, "w").write(zoo.cfg_text(name, size, size, batches[0], spec=spec))
        wts = os.path.join(tmp, name + ".weights")
        synth.write_weights(wts, layers, 7, 1.0)
        nets = {}
        for mode in ("fp32", "fp16"):
            nets[mode] = darknet.Network.parse_network_cfg(cfg)
            nets[mode].load_weights(wts)
            nets[mode].set_half(mode == "fp16")
            nets[mode].set_timing(True)
        os.remove(wts)
        for batch in batches:
            x = synth.image_batch(batch, 3, size, size)
            for net in nets.values():
                net.set_batch_network(batch)
            for rep in range(repeats):
                ts = {"fp32": [], "fp16": []}
                for it in range(forwards + WARMUP):
                    for mode in ("fp32", "fp16"):
                        nets[mode].network_predict(x)
                        if it >= WARMUP:
                            ts[mode].append(nets[mode].layer_times_ms())
                t = {m: np.median(np.array(v), axis=0) for m, v in ts.items()}
                lines.append("%s %dx%d b%d repeat %d: fp32 %.3f ms = %.1f images/s, fp16 %.3f ms = %.1f images/s" % (
                    name, size, size, batch, rep + 1, float(t["fp32"].sum()), batch / float(t["fp32"].sum()) * 1e3,
                    float(t["fp16"].sum()), batch / float(t["fp16"].sum()) * 1e3))
                for i, l in enumerate(layers):
                    if l["type"] not in ("connected", "local"):
                        continue
                    w = weights_of(l)
                    bound = weight_bound(name, batch, layers, i)
                    verdict = ""
                    if bound:
                        verdict = "  weight-bound: fp16 %s fp32" % ("below" if t["fp16"][i] < t["fp32"][i] else "NOT below")
                        if not t["fp16"][i] < t["fp32"][i]:
                            missed.append((name, batch, i, rep + 1))
                    lines.append("  %3d %-9s %9d weights  fp32 %-34s %8.4f ms %7.1f GB/s   fp16 %-28s %8.4f ms %7.1f GB/s%s" % (
                        i, l["type"], w, nets["fp32"].layer_kernel(i), t["fp32"][i], 4.0 * w / t["fp32"][i] / 1e6,
                        nets["fp16"].layer_kernel(i), t["fp16"][i], 2.0 * w / t["fp16"][i] / 1e6, verdict))
                print("\n".join(lines[-1 - sum(l["type"] in ("connected", "local") for l in layers):]), flush=True)
        for net in nets.values():
            net.free()
    lines.append("# weight-bound layers where fp16 was not below fp32: %s" % (missed if missed else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
