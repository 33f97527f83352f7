#!/usr/bin/env python3
"""What a dream step costs on the device: the reference's two nightmare cfgs (tests/golden/ref_cfg/vgg-conv.cfg and
jnet-conv.cfg, synthetic weights) on a 448x336 picture at max_layer 10, octaves 0 and 2.

Per (cfg, octave), in a fresh process each (the tool starts itself once per row):
  step      y2_dream_step after a warm-up, event times on the engine's stream around each call (the step neither copies
            nor waits, so the span is the device's): median, min and max ms of --steps calls
  new       the kernels of y2_dream.hip alone at the step's shapes, launched through the C-ABI on buffers of their own and
            event-timed the same way in trains of twenty: picture -> input (two launches), calculate_loss (three), gradient
            -> update (two), normalize + axpy + constrain (three) -> their sum, its share of the step, and the bytes they
            must move at 6.3 TB/s next to it.  The rest of the step is the reused products, pools and gradient_array.
  traffic   y2_dream_stats after the timed steps: allocations and bytes copied since the warm-up (nothing but the four
            bytes of the count)
  reference the wall-clock time of the same pass (resize_network once, then forward / calculate_loss / backward) through the
            compiled reference on this host (oracle/_ref/dream_ref time, built by `tests/golden/gen_dream_golden.py
            --driver-only` where the reference checkout exists; OMP_NUM_THREADS as the environment has it); skipped when
            the driver is not there or with --no-reference

usage: nightmare_latency.py [--steps 25] [--warmup 5] [--ref-steps 2] [--no-reference] [--row CFG:OCTAVE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth  # noqa: E402

W, H, MAX_LAYER, THRESH, RATE = 448, 336, 10, 1.0, .04
CFG_DIR = os.path.join(ROOT, "tests", "golden", "ref_cfg")
ROWS = [("vgg-conv", 0), ("vgg-conv", 2), ("jnet-conv", 0), ("jnet-conv", 2)]
HBM_BYTES_PER_S = 6.3e12          # the achievable rate, not the peak
TRAIN = 20                        # launches between two events: a lone 10 us kernel would be timed with its launch gap


def write_weights(path, net):
    """parser.c save_weights: header, then per convolution biases and weights; uniform, variance-preserving for leaky / relu"""
    with open(path, "wb") as f:
        f.write(np.array([0, 1, 0, 0], np.int32).tobytes())
        for i in range(net.n):
            l = net.layer(i)
            if l.type != 0:
                continue
            a = float(np.sqrt(6.0 / (l.c * l.size * l.size)))
            f.write(synth.uniform(100 + i, l.n, -.05, .05).astype(np.float32).tobytes())
            f.write(synth.uniform(200 + i, l.n * l.c * l.size * l.size, -a, a).astype(np.float32).tobytes())


class Timer:
    def __init__(self, stream):
        self.L, self.stream = darknet.lib(), stream
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert self.L.y2h_event_create(C.byref(self.e0)) == 0 and self.L.y2h_event_create(C.byref(self.e1)) == 0

    def ms(self, fn):
        ms = C.c_float(0)
        assert self.L.y2h_event_record(self.e0, self.stream) == 0
        fn()
        assert self.L.y2h_event_record(self.e1, self.stream) == 0
        assert self.L.y2h_event_elapsed_ms(self.e0, self.e1, C.byref(ms)) == 0
        return float(ms.value)


def dev_floats(L, n, fill=None):
    p = C.c_void_p()
    assert L.y2h_malloc(C.byref(p), max(n, 4) * 4) == 0, L.y2h_last_error()
    if fill is not None:
        a = np.ascontiguousarray(fill, dtype=np.float32)
        assert L.y2h_memcpy_h2d(p, a.ctypes.data, a.nbytes, None) == 0 and L.y2h_device_sync() == 0
    return p


def new_kernels(timer, sw, sh, last_n, reps):
    """the four groups of y2_dream.hip at the step's shapes -> {name: (ms, bytes it must move)}"""
    L = darknet.lib()
    n, m = 3 * H * W, 3 * sh * sw
    pic, upd = dev_floats(L, n, synth.uniform(1, n, 0, 1)), dev_floats(L, n)
    x, grad = dev_floats(L, m), dev_floats(L, m, synth.uniform(2, m, -1, 1))
    out, delta = dev_floats(L, last_n, synth.uniform(3, last_n, 0, 2)), dev_floats(L, last_n)
    tmp = dev_floats(L, 3 * max(H * sw, sh * W))
    part, stat, sel = dev_floats(L, 2 * L.y2h_dream_chunks(max(n, last_n))), dev_floats(L, 2), dev_floats(L, 1)
    to_in = darknet.DreamResample(3, H, W, 0, 0, -3, 5, H, W, sh, sw, 0, 0, 1, 1)
    back = darknet.DreamResample(3, sh, sw, 1, 1, 0, 0, sh, sw, H, W, 3, -5, 0, 0)
    s = timer.stream
    calls = {
        "picture_to_input": (lambda: L.y2h_dream_resample_run(C.byref(to_in), pic, tmp, x, s), 4 * (n + m)),
        "calculate_loss": (lambda: L.y2h_dream_loss(out, delta, last_n, THRESH, part, stat, sel, s), 4 * 2 * last_n),
        "gradient_to_update": (lambda: L.y2h_dream_resample_run(C.byref(back), grad, tmp, upd, s), 4 * (n + m)),
        "normalize_axpy_constrain": (lambda: L.y2h_dream_apply(pic, upd, n, 0.0, 1, part, stat, s), 4 * 3 * n),
    }
    res = {}
    for name, (fn, nbytes) in calls.items():
        def train():
            for _ in range(TRAIN):
                assert fn() == 0, L.y2h_last_error()
        train()
        ms = float(np.median([timer.ms(train) for _ in range(reps)])) / TRAIN
        res[name] = {"ms": round(ms, 4), "must_move_bytes": nbytes, "floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 5)}
    for p in (pic, upd, x, grad, out, delta, tmp, part, stat, sel):
        L.y2h_free(p)
    return res


def sized_cfg(tmp, cfg_name):
    """the cfg with the picture's size in its [net] section: jnet-conv.cfg ships with 10x10, at which its own six maxpools
    leave no pixel and the parser (the reference's too) refuses it"""
    import re
    text = open(os.path.join(CFG_DIR, cfg_name + ".cfg")).read()
    text = re.sub(r"(?m)^width\s*=.*$", "width=%d" % W, re.sub(r"(?m)^height\s*=.*$", "height=%d" % H, text))
    cfg = os.path.join(tmp, cfg_name + ".cfg")
    open(cfg, "w").write(text)
    return cfg


def row(cfg_name, octave, steps, warmup, ref_steps):
    tmp = tempfile.mkdtemp()
    cfg = sized_cfg(tmp, cfg_name)
    net = darknet.Network.parse_network_cfg(cfg)
    wts = os.path.join(tmp, cfg_name + ".weights")
    write_weights(wts, net)
    net.load_weights(wts)
    net.set_batch_network(1)
    scale = darknet.dream_scale(octave)
    sw, sh = darknet.dream_size(W, H, scale)
    pic = synth.uniform(9, 3 * H * W, 0, 1).reshape(3, H, W)
    d = net.dream_open(pic)
    draws = [(-3, 5, 1), (6, -8, 0), (0, 0, 0), (-8, 7, 1)]

    def step(k):
        dx, dy, flip = draws[k % len(draws)]
        d.step(MAX_LAYER, scale, RATE, THRESH, 1, dx, dy, flip)
    for k in range(warmup):
        step(k)
    d.fetch()
    held = d.stats()
    timer = Timer(net.stream())
    ms = [timer.ms(lambda: step(k)) for k in range(steps)]
    after = d.stats()
    finite = bool(np.isfinite(d.fetch()).all())
    # the last layer's size at this input, by the layer table of a network resized the same way (its own copy)
    shape = darknet.Network.parse_network_cfg(cfg)
    shape.set_batch_network(1)
    shape.resize_network(sw, sh)
    last_n = shape.layer(MAX_LAYER).outputs
    shape.free()
    kernels = new_kernels(timer, sw, sh, last_n, 11)
    new_ms = sum(v["ms"] for v in kernels.values())
    res = {"cfg": cfg_name, "picture": "%dx%d" % (W, H), "max_layer": MAX_LAYER, "octave": octave, "input": "%dx%d" % (sw, sh),
           "step_ms_median": round(float(np.median(ms)), 3), "step_ms_min": round(min(ms), 3), "step_ms_max": round(max(ms), 3), "steps": steps,
           "selected": after["selected"], "picture_finite": finite,
           "new_kernels": kernels, "new_kernels_ms": round(new_ms, 4), "new_share_of_step": round(new_ms / float(np.median(ms)), 4),
           "allocations_in_timed_steps": after["allocations"] - held["allocations"],
           "h2d_bytes_in_timed_steps": after["h2d_bytes"] - held["h2d_bytes"], "d2h_bytes_in_timed_steps": after["d2h_bytes"] - held["d2h_bytes"]}
    d.close()
    net.free()
    driver = os.path.join(ROOT, "oracle", "_ref", "dream_ref")
    if ref_steps and os.path.exists(driver):
        out = subprocess.run([driver, "time", cfg, wts, str(MAX_LAYER), str(sw), str(sh), str(THRESH), str(ref_steps)], capture_output=True,
                             text=True, check=True).stdout
        secs = [float(line.split()[3]) for line in out.splitlines() if line.startswith("pass")]
        res["reference"] = {"threads": os.environ.get("OMP_NUM_THREADS", "unset"), "seconds_per_pass": secs}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-steps", type=int, default=2)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--row", default=None, help="measure this row in this process, e.g. vgg-conv:2 (what the tool starts itself with)")
    a = ap.parse_args()
    ref_steps = 0 if a.no_reference else a.ref_steps
    if a.row:
        name, octave = a.row.split(":")
        print(json.dumps(row(name, int(octave), a.steps, a.warmup, ref_steps)))
        return
    rows = []
    for name, octave in ROWS:                   # a fresh process per row: no row inherits another's clocks, caches or allocator state
        cmd = [sys.executable, os.path.abspath(__file__), "--row", "%s:%d" % (name, octave), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--ref-steps", str(ref_steps)] + (["--no-reference"] if a.no_reference else [])
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            sys.exit("row %s:%d failed (%d):\n%s" % (name, octave, out.returncode, out.stderr[-2000:]))
        rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
        print("  " + json.dumps(rows[-1]))
    print(json.dumps({"tool": "nightmare_latency", "device": darknet.device_name(), "rows": rows}))


if __name__ == "__main__":
    main()
