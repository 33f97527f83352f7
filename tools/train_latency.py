#!/usr/bin/env python3
"""What a training step costs on the device: Darknet-19 (cfg/darknet19.cfg: the trunk, 1x1 -> 1000, avgpool, softmax, cost)
at 224x224, by default at batch 16 and batch 64; with --net tiny-yolo-voc or --net yolo the detector at 416x416 (batch 16 / 8
by default) with its [region] head in training mode: yolo.cfg's training options, three truths per image.

Per batch size:
  step      y2_train_step_device (input and truth already in HBM) after a warm-up: event times on the engine's stream
            around each call -> p50 ms per step and images/s.  A step ends with the copy of the loss, so the span is
            host-visible.
  products  per convolution, the three products of y2_train.hip launched on buffers of the layer's shape, event-timed the
            same way: forward y = x * w, dinput dx = dy * w^T, dweight dw += x^T * dy (its two launches together), each
            as ms and achieved TFLOP/s (2 * batch*out_h*out_w * size*size*c * n flops per product; dinput of layer 0 is
            timed although a step skips it)
  reference the wall-clock time of the same step through the compiled reference on this host (oracle/_ref/train_ref time,
            built by `tests/golden/gen_train_golden.py --driver-only` where the reference checkout exists; for a detector
            oracle/_ref/train_det_ref, by `tests/golden/gen_train_det_golden.py --driver-only`; OMP_NUM_THREADS as the
            environment has it); skipped when the driver is not there or with --no-reference

A detector's row also names the launches of its head (y2_train_det.hip: region_cells, region_truths, region_sumsq,
region_finish): their share of the step is read from one `rocprofv3 --kernel-trace --stats -- python tools/train_latency.py
--net yolo --no-products --no-reference` run.

With --loader one more row per batch size.  For --net darknet19 it is the classifier loader: `batch` frames of 500x375x3
bytes, the draws made by y2_aug_draw_classification with cfg/tiny.cfg's values (angle=7 aspect=.75 hue=.1 saturation=.75
exposure=.75 max_crop=320, min_crop = the network's width), one-hot truth rows:
  kernel    y2h_augment_cls_to_input alone on what y2_aug_cls_pack sends up, already in HBM, twenty launches back to back
            between two events -> p50 ms per launch, next to its byte floor: the output floats written once plus the
            packed source bytes read once, at 6.3 TB/s
  load      host wall time of y2_train_load_classification (p50) and its split as y2_train_load_times reports it
  step      load + y2_train_step_loaded against y2_train_step fed ready-made host floats, in alternating pairs
For a detector it is the detection loader: `batch` frames of 500x375x3 bytes with
three label rows each, the draws made by y2_aug_draw_detection from what y2_net_augment reports:
  kernel    y2h_augment_to_input alone on buffers already in HBM, twenty launches back to back between two events -> p50 ms
            per launch, next to its byte floor: the output
            floats written once plus the source bytes the windows touch read once, at 6.3 TB/s
  load      host wall time of y2_train_load_detection (p50), and its split as y2_train_load_times reports it: pack,
            enqueue (copy + kernel + truth copy), wait for the copy
  step      host wall time per step of load + y2_train_step_loaded against y2_train_step fed ready-made host floats (no
            augmentation at all, the whole float batch uploaded and transposed), in alternating pairs after a warm-up

With --precision bf16x3 or --precision bf16 the step row and the per-product rows are measured a second time in that mode
(y2_train_set_precision; the products through y2h_train_conv_*_bf16 with planes 3 or 1), in the same process on the same
buffers, and reported under "precision": the fp32 rows stay what they are.

With --net rnn the rows are char-rnn training steps (the layers of cfg/rnn.train.cfg: three batch-normalised [rnn] of 1024,
[connected] 256) at `--batches BxT,...` (default 128x576, the cfg's own, and 16x64): ms per step and characters per second;
--loader adds the wall time of train_load_chars + train_step_loaded.

usage: train_latency.py [--net darknet19|tiny-yolo-voc|yolo|tiny-yolo-v1|rnn] [--dense 32x12544x1470,...] [--batches 16,64] [--steps 10] [--warmup 3] [--reps 5] [--ref-batch 16] [--no-reference]
                        [--no-products] [--layers 4,18] [--loader] [--precision fp32|bf16x3|bf16]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

# name: (size, default batches, default reference batch, reference driver)
NETS = {"darknet19": (224, "16,64", 16, "train_ref"), "tiny-yolo-voc": (416, "16", 16, "train_det_ref"), "yolo": (416, "8", 8, "train_det_ref"),
        "tiny-yolo-v1": (448, "32", 32, None)}            # no reference row: tests/native/train_v1_ref.c has no `time` command          # cfg/yolov1/tiny-yolo.cfg: batch=64 subdivisions=2
# what cfg/yolo.cfg sets for training behind softmax=1
REGION_TRAINING = "softmax=1\nbias_match=1\nrescore=1\nobject_scale=5\nnoobject_scale=1\nclass_scale=1\ncoord_scale=1\nthresh=.6\njitter=.3"


# what cfg/yolov1/tiny-yolo.cfg sets for training
DETECTION_TRAINING = "object_scale=1\nnoobject_scale=.5\nclass_scale=1\ncoord_scale=5\njitter=.2"


def cfg_for(name, size, batch):
    if name == "tiny-yolo-v1":
        return zoo.cfg_text(name, size, size, batch).replace("jitter=.2", DETECTION_TRAINING)
    return zoo.cfg_text(name, size, size, batch).replace("softmax=1", REGION_TRAINING)


def truth_for(net, batch):
    """one-hot rows for a classifier; for a detector three boxes per image (the pattern of train_det_ref time)"""
    per = net.truth_floats()
    y = np.zeros((batch, per), np.float32)
    last = net.layer(net.n - 1)
    if last.type == darknet.LAYER_TYPES.index("REGION"):
        for i in range(batch):
            for t in range(3):
                y[i, 5 * t:5 * t + 5] = (.2 + .3 * t, .7 - .2 * t, .1 + .15 * t, .4 - .1 * t, (i + t) % last.classes)
    elif last.type == darknet.LAYER_TYPES.index("DETECTION"):            # three object cells per image: is-object, class row, box
        row = 1 + last.classes + 4
        for i in range(batch):
            for t in range(3):
                c0 = ((7 * i + 11 * t) % (last.side * last.side)) * row
                y[i, c0] = 1
                y[i, c0 + 1 + (i + t) % last.classes] = 1
                y[i, c0 + 1 + last.classes:c0 + row] = (.2 + .3 * t, .7 - .2 * t, .1 + .15 * t, .4 - .1 * t)
    else:
        y[np.arange(batch), np.arange(batch) % per] = 1
    return y


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


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def products(net, timer, reps, only=None, planes=0):
    """planes = 0: the fp32 kernels; 3 / 1: the bf16 kernels, split / rounded operands"""
    L = darknet.lib()
    rows = []
    for i in range(net.n):
        l = net.layer(i)
        if l.type != 0 or (only is not None and i not in only):                       # CONVOLUTIONAL
            continue
        g = darknet.TrainConv(net.batch, l.h, l.w, l.c, l.n, l.size, l.pad, l.out_h, l.out_w)
        nx, ny, nw = net.batch * l.h * l.w * l.c, net.batch * l.out_h * l.out_w * l.n, l.size * l.size * l.c * l.n
        x = dev_floats(L, nx, synth.uniform(7 + i, nx, -1, 1))
        dy = dev_floats(L, ny, synth.uniform(70 + i, ny, -1, 1))
        w = dev_floats(L, nw, synth.uniform(700 + i, nw, -.1, .1))
        y, dx, dw = dev_floats(L, ny), dev_floats(L, nx), dev_floats(L, nw, np.zeros(nw, np.float32))
        ws = C.c_void_p()
        assert L.y2h_malloc(C.byref(ws), L.y2h_train_dweight_ws_bytes(C.byref(g))) == 0
        calls = {"forward": lambda: L.y2h_train_conv_forward(C.byref(g), x, w, y, timer.stream),
                 "dinput": lambda: L.y2h_train_conv_dinput(C.byref(g), dy, w, dx, timer.stream),
                 "dweight": lambda: L.y2h_train_conv_dweight(C.byref(g), x, dy, dw, ws, timer.stream)}
        if planes:
            calls = {"forward": lambda: L.y2h_train_conv_forward_bf16(C.byref(g), x, w, y, planes, timer.stream),
                     "dinput": lambda: L.y2h_train_conv_dinput_bf16(C.byref(g), dy, w, dx, planes, timer.stream),
                     "dweight": lambda: L.y2h_train_conv_dweight_bf16(C.byref(g), x, dy, dw, ws, planes, timer.stream)}
        flops = 2.0 * net.batch * l.out_h * l.out_w * l.size * l.size * l.c * l.n
        row = {"layer": i, "shape": "%dx%dx%d -> %d, %dx%d" % (l.w, l.h, l.c, l.n, l.size, l.size), "gflop": round(flops / 1e9, 2),
               "dweight_splits": int(L.y2h_train_dweight_splits(C.byref(g)))}
        for name, fn in calls.items():
            assert fn() == 0, L.y2h_last_error()
            t = p50([timer.ms(fn) for _ in range(reps)])
            row[name + "_ms"] = round(t, 4)
            row[name + "_tflops"] = round(flops / (t * 1e-3) / 1e12, 2)
        for p in (x, dy, w, y, dx, dw, ws):
            L.y2h_free(p)
        print("    " + json.dumps(row))
        rows.append(row)
    return rows


HBM_BYTES_PER_S = 6.3e12          # the achievable rate, not the peak


COLD_BYTES = 640 << 20           # --cold: rotate over this many bytes of weights, 2.5 times the 256 MB last-level cache


def dense_products(batch, inputs, outputs, timer, reps, label="", cold=False):
    """the three products of one [connected] layer: the dense kernels (y2_train_dense.hip), the byte floor of each (the
    weight bytes it must move at HBM_BYTES_PER_S: w once for forward and dinput, dw read and written for dweight) and the
    baseline, the convolution template called at the 1x1 geometry (h = w = size = 1), which a step would otherwise run.
    cold: every launch takes the next of ceil(COLD_BYTES / weight bytes) copies of w and dw, so that no launch finds its
    weights in the last-level cache -- as in a step, where the convolutions' tensors pass through it in between"""
    L = darknet.lib()
    g = darknet.TrainDense(batch, inputs, outputs)
    c = darknet.TrainConv(batch, 1, 1, inputs, outputs, 1, 0, 1, 1)
    nx, ny, nw = batch * inputs, batch * outputs, inputs * outputs
    copies = -(-COLD_BYTES // (nw * 4)) if cold else 1
    x = dev_floats(L, nx, synth.uniform(7, nx, -1, 1))
    dy = dev_floats(L, ny, synth.uniform(70, ny, -1, 1))
    w0 = synth.uniform(700, nw, -.1, .1)
    ws_, dws = [dev_floats(L, nw, w0) for _ in range(copies)], [dev_floats(L, nw) for _ in range(copies)]
    for p in dws:
        assert L.y2h_memset(p, 0, C.c_size_t(nw * 4), None) == 0
    assert L.y2h_device_sync() == 0
    y, dx = dev_floats(L, ny), dev_floats(L, nx)
    plans = [darknet.train_dense_plan(batch, inputs, outputs, p) for p in (darknet.DENSE_FORWARD, darknet.DENSE_DINPUT)]
    ws, cws = C.c_void_p(), C.c_void_p()
    assert L.y2h_malloc(C.byref(ws), max(16, plans[0][1], plans[1][1])) == 0
    assert L.y2h_malloc(C.byref(cws), L.y2h_train_dweight_ws_bytes(C.byref(c))) == 0
    turn = [0]

    def nxt(bufs):
        turn[0] += 1
        return bufs[turn[0] % copies]
    calls = {"forward": (lambda: L.y2h_train_dense_forward(C.byref(g), x, nxt(ws_), y, ws, 0, timer.stream),
                         lambda: L.y2h_train_conv_forward(C.byref(c), x, nxt(ws_), y, timer.stream), nw * 4),
             "dinput": (lambda: L.y2h_train_dense_dinput(C.byref(g), dy, nxt(ws_), dx, 0, ws, 0, timer.stream),
                        lambda: L.y2h_train_conv_dinput(C.byref(c), dy, nxt(ws_), dx, timer.stream), nw * 4),
             "dweight": (lambda: L.y2h_train_dense_dweight(C.byref(g), x, dy, nxt(dws), timer.stream),
                         lambda: L.y2h_train_conv_dweight(C.byref(c), x, dy, nxt(dws), cws, timer.stream), 2 * nw * 4)}
    row = {"dense": "%s%d x %d x %d" % (label, batch, inputs, outputs), "weights": "cold, %d copies in turn" % copies if cold else "warm, one copy",
           "forward_ranges": plans[0][0], "dinput_ranges": plans[1][0], "ws_bytes": int(max(plans[0][1], plans[1][1]))}
    for name, (new, old, nbytes) in calls.items():
        times = {"new": [], "old": []}
        for fn in (new, old):
            assert fn() == 0, L.y2h_last_error()
        for _ in range(reps):                              # alternating: both see the same clocks and the same cache state
            times["new"].append(timer.ms(new))
            times["old"].append(timer.ms(old))
        row[name] = {"ms": round(p50(times["new"]), 4), "min_max_ms": [round(min(times["new"]), 4), round(max(times["new"]), 4)],
                     "byte_floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4),
                     "conv_template_1x1_ms": round(p50(times["old"]), 4),
                     "conv_template_min_max_ms": [round(min(times["old"]), 4), round(max(times["old"]), 4)]}
    for p in [x, dy, y, dx, ws, cws] + ws_ + dws:
        L.y2h_free(p)
    print("    " + json.dumps(row))
    return row


def detection_head_ms(net, timer, reps):
    """the [detection] head alone (forward, delta, cost, statistics) at the network's shape"""
    L = darknet.lib()
    l = net.layer(net.n - 1)
    g = darknet.TrainDetection(net.batch, l.side, l.n, l.classes, l.softmax, l.sqrt, l.rescore, l.forced, l.coord_scale, l.object_scale,
                               l.noobject_scale, l.class_scale)
    n = net.batch * l.outputs
    x = dev_floats(L, n, synth.uniform(3, n, .1, .9))
    t = dev_floats(L, net.batch * l.truths, truth_for(net, net.batch))
    bufs = [dev_floats(L, n) for _ in range(3)] + [dev_floats(L, 16), dev_floats(L, 16)]
    sc = C.c_void_p()
    assert L.y2h_malloc(C.byref(sc), L.y2h_train_detection_scratch_bytes(C.byref(g))) == 0

    def fn():
        return L.y2h_train_detection_loss(C.byref(g), x, t, bufs[0], bufs[1], bufs[2], 0, bufs[3], bufs[4], sc, timer.stream)
    assert fn() == 0, L.y2h_last_error()
    ms = p50([timer.ms(fn) for _ in range(reps)])
    for p in [x, t, sc] + bufs:
        L.y2h_free(p)
    return round(ms, 4)


def measure_loader(net, batch, timer, steps, warmup, reps, label, table, pixels, touched, frame_bytes, launch, load):
    """what both --loader rows measure: `launch(d_desc, d_pix, d_out)` alone on `table` and `pixels` already in HBM, twenty
    launches between two events; `load(k)` alone with its split; load + y2_train_step_loaded against y2_train_step fed
    ready-made host floats, in alternating pairs"""
    L = darknet.lib()
    w, h = net.net.w, net.net.h
    d_desc, d_pix, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    out_bytes = batch * h * w * 3 * 4
    assert L.y2h_malloc(C.byref(d_desc), table.size) == 0 and L.y2h_malloc(C.byref(d_pix), pixels.size) == 0 and L.y2h_malloc(C.byref(d_out), out_bytes) == 0
    assert L.y2h_memcpy_h2d(d_desc, table.ctypes.data, table.size, None) == 0 and L.y2h_memcpy_h2d(d_pix, pixels.ctypes.data, pixels.size, None) == 0
    assert L.y2h_device_sync() == 0

    BACK_TO_BACK = 20                                    # one pair of events around a train of launches: a lone 10 us kernel
                                                         # would be timed with its launch gap

    def kernel():
        for _ in range(BACK_TO_BACK):
            assert launch(d_desc, d_pix, d_out) == 0
    for _ in range(warmup):
        kernel()
    kernel_ms = p50([timer.ms(kernel) for _ in range(max(reps, 5) * 4)]) / BACK_TO_BACK
    for p_ in (d_desc, d_pix, d_out):
        L.y2h_free(p_)
    floor_ms = (out_bytes + touched) / HBM_BYTES_PER_S * 1e3
    # the load, and load + step against the host-float step, in alternating pairs
    x = synth.uniform(5, batch * net.net.inputs, 0, 1)
    y = truth_for(net, batch)
    loss = C.c_float(0)

    def new_step(k):
        load(k, y)
        assert L.y2_train_step_loaded(C.byref(net.net), C.byref(loss)) == 0, darknet._check()

    def old_step(k):
        assert L.y2_train_step(C.byref(net.net), x.ctypes.data, y.ctypes.data, C.byref(loss)) == 0, darknet._check()

    def wall(fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        return (time.perf_counter() - t0) * 1e3
    for k in range(warmup):
        new_step(k)
        old_step(k)
    new_ms, old_ms, load_ms, split = [], [], [], []
    for k in range(steps):
        new_ms.append(wall(new_step, k))
        old_ms.append(wall(old_step, k))
    for k in range(steps):
        load_ms.append(wall(load, k, y))
        split.append(net.train_load_times())
    return {"loader": {"frames": "%d x %s -> %dx%d" % (batch, label, w, h), "kernel_p50_ms": round(kernel_ms, 4), "byte_floor_ms": round(floor_ms, 4),
                       "kernel_over_floor": round(kernel_ms / floor_ms, 2), "kernel_share_of_step": round(kernel_ms / p50(new_ms), 4),
                       "output_bytes": out_bytes, "touched_source_bytes": int(touched),
                       "frame_bytes": int(frame_bytes), "host_float_bytes": int(x.nbytes), "load_wall_p50_ms": round(p50(load_ms), 3),
                       "load_pack_ms": round(p50([s_[0] for s_ in split]), 3), "load_enqueue_ms": round(p50([s_[1] for s_ in split]), 3),
                       "load_wait_copy_ms": round(p50([s_[2] for s_ in split]), 3),
                       "load_plus_step_p50_ms": round(p50(new_ms), 3), "host_float_step_p50_ms": round(p50(old_ms), 3),
                       "new_over_old": round(p50(new_ms) / p50(old_ms), 3),
                       "load_plus_step_ms": [round(v, 3) for v in new_ms], "host_float_step_ms": [round(v, 3) for v in old_ms]}}


def loader_row(net, batch, timer, steps, warmup, reps):
    """the --loader row of a detector: see the module docstring"""
    L = darknet.lib()
    aug = net.net_augment()
    w, h = net.net.w, net.net.h
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, size=(375, 500, 3), dtype=np.uint8) for _ in range(batch)]
    boxes = np.array([[3, .3, .4, .2, .3], [7, .6, .5, .3, .4], [11, .5, .7, .25, .2]], np.float32)
    hue, sat, exp = (aug["hue"], aug["saturation"], aug["exposure"]) if aug["hue"] else (.1, 1.5, 1.5)    # yolo.cfg's, where the cfg text has none
    darknet.srand(1)
    sets = []
    for _ in range(4):                                   # four batches of draws, reused in turn
        items = [dict(darknet.aug_draw_detection(500, 375, aug["jitter"], hue, sat, exp, len(boxes)), frame=f, boxes=boxes) for f in frames]
        sets.append((items,) + darknet.aug_items(items))
    # kernel alone: whole frames and a table made here
    items = sets[0][0]
    desc = (darknet.Aug * batch)()
    touched = 0
    for i, it in enumerate(items):
        desc[i] = darknet.Aug(i * 375 * 1500, 1500, 3, 0, 0, 500, 375, 500, 375, it["pleft"], it["ptop"], it["swidth"], it["sheight"], it["flip"],
                              it["dhue"], it["dsat"], it["dexp"], np.float32(it["swidth"] - 1) / np.float32(w - 1),
                              np.float32(it["sheight"] - 1) / np.float32(h - 1))
        cols = min(max(it["pleft"] + it["swidth"] - 1, 0), 499) - min(max(it["pleft"], 0), 499) + 1
        rows = min(max(it["ptop"] + it["sheight"] - 1, 0), 374) - min(max(it["ptop"], 0), 374) + 1
        touched += cols * rows * 3
    pixels = np.concatenate([f.reshape(-1) for f in frames])
    table = np.frombuffer(bytes(desc), np.uint8)

    def launch(d_desc, d_pix, d_out):
        return L.y2h_augment_to_input(d_desc, batch, d_pix, 0, h, w, d_out, timer.stream)

    def load(k, _y):
        _, arr, _keep = sets[k % len(sets)]
        assert L.y2_train_load_detection(C.byref(net.net), arr, batch, 0) == 0, darknet._check()
    return measure_loader(net, batch, timer, steps, warmup, reps, "500x375x3", table, pixels, touched, sum(f.nbytes for f in frames), launch, load)


TINY_CFG = dict(angle=7., aspect=.75, hue=.1, saturation=.75, exposure=.75, max_crop=320)      # cfg/tiny.cfg's [net] values


def cls_loader_row(net, batch, timer, steps, warmup, reps):
    """the --loader row of a classifier: see the module docstring"""
    L = darknet.lib()
    size = net.net.w
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, size=(375, 500, 3), dtype=np.uint8) for _ in range(batch)]
    a = TINY_CFG
    darknet.srand(1)
    sets = []
    for _ in range(4):                                   # four batches of draws, reused in turn
        items = [dict(darknet.aug_draw_classification(500, 375, size, a["max_crop"], size, a["angle"], a["aspect"], a["hue"], a["saturation"],
                                                      a["exposure"]), frame=f) for f in frames]
        sets.append((items,) + darknet.aug_cls_items(items))
    # kernel alone: the packer's table and rectangles
    _, arr, _keep = sets[0]
    touched = int(L.y2_aug_cls_pack_bytes(arr, batch, size))
    desc = (darknet.AugCls * batch)()
    pixels = np.zeros(touched, np.uint8)
    L.y2_aug_cls_pack(arr, batch, size, desc, pixels.ctypes.data)
    table = np.frombuffer(bytes(desc), np.uint8)

    def launch(d_desc, d_pix, d_out):
        return L.y2h_augment_cls_to_input(d_desc, batch, d_pix, 0, size, d_out, timer.stream)

    def load(k, y):
        _, arr, _keep = sets[k % len(sets)]
        assert L.y2_train_load_classification(C.byref(net.net), arr, y.ctypes.data, batch, 0) == 0, darknet._check()
    return measure_loader(net, batch, timer, steps, warmup, reps, "500x375x3", table, pixels, touched, sum(f.nbytes for f in frames), launch, load)


def reference_step(tmp, wts, name, size, batch, steps=2):
    driver = NETS[name][3] and os.path.join(ROOT, "oracle", "_ref", NETS[name][3])
    if not driver or not os.path.exists(driver):
        return None
    cfg = os.path.join(tmp, "ref_b%d.cfg" % batch)
    open(cfg, "w").write(cfg_for(name, size, batch))
    out = subprocess.run([driver, "time", cfg, wts, str(steps)], capture_output=True, text=True, check=True).stdout
    secs = [float(line.split()[3]) for line in out.splitlines() if line.startswith("step")]
    return {"batch": batch, "threads": os.environ.get("OMP_NUM_THREADS", "unset"), "seconds_per_step": secs}


def rnn_rows(a):
    """--net rnn: char-rnn training (cfg/rnn.train.cfg's layers) at B sequences x T steps, `--batches BxT,...`: ms per step and
    characters per second through train_step_device, with --loader through train_load_chars + train_step_loaded as well.
    The split of a step is read from a kernel trace of this run with --steps 1."""
    L = darknet.lib()
    out = []
    print("rnn, device %s" % darknet.device_name())
    tmp = tempfile.mkdtemp()
    text = bytes(1 + (i * 7 + i // 13) % 250 for i in range(1 << 16))
    for shape in (a.batches or "128x576,16x64").split(","):
        B, T = [int(v) for v in shape.split("x")]
        cfg = os.path.join(tmp, "rnn_%dx%d.cfg" % (B, T))
        open(cfg, "w").write(zoo.recurrent_cfg_text("rnn", B, T).replace("[net]", "[net]\nlearning_rate=0.1\nmomentum=0.9\ndecay=0.001", 1))
        net = darknet.Network.parse_network_cfg(cfg)
        t0 = time.time()
        net.train_prepare()
        rows, inputs = B * T, net.net.inputs
        off = np.arange(B, dtype=np.uint64) * 101
        x, y = darknet.get_rnn_data(text, off, inputs, B, T)
        d_x, d_y = dev_floats(L, x.size, x), dev_floats(L, y.size, y)
        timer = Timer(net.stream())
        losses = [net.train_step_device(d_x.value, d_y.value) for _ in range(a.warmup)]
        ms = [timer.ms(lambda: losses.append(net.train_step_device(d_x.value, d_y.value))) for _ in range(a.steps)]
        res = {"sequences": B, "time_steps": T, "prepare_s": round(time.time() - t0, 2)}
        if ms:
            res.update(step_p50_ms=round(p50(ms), 3), step_max_ms=round(max(ms), 3), chars_per_s=round(rows / (p50(ms) * 1e-3), 1),
                       first_loss=losses[0], last_loss=losses[-1])
        if a.loader:
            def loaded():
                net.train_load_chars(text, off)
                losses.append(net.train_step_loaded())
            for _ in range(a.warmup):
                loaded()
            wall = []
            for _ in range(max(a.steps, 1)):
                w0 = time.perf_counter()
                loaded()
                wall.append((time.perf_counter() - w0) * 1e3)
            res["loader"] = {"load_and_step_wall_p50_ms": round(p50(wall), 3), "chars_per_s": round(rows / (p50(wall) * 1e-3), 1)}
        print("  " + json.dumps(res))
        L.y2h_free(d_x)
        L.y2h_free(d_y)
        net.free()
        out.append(res)
    print(json.dumps({"tool": "train_latency", "device": darknet.device_name(), "net": "rnn", "rows": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="darknet19", choices=sorted(NETS) + ["rnn"])
    ap.add_argument("--batches", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-batch", type=int, default=None)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--no-products", action="store_true")
    ap.add_argument("--layers", default=None, help="only these layers' products, e.g. 4,18 (with --steps 0 --warmup 0 "
                    "--no-reference: the few launches a counter run wants, `rocprofv3 --pmc ... -- python tools/train_latency.py ...`)")
    ap.add_argument("--precision", default="fp32", choices=darknet.TRAIN_PRECISIONS, help="measure the step and the products in this mode as well")
    ap.add_argument("--dense", default=None, help="only the three dense products at these shapes, batch x inputs x outputs, "
                    "e.g. 32x12544x1470,64x4096x1470: the dense kernels, their byte floors and the convolution template at 1x1")
    ap.add_argument("--cold", action="store_true", help="with --dense: rotate over copies of the weights so that no launch finds them in the last-level cache")
    ap.add_argument("--loader", action="store_true", help="add the loader's row: the classifier loader for darknet19, the detection loader for a detector")
    a = ap.parse_args()
    if a.net == "rnn":
        return rnn_rows(a)
    SIZE, batches, ref_batch = NETS[a.net][:3]
    L = darknet.lib()
    if a.dense:
        stream = C.c_void_p()
        assert L.y2h_stream_create(C.byref(stream)) == 0
        print("dense products, device %s" % darknet.device_name())
        print(json.dumps({"dense": [dense_products(*[int(v) for v in shape.split("x")], Timer(stream), max(a.reps, 11), "", a.cold)
                                    for shape in a.dense.split(",")]}))
        return
    tmp = tempfile.mkdtemp()
    wts = os.path.join(tmp, "net.weights")
    synth.write_weights(wts, zoo.resolve(a.net, SIZE), 41, 1.0)
    print("%s at %d, device %s" % (a.net, SIZE, darknet.device_name()))
    out = []
    for batch in [int(b) for b in (a.batches or batches).split(",")]:
        cfg = os.path.join(tmp, "net_b%d.cfg" % batch)
        open(cfg, "w").write(cfg_for(a.net, SIZE, batch))
        net = darknet.Network.parse_network_cfg(cfg)
        net.load_weights(wts)
        net.train_prepare()
        y = truth_for(net, batch)
        d_x = dev_floats(L, batch * net.net.inputs, synth.uniform(5, batch * net.net.inputs, -1, 1))
        d_y = dev_floats(L, y.size, y)
        timer = Timer(net.stream())
        losses = [net.train_step_device(d_x.value, d_y.value) for _ in range(a.warmup)]
        ms = []
        for _ in range(a.steps):
            ms.append(timer.ms(lambda: losses.append(net.train_step_device(d_x.value, d_y.value))))
        res = {"batch": batch}
        if ms:
            res.update(step_p50_ms=round(p50(ms), 3), step_max_ms=round(max(ms), 3),
                       images_per_s=round(batch / (p50(ms) * 1e-3), 1), first_loss=losses[0], last_loss=losses[-1])
        if ms and a.net == "tiny-yolo-v1":
            res["detection"] = {k: (None if v != v else v) for k, v in net.train_detection_stats().items()}
            res["head_ms"] = detection_head_ms(net, timer, max(a.reps, 11))
            res["head_share_of_step"] = round(res["head_ms"] / res["step_p50_ms"], 4)
            if not a.no_products:
                dense = [dense_products(batch, net.layer(i).inputs, net.layer(i).outputs, timer, max(a.reps, 11), "layer %d: " % i)
                         for i in range(net.n) if net.layer(i).type == darknet.LAYER_TYPES.index("CONNECTED")]
                res["dense"] = dense
                res["dense_share_of_step"] = round(sum(d[k]["ms"] for d in dense for k in ("forward", "dinput", "dweight")) / res["step_p50_ms"], 4)
        elif ms and a.net != "darknet19":
            res["region"] = {k: (None if v != v else v) for k, v in net.train_region_stats().items()}
        print("  " + json.dumps(res))
        only = None if a.layers is None else {int(v) for v in a.layers.split(",")}
        if not a.no_products:
            res["products"] = products(net, timer, a.reps, only)
            for k in ("forward", "dinput", "dweight"):
                res[k + "_sum_ms"] = round(sum(r[k + "_ms"] for r in res["products"]), 3)
        if a.precision != "fp32":                                    # the same rows once more, in that mode
            net.train_set_precision(a.precision)
            mode = {"mode": a.precision}
            for _ in range(a.warmup):
                net.train_step_device(d_x.value, d_y.value)
            ms = [timer.ms(lambda: losses.append(net.train_step_device(d_x.value, d_y.value))) for _ in range(a.steps)]
            if ms:
                mode.update(step_p50_ms=round(p50(ms), 3), step_max_ms=round(max(ms), 3), images_per_s=round(batch / (p50(ms) * 1e-3), 1),
                            last_loss=losses[-1], step_over_fp32=round(p50(ms) / res["step_p50_ms"], 3))
            print("  " + json.dumps(mode))
            if not a.no_products:
                mode["products"] = products(net, timer, a.reps, only, 3 if a.precision == "bf16x3" else 1)
                for k in ("forward", "dinput", "dweight"):
                    mode[k + "_sum_ms"] = round(sum(r[k + "_ms"] for r in mode["products"]), 3)
            res["precision"] = mode
            net.train_set_precision("fp32")
        if a.loader:
            res.update((cls_loader_row if a.net == "darknet19" else loader_row)(net, batch, timer, max(a.steps, 1), a.warmup, a.reps))
            print("  " + json.dumps(res["loader"]))
        L.y2h_free(d_x)
        L.y2h_free(d_y)
        net.free()
        out.append(res)
    ref = None if a.no_reference else reference_step(tmp, wts, a.net, SIZE, a.ref_batch or ref_batch)
    if ref:
        print("  reference: " + json.dumps(ref))
    print(json.dumps({"tool": "train_latency", "device": darknet.device_name(), "net": a.net, "size": SIZE, "rows": out, "reference": ref}))


if __name__ == "__main__":
    main()
