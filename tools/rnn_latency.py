#!/usr/bin/env python3
"""Per-character latency of the recurrent generation loop (test_char_rnn, rnn.c:225-280) and the throughput of
rnn.train.cfg's shape, on synthetic weights.

    python tools/rnn_latency.py [--iters 200] [--no-train] [--generate N]

Prints one JSON line per case: p50 / p95 per character through network_predict (B=1, T=1, graph replay off and on),
the device time of one character (HIP events around 100 back-to-back y2_forward_device calls), and characters per
second at 128 sequences x 576 steps with the per-layer device times (y2_set_timing).  Where oracle/_ref/ref_driver was
built, the reference's own CPU network_predict per character is timed beside it (ref_driver time, same cfg and weights).
--generate N times text generation instead, rnn.cfg and gru.cfg at 1 and 8 sequences: the device loop (y2_rnn_generate, N
characters per call: wall time per character, and device time per character from HIP events around the call) beside
the loop a caller had to write before it -- one network_predict per character with the sample drawn on the host
(numpy: threshold, fp32 running sum, search), also timed without the sampling.  With Y2_LIB pointing at a build that has
no y2_rnn_generate only that second loop runs.
Kernels per character are not counted here: run this tool under rocprofv3 --kernel-trace --stats for that."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402


def _net(tmp, name, B, T):
    cfg = os.path.join(tmp, "%s_%d_%d.cfg" % (name, B, T))
    with open(cfg, "w") as f:
        f.write(zoo.recurrent_cfg_text(name, B, T))
    w = os.path.join(tmp, name + ".weights")
    if not os.path.exists(w):
        synth.write_recurrent_weights(w, name, 7)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(w)
    return net


def generation(tmp, name, iters, graph):
    L = darknet.lib()
    net = _net(tmp, name, 1, 1)
    net.set_graph(graph)
    x = np.zeros(256, np.float32)
    ts = []
    for i in range(iters + 20):
        x[:] = 0
        x[(i * 7) % 256] = 1
        t0 = time.perf_counter()
        net.network_predict(x)
        if i >= 20:
            ts.append(time.perf_counter() - t0)
    p = C.c_void_p()
    L.y2h_malloc(C.byref(p), 256 * 4)
    s = C.c_void_p(net.stream())
    L.y2h_memcpy_h2d(p, x.ctypes.data, 256 * 4, s)
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.y2h_event_create(C.byref(e0))
    L.y2h_event_create(C.byref(e1))
    net.forward_device(p.value)
    net.sync()
    L.y2h_event_record(e0, s)
    for _ in range(100):
        net.forward_device(p.value)
    L.y2h_event_record(e1, s)
    net.sync()
    ms = C.c_float()
    L.y2h_event_elapsed_ms(e0, e1, C.byref(ms))
    L.y2h_event_destroy(e0)
    L.y2h_event_destroy(e1)
    L.y2h_free(p)
    ts = np.array(ts) * 1e6
    out = dict(net=name, graph=graph, p50_us=round(float(np.percentile(ts, 50)), 1), p95_us=round(float(np.percentile(ts, 95)), 1),
               device_us_per_char=round(ms.value * 10.0, 1), kernels=[net.layer_kernel(i) for i in range(net.n)])
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_driver")
    if os.path.exists(ref) and not graph:
        cfg = os.path.join(tmp, "%s_1_1.cfg" % name)
        r = subprocess.run([ref, "time", cfg, os.path.join(tmp, name + ".weights"), "50"], capture_output=True, text=True, timeout=600)
        if r.returncode == 0 and r.stdout.strip():
            out["ref_cpu_us_per_char"] = round(json.loads(r.stdout.strip().splitlines()[-1])["median_s"] * 1e6, 1)
    net.free()
    return out


def generate(tmp, name, B, N):
    L = darknet.lib()
    net = _net(tmp, name, B, 1)
    net.set_temperature(.7)
    out = dict(net=name, sequences=B, characters=N)
    u = darknet.Network.rnn_uniforms(1, N * B).reshape(N, B) if hasattr(L, "y2_rnn_uniforms") else np.random.RandomState(1).rand(N, B).astype(np.float32)
    # the caller's loop: a one-hot row up, the forward, the probabilities down, the draw on the host
    for sample in (False, True):
        x = np.zeros((B, 256), np.float32)
        c = np.zeros(B, np.int64)
        ts = []
        for i in range(N + 20):
            t0 = time.perf_counter()
            x[np.arange(B), c] = 1
            p = net.network_predict(x).reshape(B, -1)[:, :256]
            x[np.arange(B), c] = 0
            if sample:
                p = np.where(p < 1e-4, np.float32(0), p)
                a = np.cumsum(p * (1 / p.sum(axis=1, dtype=np.float32))[:, None], axis=1, dtype=np.float32)
                c = np.minimum((a < u[i % N][:, None]).sum(axis=1), 255)
            else:
                c = (c * 7 + 1) % 256
            if i >= 20:
                ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e6
        key = "predict_loop_host_sampling" if sample else "predict_loop_no_sampling"
        out[key + "_us_per_char"] = round(float(np.percentile(ts, 50)), 1)
        out[key + "_mean_us_per_char"] = round(float(ts.mean()), 1)
    if hasattr(L, "y2_rnn_generate"):
        s = C.c_void_p(net.stream())
        e0, e1 = C.c_void_p(), C.c_void_p()
        L.y2h_event_create(C.byref(e0))
        L.y2h_event_create(C.byref(e1))
        seed = np.zeros((1, B), np.int32)
        net.rnn_generate(seed, 16, u[:16])
        wall, dev = [], []
        for _ in range(5):
            net.sync()
            L.y2h_event_record(e0, s)
            t0 = time.perf_counter()
            net.rnn_generate(seed, N, u)
            wall.append((time.perf_counter() - t0) / N * 1e6)
            L.y2h_event_record(e1, s)
            net.sync()
            ms = C.c_float()
            L.y2h_event_elapsed_ms(e0, e1, C.byref(ms))
            dev.append(ms.value * 1e3 / N)
        L.y2h_event_destroy(e0)
        L.y2h_event_destroy(e1)
        out["device_loop_us_per_char"] = round(float(np.median(wall)), 1)
        out["device_loop_runs_us_per_char"] = [round(v, 1) for v in wall]
        out["device_loop_device_us_per_char"] = round(float(np.median(dev)), 1)
    out["kernels"] = [net.layer_kernel(i) for i in range(net.n)]
    net.free()
    return out


def throughput(tmp, name, B=128, T=576):
    net = _net(tmp, name, B, T)
    x = synth.char_rows(11, B, T, 256, True)
    net.network_predict(x)
    t0 = time.perf_counter()
    net.network_predict(x)
    dt = time.perf_counter() - t0
    net.set_timing(True)
    net.network_predict(x)
    ms = net.layer_times_ms()
    out = dict(net=name, sequences=B, steps=T, chars_per_s=round(B * T / dt), forward_s=round(dt, 4),
               layer_ms=[round(float(v), 3) for v in ms], kernels=[net.layer_kernel(i) for i in range(net.n)])
    net.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--generate", type=int, default=0, metavar="N", help="time generating N characters per call instead")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if a.generate:
            for name in ("rnn", "gru"):
                for B in (1, 8):
                    print(json.dumps(generate(tmp, name, B, a.generate)), flush=True)
            return
        for name in ("rnn", "gru"):
            for graph in (False, True):
                print(json.dumps(generation(tmp, name, a.iters, graph)), flush=True)
        if not a.no_train:
            print(json.dumps(throughput(tmp, "rnn")), flush=True)


if __name__ == "__main__":
    main()
