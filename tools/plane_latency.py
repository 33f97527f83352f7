#!/usr/bin/env python3
"""What the table-plane removal of the Grasp branch costs on the device, at the Kinect's shapes: colour 1920x1080, depth
512x424, 50 hypotheses (KinectUtil_with_cam.cpp:364-377 calls desk_seg(1.0) on every frame).

Every time is measured between two events on the engine's stream (y2h_event_elapsed_ms), p50 / p90 of --iters calls after
--warmup.  y2_depth_upload with the removal off and on take turns inside one loop; then every new launch alone, on buffers
of this tool's own, with the bytes it must stream:
  count     2 B of depth + 8 B of table per depth pixel, once; 50 point-plane tests per pixel in registers
  sums      the same read; ten doubles per workgroup out
  fit       one workgroup: the slab of partials in index order, the eigen routine, the record
  apply     the same read; 2 B of grasp depth per depth pixel out
  register  4 B of dxy in and 2 B of grasp16 out per colour pixel (the gather hits a 0.43 MB plane in L2)

usage: plane_latency.py [--iters 200] [--warmup 20] [--hyps 50]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402
from depth_latency import DH, DW, H, W, Timer, dev_array  # noqa: E402


class PlaneJob(C.Structure):   # include/y2_hip.h y2h_plane_job
    _fields_ = [("depth", C.c_void_p), ("tab", C.c_void_p), ("triples", C.c_void_p), ("n", C.c_long), ("iters", C.c_int),
                ("far_mm", C.c_float), ("dist_m", C.c_float), ("counts", C.c_void_p), ("slab", C.c_void_p), ("rec", C.c_void_p),
                ("grasp_depth", C.c_void_p)]


def scene():
    """a table seen from above its near edge, three boxes on it, 3 % dropped pixels, the far end beyond 1 m"""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:DH, 0:DW].astype(np.float64)
    table = np.stack([(xx - DW / 2) / 365., (DH / 2 - yy) / 365.], axis=-1).astype(np.float32)
    n = np.array([0.04, 0.5, 0.865])
    n /= np.linalg.norm(n)
    z = 0.70 / (n[0] * table[..., 0] + n[1] * table[..., 1] + n[2])
    mm = np.rint(z * 1000.0) + rng.integers(-4, 5, (DH, DW))
    for k in range(3):
        mm[60 + 30 * k:130 + 30 * k, 60 + 150 * k:130 + 150 * k] -= 120
    mm[rng.random((DH, DW)) < 0.03] = 0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.stack([(xs - 210) * np.float32(DW / 1500.), ys * np.float32(DH / H) + np.float32(0.3)], axis=-1).astype(np.float32)
    return mm.astype(np.uint16), m, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hyps", type=int, default=50)
    a = ap.parse_args()
    L = darknet.lib()
    L.y2h_depth_align.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 5
    L.y2h_plane_remove.argtypes = [C.POINTER(PlaneJob), C.c_int, C.c_void_p]
    L.y2h_plane_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_plane_chunks.restype = C.c_ulong
    L.y2h_plane_chunks.argtypes = [C.c_long]
    tmp = tempfile.mkdtemp()
    cfg, wts = os.path.join(tmp, "n.cfg"), os.path.join(tmp, "n.weights")
    open(cfg, "w").write(zoo.cfg_text("tiny-yolo-voc", 416, 416, 1))
    synth.write_weights(wts, zoo.resolve("tiny-yolo-voc", 416), 7)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    depth, m, table = scene()
    net.depth_set_camera_table(table)
    tm = Timer(L, L.y2_stream(net.net))

    def upload(on):
        net.depth_set_plane_removal(1.0, 0.02, a.hyps if on else 0, 2017)
        net.depth_upload(depth, None, m)

    upload(True)
    plane = net.depth_plane()
    res = tm.stats_turns({"depth_upload_removal_off": lambda: upload(False), "depth_upload_removal_on": lambda: upload(True)},
                         a.iters, a.warmup)
    # the launches alone
    nd, npix = DH * DW, H * W
    tri = darknet.plane_samples(depth, 1.0, a.hyps, 2017)
    d_depth, d_map, d_tab, d_tri = (dev_array(L, x) for x in (depth, m, table, tri))
    d16, d8, dper, dxy, d_gd, d_g16 = (dev_array(L, np.zeros(n, np.uint8)) for n in (npix * 2, npix, npix, npix * 4, nd * 2, npix * 2))
    chunks = int(L.y2h_plane_chunks(nd))
    d_cnt, d_slab, d_rec = (dev_array(L, np.zeros(n, np.uint8)) for n in (260 * 4, chunks * 80, 64))
    assert L.y2h_depth_align(d_depth, None, d_map, DH, DW, H, W, d16, d8, dper, dxy, tm.stream) == 0
    job = PlaneJob(d_depth, d_tab, d_tri, nd, a.hyps, 1000.0, 0.02, d_cnt, d_slab, d_rec, d_gd)
    assert L.y2h_plane_remove(C.byref(job), 31, tm.stream) == 0 and L.y2h_stream_sync(tm.stream) == 0
    # each single stage runs on the state the full chain left: the counts stay finished while sums / fit / apply are timed
    # (the count stage timed alone adds onto them, so it goes last, behind a clear of its own)
    for name, stages in (("plane_all", 31), ("plane_sums", 4), ("plane_fit", 8), ("plane_apply", 16), ("plane_clear", 1),
                         ("plane_clear_count", 3)):
        res[name] = tm.stats(lambda: L.y2h_plane_remove(C.byref(job), stages, tm.stream), a.iters, a.warmup)
    res["plane_register"] = tm.stats(lambda: L.y2h_plane_register(d_gd, dxy, H, W, DW, d_g16, tm.stream), a.iters, a.warmup)
    added = res["depth_upload_removal_on"]["p50_ms"] - res["depth_upload_removal_off"]["p50_ms"]
    print("colour %dx%d, depth %dx%d, %d hypotheses; plane found %d (hypothesis %d, %d of %d valid points, %d removed); %d timed"
          " calls after %d warm-up (event ms on the engine's stream):"
          % (W, H, DW, DH, a.hyps, plane["found"], plane["best"], plane["best_count"], plane["valid_points"], plane["removed"],
             a.iters, a.warmup))
    for k, v in res.items():
        print("  %-32s p50 %8.4f   p90 %8.4f" % (k, v["p50_ms"], v["p90_ms"]))
    print("  removal on over off at the same inputs: %+.4f ms p50" % added)
    read_b = nd * 10
    for name, out_b in (("plane_clear_count", 0), ("plane_sums", chunks * 80), ("plane_apply", nd * 2)):
        print("  %s: %.2f MB streamed -> %.0f GB/s" % (name[6:], (read_b + out_b) / 1e6, (read_b + out_b) / 1e6 / res[name]["p50_ms"]))
    print("  register: %.1f MB streamed -> %.0f GB/s" % (npix * 6 / 1e6, npix * 6 / 1e6 / res["plane_register"]["p50_ms"]))
    print(json.dumps({"iters": a.iters, "hyps": a.hyps, "device": darknet.device_name(), "added_p50_ms": round(added, 4),
                      "plane": plane, **res}))
    net.free()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
