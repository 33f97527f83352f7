"""bench.py as the driver runs it: a plain run times exactly --steps steps and carries none of the --full figures, and
--dump-outputs writes the detections of the last timed step -- the same from run to run, and the same as one
detect() call of the library on the benchmark's frames and weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from sr_object_detection_amd import darknet, synth, zoo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "yolo416_b1",
                        "--steps", "7", "--warmup", "2", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_and_dumped_outputs(tmp_path):
    lines = [_plain_run(str(tmp_path / r)) for r in ("a", "b")]
    for line in lines:
        assert line["metric"] == "images/sec yolo 416x416 fp32" and line["unit"] == "images/sec"
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 7
        assert line["value"] > 0 and abs(line["ms_per_step"] - 1e3 / line["value"]) < 0.01 * line["ms_per_step"] + 1e-3
        assert line["roofline"] is not None
        for k in ("cpu_baseline", "host_input", "map_equiv_vs_cpu", "latency", "mfma_f32_clock_ghz"):
            assert line[k] is None, k
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["counts.npy", "detections.npy"]
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
    det, counts = np.load(a / "detections.npy"), np.load(a / "counts.npy")
    assert det.dtype == counts.dtype == np.float64 and counts.sum() == len(det) == lines[0]["config"]["detections_in_last_batch"]
    # the same frames and weights through the library directly
    cfg = bench.write_cfg(str(tmp_path), "yolo", 416, 1)
    wts = str(tmp_path / "w.weights")
    synth.write_weights(wts, zoo.resolve("yolo", 416), 31)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    dets, want = net.detect(synth.image_batch(1, 3, 416, 416, seed=0xC0FFEE), bench.THRESH, bench.NMS)
    assert np.array_equal(counts, want.astype(np.float64)) and int(want.sum()) > 0
    d = dets[0]
    assert np.array_equal(det[:, 1:], np.stack([d[f].astype(np.float64) for f in ("x", "y", "w", "h", "prob", "obj_id")], 1))
    net.free()
