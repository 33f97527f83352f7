"""bench.py's command line and output dump, without a GPU: what a plain run does by default, which figures wait for
--full, and the layout of --dump-outputs."""
import os
import sys

import numpy as np
import pytest

import bench
from sr_object_detection_amd import darknet


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse_args()


def test_plain_run_skips_the_extras_and_full_restores_them(monkeypatch):
    a = _args(monkeypatch, "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.host_input, a.dump_outputs) == (7, 2, False, "off", None)
    a = _args(monkeypatch, "--full")
    assert a.full and a.host_input == "also"
    a = _args(monkeypatch, "--host-input", "only")            # an explicit choice holds either way
    assert not a.full and a.host_input == "only"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _args(monkeypatch, *argv)


def _dets(rng, counts):
    out = []
    for n in counts:
        d = np.zeros(n, dtype=darknet.DET_DTYPE)
        for f in ("x", "y", "w", "h", "prob"):
            d[f] = rng.random(n, dtype=np.float32)
        d["obj_id"] = rng.integers(0, 80, n)
        out.append(d)
    return out


def test_dump_outputs_detector_layout(tmp_path):
    counts = np.array([3, 0, 2], dtype=np.int32)
    dets = _dets(np.random.default_rng(5), counts)
    bench.dump_outputs(str(tmp_path), True, dets, counts, 3)
    assert sorted(os.listdir(tmp_path)) == ["counts.npy", "detections.npy"]
    got = np.load(tmp_path / "detections.npy")
    assert got.dtype == np.float64 and got.shape == (5, 7)
    assert np.array_equal(np.load(tmp_path / "counts.npy"), counts.astype(np.float64))
    assert np.array_equal(got[:, 0], [0, 0, 0, 2, 2])
    want = np.concatenate([np.stack([d[f].astype(np.float64) for f in ("x", "y", "w", "h", "prob", "obj_id")], 1) for d in dets])
    assert np.array_equal(got[:, 1:], want)                   # float32 fields and class ids exactly


def test_dump_outputs_classifier_and_size_cap(tmp_path, monkeypatch):
    scores = np.random.default_rng(1).random(16 * 1000, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "all"), False, scores, np.zeros(1), 16)
    got = np.load(tmp_path / "all" / "class_scores.npy")
    assert got.dtype == np.float32 and np.array_equal(got, scores.reshape(16, 1000))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 5 * 4008)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), False, scores, np.zeros(1), 16)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_LIMIT_BYTES
    rows = np.load(a / "class_scores_rows.npy")
    assert np.array_equal(rows, np.load(b / "class_scores_rows.npy")) and np.all(np.diff(rows) > 0)   # seeded, ascending
    assert np.array_equal(np.load(a / "class_scores.npy"), scores.reshape(16, 1000)[rows.astype(int)])
