#!/usr/bin/env python3
"""Reference-run fixtures for the multi-view classifier evaluations (classifier.c:336-593): tests/golden/tta_mini.npz.

For four frames of sizes 50x40, 40x50, 64x64 and 33x47 every view of the three modes is built with the rule of
tests/tta_rule.py (resizes by the oracle's resize_image, which is pinned to image.c:1950), one cfg per distinct view
size is written with batch = the number of views of that size, and the COMPILED REFERENCE (oracle/_ref/ref_driver net,
built by oracle/build_ref.sh where the reference checkout exists) predicts them.  Stored: the frames, the per-view rows,
the sequential fp32 sums and the top-3 of each sum, for CROP10, for MULTI with scales (24, 32, 40) and for FULL.

The generator searches its seeds: in every stored sum the gaps between the 1st .. 4th largest values must be at least
1e-3, so that top-3 is decided well inside the fast path's error; and the reference must have accepted every size.  It
fails rather than write a fixture that breaks either condition.

    python tests/golden/gen_tta_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_capi  # noqa: E402
from tests import tta_rule as R  # noqa: E402

REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
OUT = os.path.join(ROOT, "tests", "golden", "tta_mini.npz")
MODES = (("crop10", R.CROP10, None), ("multi", R.MULTI, R.MINI_SCALES), ("full", R.FULL, None))
MIN_GAP = 1e-3
SEED0, FRAME_SEED0 = 301, 0x7A5


def reference_predict(tmp, seed):
    def predict(size, x):
        w, h = size
        cfg, wts = R.write_mini(tmp, seed, w, h, len(x))
        inp = os.path.join(tmp, "in.bin")
        np.ascontiguousarray(x, dtype=np.float32).tofile(inp)
        out = os.path.join(tmp, "out_%dx%d_%d" % (w, h, len(x)))
        os.makedirs(out, exist_ok=True)
        subprocess.check_call([REF_DRIVER, "net", cfg, wts, inp, out, "0", "0", "0"], stderr=subprocess.DEVNULL,
                              stdout=subprocess.DEVNULL)
        meta = dict(line.split() for line in open(os.path.join(out, "meta.txt")))
        assert (int(meta["w"]), int(meta["h"]), int(meta["batch"])) == (w, h, len(x)), "the reference did not accept %dx%d" % size
        rows = np.fromfile(os.path.join(out, "out.bin"), dtype=np.float32)
        assert rows.size == len(x) * R.MINI_CLASSES, "the reference did not accept %dx%d" % size
        return rows.reshape(len(x), R.MINI_CLASSES)
    return predict


def attempt(seed, frame_seed):
    frames = R.mini_frames(frame_seed)
    fix = {"seed": seed, "frame_seed": frame_seed, "scales": np.array(R.MINI_SCALES, np.int32)}
    for i, f in enumerate(frames):
        fix["frame_%d" % i] = f
    worst = np.inf
    with tempfile.TemporaryDirectory() as tmp:
        predict = reference_predict(tmp, seed)
        for name, mode, scales in MODES:
            views, per = R.mode_views(mode, frames, oracle_capi.resize_image, scales)
            rows = R.rows_of(views, predict)
            sums = R.sums_of(rows, per)
            for s in sums:
                top = np.sort(s.astype(np.float64))[::-1][:4]
                worst = min(worst, float(np.min(-np.diff(top))))
            fix[name + "_rows"] = rows.reshape(len(frames), per, -1)
            fix[name + "_sums"] = sums
            fix[name + "_top3"] = np.stack([R.top_k(s, 3) for s in sums])
            fix[name + "_sizes"] = np.array([s for s, _ in views], np.int32).reshape(len(frames), per, 2)
    fix["min_gap"] = np.float64(worst)
    return fix, worst


def main():
    if not os.path.exists(REF_DRIVER):
        sys.exit("oracle/_ref/ref_driver missing: run oracle/build_ref.sh where the reference checkout exists")
    oracle_capi.build()
    for k in range(40):
        seed, frame_seed = SEED0 + 100 * k, FRAME_SEED0 + 1000 * k
        fix, worst = attempt(seed, frame_seed)
        if worst >= MIN_GAP:
            break
        print("  seeds (%d, %d) rejected: smallest gap among the four largest sums %.2e" % (seed, frame_seed, worst))
    else:
        sys.exit("no seed keeps the top-4 gaps of every sum above %g" % MIN_GAP)
    assert worst >= MIN_GAP
    np.savez_compressed(OUT, **fix)
    print("wrote %s (%d KB): seeds (%d, %d), smallest top-4 gap %.3e" % (OUT, os.path.getsize(OUT) // 1024, seed, frame_seed, worst))


if __name__ == "__main__":
    main()
