#!/usr/bin/env python3
"""Generate tests/golden/{lrn_mini,lrn_route,act_flat,lrn_mini_f16}.npz for the [normalization] / [activation] layers by
running the REFERENCE's own compiled CPU path.

    make -C oracle ref && python tests/golden/gen_lrn_golden.py

For every network of sr_object_detection_amd.zoo.LRN: the cfg text (zoo.lrn_cfg_text), seeded synthetic weights
(synth.write_weights) and a seeded input batch go into a scratch directory, and oracle/_ref/ref_driver runs them through
the reference's parse_network_cfg / load_weights / network_predict.  A fixture holds the input, the final output, the
per-layer statistics, every layer's dump (NCHW, as the reference stores it) and the seeds -- data only.  The .npz files
are written with fixed zip timestamps, so a re-run reproduces them byte for byte.
"""
from __future__ import annotations

import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import synth, zoo  # noqa: E402

REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
OUT = os.path.dirname(os.path.abspath(__file__))

# name (a zoo.LRN network), weight seed, input seed
CASES = [("lrn_mini", 401, 501), ("lrn_route", 411, 511), ("act_flat", 421, 521), ("lrn_mini_f16", 431, 531)]


def save_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed without the wall-clock timestamps"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def case_input(name: str, xseed: int) -> np.ndarray:
    """[batch][3][h][w] in [-1, 1): signed, so that the squares and the activations see both signs"""
    w, h, b, _ = zoo.LRN[name]
    return (synth.image_batch(b, 3, h, w, xseed) * np.float32(2) - np.float32(1)).astype(np.float32)


def run_case(name, wseed, xseed):
    w, h, b, _ = zoo.LRN[name]
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "net.cfg")
        with open(cfg, "w") as f:
            f.write(zoo.lrn_cfg_text(name))
        wts = os.path.join(tmp, "net.weights")
        synth.write_weights(wts, zoo.lrn_resolve(name), wseed, 1.0)
        x = case_input(name, xseed)
        inp = os.path.join(tmp, "x.bin")
        x.tofile(inp)
        subprocess.check_call([REF_DRIVER, "net", cfg, wts, inp, tmp, "0", "0", "1"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        fix = {"x": x, "out": np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float32).reshape(b, -1),
               "seeds": np.array([wseed, xseed], np.int64)}
        stats = np.loadtxt(os.path.join(tmp, "layers.txt"), dtype=np.float64, ndmin=2)
        fix["layer_stats"] = stats
        for i in range(stats.shape[0]):
            p = os.path.join(tmp, "layer_%02d.bin" % i)
            if os.path.exists(p):
                fix["layer_%02d" % i] = np.fromfile(p, dtype=np.float32)
    save_npz(os.path.join(OUT, name + ".npz"), fix)
    print("%-14s out %s  max|out| %.4g  %d bytes" % (name, fix["out"].shape, float(np.abs(fix["out"]).max()),
                                                     os.path.getsize(os.path.join(OUT, name + ".npz"))))


def main():
    if not os.path.exists(REF_DRIVER):
        sys.exit("gen_lrn_golden: %s is missing (make -C oracle ref where the reference checkout exists)" % REF_DRIVER)
    for case in CASES:
        run_case(*case)


if __name__ == "__main__":
    main()
