#!/usr/bin/env python3
"""Generate tests/golden/{layer_short,layer_dense,layer_xnor}.npz for the layers between the convolutions -- [shortcut] in
three geometries, [crop], a standalone [batchnorm], [local], [connected], an xnor convolution -- by running the REFERENCE's
own compiled CPU path.

    make -C oracle ref && python tests/golden/gen_layer_golden.py

For every network of tests/layer_rule.py NETS: the cfg text (zoo.cfg_text with the spec), seeded synthetic weights
(synth.write_weights) and a seeded input batch in [0, 1) go into a scratch directory, and oracle/_ref/ref_driver runs them
through the reference's parse_network_cfg / load_weights / network_predict.  A fixture holds the input, the final output,
the per-layer statistics, every layer's dump (NCHW, as the reference stores it) and the seeds -- data only.  The .npz files
are written with fixed zip timestamps, so a re-run reproduces them byte for byte.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import synth, zoo  # noqa: E402
from tests import layer_rule  # noqa: E402
from tests.golden.gen_lrn_golden import save_npz  # noqa: E402

REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
OUT = os.path.dirname(os.path.abspath(__file__))


def run_case(name):
    w, h, b, spec, wseed, xseed = layer_rule.NETS[name]
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "net.cfg")
        with open(cfg, "w") as f:
            f.write(zoo.cfg_text(name, w, h, b, spec=spec))
        wts = os.path.join(tmp, "net.weights")
        synth.write_weights(wts, zoo.resolve(spec, w, h), wseed, 1.0)
        x = layer_rule.net_input(name)
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
    path = os.path.join(OUT, name + ".npz")
    save_npz(path, fix)
    print("%-12s out %s  max|out| %.4g  %d layers  %d bytes" % (name, fix["out"].shape, float(np.abs(fix["out"]).max()),
                                                               stats.shape[0], os.path.getsize(path)))
    return os.path.getsize(path)


def main():
    if not os.path.exists(REF_DRIVER):
        sys.exit("gen_layer_golden: %s is missing (make -C oracle ref where the reference checkout exists)" % REF_DRIVER)
    total = sum(run_case(name) for name in layer_rule.NETS)
    print("total %d bytes" % total)
    assert total < 300 * 1024


if __name__ == "__main__":
    main()
