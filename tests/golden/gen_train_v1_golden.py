#!/usr/bin/env python3
"""Reference-run fixtures for YOLOv1 training: tests/golden/train_H.npz and train_I.npz.

Everything stored comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by oracle/build_ref.sh where
the reference checkout exists) through tests/native/train_v1_ref.c, compiled here into a temporary directory with the link
line of gen_train_det_golden.py: three train_network_datum calls, srand(step) before each, on the networks of
tests/train_v1_rule.py NETS, from the parameters, inputs and truths that module derives from the stored seed.

  H, I   every array of every layer after step 1 (full arrays; for I's [dropout] its rand); parameters, update buffers and
         the loss after steps 2 and 3; the reference's network_predict of the first input after its three steps

The generator runs the float64 rule first and ASSERTS that every discrete decision of the run keeps a margin of 1e-4 over
all three steps: leaky pre-activations, maxpool windows, the gap between the best and the second IoU of an object cell,
`iou > 0` against the rmse branch, the gap between the rmse values, and truth.w * truth.h against .1 under forced.  It
searches the seed for that.  For H it also asserts that the truths hold an image without objects, an image with an object
in every cell and an object cell none of whose boxes has a positive IoU.  It then asserts that the rule reproduces every
stored array within 1e-5 relative (I's rand: exactly), and exits non-zero rather than write a fixture that breaks any of it.

    python tests/golden/gen_train_v1_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_rule as T  # noqa: E402
from tests import train_v1_rule as V  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

SEED0 = {"H": 10103, "I": 11213}
UPDATES = ("weight_updates", "bias_updates", "scale_updates")
RULE_BOUND = 1e-5


def build_driver(tmp):
    """the link line of gen_train_det_golden.build_driver"""
    exe = os.path.join(tmp, "train_v1_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "train_v1_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + REF_DIR, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread"])
    return exe


def reference_run(exe, tmp, name, seed):
    work = os.path.join(tmp, "%s_%d" % (name, seed))
    os.makedirs(work, exist_ok=True)
    cfg, wts, _ = V.materialize(work, name, seed)
    for k in range(1, V.STEPS + 1):
        x, y = V.inputs(name, seed, k)
        x.astype(np.float32).tofile(os.path.join(work, "x_%d.bin" % k))
        y.astype(np.float32).tofile(os.path.join(work, "y_%d.bin" % k))
    subprocess.check_call([exe, "steps", cfg, wts, work, str(V.STEPS), work], stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)

    def get(stem):
        p = os.path.join(work, stem + ".bin")
        return np.fromfile(p, dtype=np.float32) if os.path.exists(p) else None
    return get


def fixture(exe, tmp, name):
    spec = V.NETS[name]
    for attempt in range(400):
        seed = SEED0[name] + 97 * attempt
        t, snaps, losses, stats = V.rule_snapshots(name, seed)
        if V.margins_ok(t):
            break
        print("  %s: seed %d rejected: |pre-activation| %.2e, maxpool gap %.2e, margins %s" % (name, seed, t.min_preact, t.min_gap, t.margins))
    else:
        sys.exit("%s: no seed keeps every margin %g away" % (name, T.KINK))
    if name == "H":
        y = V.truths(name, 1)
        assert (y[:, :, 0].sum(axis=1) == 0).any(), "H: no image without objects"
        assert (y[:, :, 0].sum(axis=1) == y.shape[1]).any(), "H: no image with an object in every cell"
        assert t.margins.get("rmse_cells", 0) >= 1, "H: no object cell takes the rmse branch"
    get = reference_run(exe, tmp, name, seed)
    fix = {"seed": np.int64(seed), "min_preact": np.float64(t.min_preact), "min_gap": np.float64(min(t.min_gap, 1e30))}
    for k in ("iou_gap", "iou_zero", "rmse", "forced"):
        fix["margin_" + k] = np.float64(min(t.margins.get(k, 1e30), 1e30))
    worst = 0.0
    for k in range(1, V.STEPS + 1):
        loss = get("s%d_loss" % k)
        fix["s%d_loss" % k] = loss
        e = abs(float(loss[0]) - losses[k - 1]) / abs(losses[k - 1])
        assert e <= RULE_BOUND, "%s: the rule's loss differs from the reference in step %d: %.3g" % (name, k, e)
        worst = max(worst, e)
        for i in range(len(spec["layers"])):
            for a, want in snaps[k - 1][i].items():
                if k > 1 and a not in T.PARAMS + UPDATES:
                    continue
                got = get("s%d_l%d_%s" % (k, i, a))
                assert got is not None and got.size == want.size, "%s: step %d layer %d has no %s" % (name, k, i, a)
                if a == "rand":
                    assert np.array_equal(got, want.reshape(-1)), "%s: the rule's draws are not the reference's" % name
                e = T.err(got, want.reshape(-1))
                assert e <= RULE_BOUND, "%s: the rule differs from the reference in step %d layer %d %s: %.3g" % (name, k, i, a, e)
                worst = max(worst, e)
                fix["s%d_l%d_%s" % (k, i, a)] = got.copy()
    fix["predict"] = get("predict")
    print("%s: seed %d, |pre-activation| >= %.3g, maxpool gap >= %.3g, margins %s, rule vs reference <= %.3g" % (
        name, seed, t.min_preact, t.min_gap, {k: "%.3g" % v for k, v in t.margins.items()}, worst))
    return fix


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in sorted(V.NETS):
            out = os.path.join(ROOT, "tests", "golden", "train_%s.npz" % name)
            write_npz(out, fixture(exe, tmp, name))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
