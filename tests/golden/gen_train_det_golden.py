#!/usr/bin/env python3
"""Reference-run fixtures for detector training: tests/golden/train_E.npz, train_F.npz, train_G.npz.

Everything stored comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by oracle/build_ref.sh where
the reference checkout exists) through tests/native/train_det_ref.c, compiled here into a temporary directory with the link
line of gen_train_golden.py: three train_network_datum calls on the networks of tests/train_det_rule.py NETS, from the
parameters, inputs and truths that module derives from the stored seed, with *net.seen started at the network's `seen`.

  E, F, G  every array of every layer after step 1 (full arrays); parameters, update buffers and the loss after steps 2 and
         3; the reference's network_predict of the first input after its three steps

The generator runs the float64 rule first and ASSERTS that every discrete decision of the run keeps a margin of 1e-4 over
all three steps: leaky pre-activations, maxpool windows, |best_iou - thresh|, the gap between the best and second anchor
of a truth, |iou - .5| and the distance of truth.x*w / truth.y*h from an integer.  It searches the seed for that.  For E it
also asserts that some prediction exceeds thresh against a truth, and that two truths of image 0 land on one
(cell, anchor).  It then asserts that the rule reproduces every stored array within 1e-5 relative, and exits non-zero
rather than write a fixture that breaks any of it.

    python tests/golden/gen_train_det_golden.py
    python tests/golden/gen_train_det_golden.py --driver-only   # only leave the compiled driver as oracle/_ref/train_det_ref,
                                                                # for the reference timing of tools/train_latency.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_det_rule as D  # noqa: E402
from tests import train_rule as T  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

SEED0 = {"E": 7103, "F": 8209, "G": 9311}
UPDATES = ("weight_updates", "bias_updates", "scale_updates")
RULE_BOUND = 1e-5


def build_driver(tmp, rpath=REF_DIR):
    """the link line of gen_train_golden.build_train_ref"""
    exe = os.path.join(tmp, "train_det_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "train_det_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + rpath, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread"])
    return exe


def reference_run(exe, tmp, name, seed):
    spec = D.NETS[name]
    work = os.path.join(tmp, "%s_%d" % (name, seed))
    os.makedirs(work, exist_ok=True)
    cfg, wts, _ = D.materialize(work, name, seed)
    for k in range(1, D.STEPS + 1):
        x, y = D.inputs(name, seed, k)
        x.astype(np.float32).tofile(os.path.join(work, "x_%d.bin" % k))
        y.astype(np.float32).tofile(os.path.join(work, "y_%d.bin" % k))
    subprocess.check_call([exe, "steps", cfg, wts, work, str(D.STEPS), work, str(spec["seen"])], stderr=subprocess.DEVNULL,
                          stdout=subprocess.DEVNULL)

    def get(stem):
        p = os.path.join(work, stem + ".bin")
        return np.fromfile(p, dtype=np.float32) if os.path.exists(p) else None
    return get


def same_cell_and_anchor(name, seed):
    """E: the first two truths of image 0 pick one (cell, anchor) on step 1 -- with bias_match the anchor depends on the
    truth's size alone"""
    spec = D.NETS[name]
    reg = spec["layers"][-1][1]
    _, (_, gh, gw) = D.shapes(spec)[-1]
    y = D.truths(name, 1)[0]
    pick = []
    for t in (0, 1):
        ious = [D.box_iou((0, 0, reg["anchors"][2 * a] / gw, reg["anchors"][2 * a + 1] / gh), (0, 0, y[t, 2], y[t, 3])) for a in range(reg["num"])]
        pick.append((int(y[t, 0] * gw), int(y[t, 1] * gh), int(np.argmax(ious))))
    return pick[0] == pick[1]


def fixture(exe, tmp, name):
    spec = D.NETS[name]
    reg = spec["layers"][-1][1]
    for attempt in range(60):
        seed = SEED0[name] + 97 * attempt
        t, snaps, losses, stats = D.rule_snapshots(name, seed)
        if D.margins_ok(t):
            break
        print("  %s: seed %d rejected: |pre-activation| %.2e, maxpool gap %.2e, margins %s" % (name, seed, t.min_preact, t.min_gap, t.margins))
    else:
        sys.exit("%s: no seed keeps every margin %g away" % (name, T.KINK))
    assert D.margins_ok(t)
    if name == "E":
        assert t.margins["max_best_iou"] > reg["thresh"], "E: no prediction exceeds thresh against a truth"
        assert reg["bias_match"] and same_cell_and_anchor(name, seed), "E: the first two truths of image 0 must share (cell, anchor)"
        assert spec["seen"] + D.STEPS * spec["batch"] < 12800
    elif name == "F":
        assert spec["seen"] >= 12800
    get = reference_run(exe, tmp, name, seed)
    fix = {"seed": np.int64(seed), "min_preact": np.float64(t.min_preact), "min_gap": np.float64(min(t.min_gap, 1e30))}
    for k in ("thresh", "anchor", "recall", "cell"):
        fix["margin_" + k] = np.float64(t.margins[k])
    worst = 0.0
    for k in range(1, D.STEPS + 1):
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
    if "--driver-only" in sys.argv:
        print("built " + build_driver(REF_DIR, "$ORIGIN"))
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in sorted(D.NETS):
            out = os.path.join(ROOT, "tests", "golden", "train_%s.npz" % name)
            write_npz(out, fixture(exe, tmp, name))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
