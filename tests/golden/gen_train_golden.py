#!/usr/bin/env python3
"""Reference-run fixtures for training: tests/golden/train_A.npz, train_B.npz, train_C.npz, train_D.npz.

Everything stored comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by oracle/build_ref.sh where
the reference checkout exists) through tests/native/train_ref.c, compiled here into a temporary directory: three
train_network_datum calls on the networks of tests/train_rule.py NETS from the parameters and inputs that module derives
from the stored seed, and get_current_rate of every supported policy (RATE_NETS) at RATE_SEEN.

  A, B   every array of every layer after step 1; parameters, update buffers and the loss after steps 2 and 3; the
         reference's network_predict of the first input after its three steps
  C      step 1 likewise, then the parameters, update buffers and loss after step 3 only; its arrays above 40000 values, and the
         step-3 update buffers, kept as every 61st value (train_rule.subsample)
  D      rate_<policy>: float32 [len(RATE_SEEN)]

The generator runs the float64 rule first and ASSERTS that no pre-activation of a leaky / relu layer is closer to 0 than
1e-4 and that no maxpool window's two largest values are closer than 1e-4, over all three steps; A and B search their
seed for that, C gets it by construction (train_rule.C_GAIN).  It also asserts that the rule reproduces every stored array
within 1e-5 relative (C, whose reductions are 4096 long: 1e-4).  It exits non-zero rather than write a fixture that breaks either.

    python tests/golden/gen_train_golden.py
    python tests/golden/gen_train_golden.py --driver-only     # only leave the compiled driver as oracle/_ref/train_ref, for
                                                              # the reference timing of tools/train_latency.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_rule as T  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

SEED0 = {"A": 4101, "B": 5203, "C": 6301}
UPDATES = ("weight_updates", "bias_updates", "scale_updates")
# how far the reference's fp32 arrays may lie from the float64 rule: about a hundred roundings on A and B (what
# tests/test_train_host.py holds them to); C sums 4096 values per filter and cancels in the batch-norm backward
RULE_BOUND = {"A": 1e-5, "B": 1e-5, "C": 1e-4}


def build_train_ref(tmp, rpath=REF_DIR):
    """the link line of oracle/build_ref.sh:36-38"""
    exe = os.path.join(tmp, "train_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "train_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + rpath, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread"])
    return exe


def rule_run(name, seed):
    spec = T.NETS[name]
    t = T.Trainer(spec, T.params_for(name, seed))
    snaps, losses = [], []
    for k in range(1, T.STEPS + 1):
        x, y = T.inputs(spec, seed, k)
        losses.append(t.step(x, y))
        snaps.append([{a: np.array(v) for a, v in t.arrays(i).items()} for i in range(len(spec["layers"]))])
    return t, snaps, losses


def reference_run(exe, tmp, name, seed):
    spec = T.NETS[name]
    work = os.path.join(tmp, "%s_%d" % (name, seed))
    os.makedirs(work, exist_ok=True)
    cfg, wts, _ = T.materialize(work, name, seed)
    for k in range(1, T.STEPS + 1):
        x, y = T.inputs(spec, seed, k)
        x.astype(np.float32).tofile(os.path.join(work, "x_%d.bin" % k))
        y.astype(np.float32).tofile(os.path.join(work, "y_%d.bin" % k))
    subprocess.check_call([exe, "steps", cfg, wts, work, str(T.STEPS), work], stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)

    def get(stem):
        p = os.path.join(work, stem + ".bin")
        return np.fromfile(p, dtype=np.float32) if os.path.exists(p) else None
    return get


def fixture(exe, tmp, name):
    for attempt in range(60):
        seed = SEED0[name] + 97 * attempt
        t, snaps, losses = rule_run(name, seed)
        if t.min_preact >= T.KINK and t.min_gap >= T.KINK:
            break
        print("  %s: seed %d rejected: smallest |pre-activation| %.2e, smallest maxpool gap %.2e" % (name, seed, t.min_preact, t.min_gap))
    else:
        sys.exit("%s: no seed keeps every kink %g away" % (name, T.KINK))
    assert t.min_preact >= T.KINK and t.min_gap >= T.KINK
    get = reference_run(exe, tmp, name, seed)
    fix = {"seed": np.int64(seed), "min_preact": np.float64(t.min_preact), "min_gap": np.float64(min(t.min_gap, 1e30))}
    worst = 0.0
    for k in range(1, T.STEPS + 1):
        loss = get("s%d_loss" % k)
        fix["s%d_loss" % k] = loss
        worst = max(worst, abs(float(loss[0]) - losses[k - 1]) / abs(losses[k - 1]))
        for i in range(len(T.NETS[name]["layers"])):
            for a, want in snaps[k - 1][i].items():
                if k > 1 and a not in T.PARAMS + UPDATES:
                    continue
                if name == "C" and 1 < k < T.STEPS:
                    continue                                   # C: step 1 and the last step only (size)
                got = get("s%d_l%d_%s" % (k, i, a))
                assert got is not None and got.size == want.size, "%s: step %d layer %d has no %s" % (name, k, i, a)
                e = T.err(got, want.reshape(-1))
                assert e <= RULE_BOUND[name], "%s: the rule differs from the reference in step %d layer %d %s: %.3g" % (name, k, i, a, e)
                worst = max(worst, e)
                fix["s%d_l%d_%s" % (k, i, a)] = T.subsample(name, a, got, k).copy()
    fix["predict"] = get("predict")
    print("%s: seed %d, |pre-activation| >= %.3g, maxpool gap >= %.3g, rule vs reference <= %.3g" % (name, seed, t.min_preact, t.min_gap, worst))
    return fix


def rates(exe, tmp):
    fix = {"seen": np.array(T.RATE_SEEN, np.int64)}
    for name in T.RATE_NETS:
        cfg, out = os.path.join(tmp, "rate_%s.cfg" % name), os.path.join(tmp, "rate_%s.bin" % name)
        with open(cfg, "w") as f:
            f.write(T.net_text(T.rate_spec(name)))
        subprocess.check_call([exe, "rates", cfg, out] + [str(s) for s in T.RATE_SEEN], stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        fix["rate_" + name] = np.fromfile(out, dtype=np.float32)
        assert fix["rate_" + name].size == len(T.RATE_SEEN)
    return fix


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    if "--driver-only" in sys.argv:
        print("built " + build_train_ref(REF_DIR, "$ORIGIN"))
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_train_ref(tmp)
        for name in sorted(T.NETS):
            out = os.path.join(ROOT, "tests", "golden", "train_%s.npz" % name)
            write_npz(out, fixture(exe, tmp, name))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))
        out = os.path.join(ROOT, "tests", "golden", "train_D.npz")
        write_npz(out, rates(exe, tmp))
        print("wrote %s" % out)


if __name__ == "__main__":
    main()
