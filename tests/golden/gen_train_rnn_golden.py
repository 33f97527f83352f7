#!/usr/bin/env python3
"""Reference-run fixtures for char-rnn training: tests/golden/train_rnn_J.npz, _K.npz, _L.npz and train_rnn_long.npz.

Everything stored comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by oracle/build_ref.sh where
the reference checkout exists) through tests/native/train_rnn_ref.c, compiled here into a temporary directory with the link
line of gen_train_v1_golden.py: three train_network_datum calls on the networks of tests/train_rnn_rule.py NETS, from the
parameters, inputs and truths that module derives from the stored seed.

  J, K, L  after step 1 every array of every sub-layer of every [rnn], its state history, and every array of the other
           layers; after steps 2 and 3 the parameters, the update buffers and the loss; the reference's network_predict
           of the first input after its three steps
  long     the reference's thirty losses on tests/train_rnn_rule.py LONG (logistic only: no kink) and their largest relative
           deviation from the float64 rule's: the measure the GPU's loss curve is held to four times of

The generator runs the float64 rule first and searches the seed until no leaky / relu pre-activation lies within 1e-4 of
zero over all three steps and the FLOAT32 rule reproduces every
stored array of the reference within 1e-5 relative; it exits non-zero rather than write a fixture that breaks either.

    python tests/golden/gen_train_rnn_golden.py [J|K|L ...]      (names: only those fixtures)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import train_rule as T  # noqa: E402
from tests import train_rnn_rule as R  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

SEED0 = {"J": 20011, "K": 21013, "L": 22003}
RULE_BOUND = 1e-5


def build_driver(tmp):
    """the link line of gen_train_v1_golden.build_driver"""
    exe = os.path.join(tmp, "train_rnn_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "train_rnn_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + REF_DIR, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread"])
    return exe


def reference_run(exe, tmp, tag, spec, seed, batches, verb="steps"):
    work = os.path.join(tmp, "%s_%d" % (tag, seed))
    os.makedirs(work, exist_ok=True)
    cfg, wts, _ = R.materialize(work, tag, seed, spec)
    for k, (x, y) in enumerate(batches, 1):
        x.astype(np.float32).tofile(os.path.join(work, "x_%d.bin" % k))
        y.astype(np.float32).tofile(os.path.join(work, "y_%d.bin" % k))
    subprocess.check_call([exe, verb, cfg, wts, work, str(len(batches)), work], stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)

    def get(stem):
        p = os.path.join(work, stem + ".bin")
        return np.fromfile(p, dtype=np.float32) if os.path.exists(p) else None
    return get


class Miss(Exception):
    pass


def fixture(exe, tmp, name):
    """The first seed that keeps both: the kink margin and the rule bound.  The reference's own rounding error grows through a
    batch-norm backward over few rows (K: five, and with the LAST step's statistics the backward is no projection), so a seed
    can miss 1e-5 by noise alone; such a seed is reported and passed over, never written."""
    for attempt in range(6000):
        seed = SEED0[name] + 97 * attempt
        t, _, _ = R.rule_snapshots(R.NETS[name], seed)
        if t.min_preact < T.KINK:
            continue
        try:
            return fixture_of(exe, tmp, name, seed, t)
        except Miss as m:
            print("  %s: seed %d rejected: %s" % (name, seed, m))
    sys.exit("%s: no seed keeps every pre-activation %g away from zero and the fp32 rule within %g of the reference" % (name, T.KINK, RULE_BOUND))


def check(ok, text):
    if not ok:
        raise Miss(text)


def fixture_of(exe, tmp, name, seed, t):
    spec = R.NETS[name]
    _, snaps, losses = R.rule_snapshots(spec, seed, np.float32)          # the form held against the reference
    get = reference_run(exe, tmp, name, spec, seed, [R.inputs(spec, seed, k) for k in range(1, R.STEPS + 1)])
    fix = {"seed": np.int64(seed), "min_preact": np.float64(t.min_preact)}
    worst = 0.0
    for k in range(1, R.STEPS + 1):
        loss = get("s%d_loss" % k)
        fix["s%d_loss" % k] = loss
        e = abs(float(loss[0]) - losses[k - 1]) / abs(losses[k - 1])
        check(e <= RULE_BOUND, "the rule's loss differs from the reference in step %d: %.3g" % (k, e))
        for i in range(len(spec["layers"])):
            for a, want in snaps[k - 1][i].items():
                if not R.kept(k, a):
                    continue
                got = get("s%d_l%d_%s" % (k, i, a))
                assert got is not None and got.size == want.size, "%s: step %d layer %d has no %s" % (name, k, i, a)
                e = T.err(got, want.reshape(-1))
                check(e <= RULE_BOUND, "the fp32 rule differs from the reference in step %d layer %d %s: %.3g" % (k, i, a, e))
                worst = max(worst, e)
                fix["s%d_l%d_%s" % (k, i, a)] = got.copy()
    fix["predict"] = get("predict")
    print("%s: seed %d, |pre-activation| >= %.3g, fp32 rule vs reference <= %.3g" % (name, seed, t.min_preact, worst))
    return fix


def long_fixture(exe, tmp):
    get = reference_run(exe, tmp, "long", R.LONG, R.LONG_SEED, R.long_inputs(), "losses")
    ref, t64 = get("losses").astype(np.float64), R.long_losses()
    dev = float(np.abs(ref - t64).max() / np.abs(t64).max())
    assert ref.size == R.LONG_STEPS and dev <= RULE_BOUND, "long: the reference's loss curve is %.3g off the rule's" % dev
    assert t64[-1] < 0.97 * t64[0], "long: the loss does not fall (%.4g -> %.4g)" % (t64[0], t64[-1])
    print("long: loss %.5g -> %.5g, reference vs float64 rule %.3g" % (t64[0], t64[-1], dev))
    return {"losses": ref.astype(np.float32), "deviation": np.float64(dev)}


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in sys.argv[1:] or sorted(R.NETS):
            out = os.path.join(ROOT, "tests", "golden", "train_rnn_%s.npz" % name)
            write_npz(out, fixture(exe, tmp, name))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))
        if not sys.argv[1:]:
            out = os.path.join(ROOT, "tests", "golden", "train_rnn_long.npz")
            write_npz(out, long_fixture(exe, tmp))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
