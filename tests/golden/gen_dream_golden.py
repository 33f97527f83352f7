#!/usr/bin/env python3
"""Reference-run fixtures for dreaming: tests/golden/dream_D1.npz, dream_D2.npz, dream_D3.npz.

The network half of every stored step comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by
oracle/build_ref.sh where the reference checkout exists) through tests/native/dream_ref.c, compiled here together with the
reference's nightmare.c from where it lies, so calculate_loss is the reference's own: resize_network, forward_network, the
delta copy, calculate_loss and backward_network with a zeroed state.delta, on the network input tests/dream_rule.py builds
in float32 from the picture the stored seed gives.  image.c has no compiled form, so the picture half (crop, resize, flip,
normalize, axpy, constrain) is the float32 rule applied to the reference's image gradient.

  s<k>_l<i>_output, s<k>_l<i>_delta, s<k>_grad      setting k of dream_rule.SETTINGS[name], every layer up to its max_layer
  c<k>_...                                          step k of dream_rule.CHAIN[name], each from the picture the step before left
  c<k>_picture                                      that picture ([c][h][w], the float32 rule on the reference's gradient)
  seed, s<k>_pseed, c_pseed                         the seed of the weights, and of each setting's (the chain's) picture

The generator runs the float64 rule first and ASSERTS, at every step it stores, that no leaky / relu pre-activation is
closer to 0 than 1e-4, that no maxpool window's two largest values differ by less than 1e-4 and that no element of the last
layer is closer than 1e-4 * max|output| to calculate_loss's threshold; it searches each setting's picture for that.  (Two
values that are EQUAL are not a kink: crop_image repeats edge pixels, the convolution windows inside such a band are identical
in every form, and the exact tie of a maxpool window over them goes to the first element in scan order in every form.)  On the reference's
own dump it asserts the same threshold margin, the same selected set and the same signs as the float64 run, and that the
rule in float32 and in float64 reproduces every stored array within 1e-5 relative.  It exits non-zero rather than write a
fixture that breaks any of these.

    python tests/golden/gen_dream_golden.py
    python tests/golden/gen_dream_golden.py --driver-only     # only leave the compiled driver as oracle/_ref/dream_ref, for
                                                              # the reference timing of tools/nightmare_latency.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import dream_rule as R  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

SEED0 = {"D1": 7103, "D2": 8209, "D3": 9311}
RULE_BOUND = 1e-5
F = np.float32


def build_dream_ref(tmp, rpath=None):
    """the reference's nightmare.c as a shared object of its own beside the driver -- the image.c symbols its run_nightmare
    and optimize_picture name stay unresolved there, as they do in libdarknet_ref.so, and nothing here calls those two --
    then the link line of oracle/build_ref.sh:36-38"""
    exe = os.path.join(tmp, "dream_ref")
    src = reference_sources()
    flags = ["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-iquote", src]
    subprocess.check_call(flags + ["-fPIC", "-shared", os.path.join(src, "nightmare.c"), "-o", os.path.join(tmp, "libnightmare_ref.so")])
    subprocess.check_call(flags + [os.path.join(ROOT, "tests", "native", "dream_ref.c"), "-o", exe, "-L" + tmp, "-lnightmare_ref",
                                   "-L" + REF_DIR, "-ldarknet_ref", "-Wl,-rpath," + (rpath or tmp + ":" + REF_DIR),
                                   "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread"])
    return exe


def reference_step(exe, work, cfg, wts, name, x, setting, tag):
    max_layer, _, _, _, _, thresh, _ = setting
    out = os.path.join(work, tag)
    os.makedirs(out, exist_ok=True)
    inp = os.path.join(out, "input.bin")
    np.ascontiguousarray(x, dtype=F).tofile(inp)
    c, h, w = x.shape
    subprocess.check_call([exe, "step", cfg, wts, str(max_layer), str(w), str(h), repr(float(thresh)), inp, out],
                          stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
    return lambda stem: np.fromfile(os.path.join(out, stem + ".bin"), dtype=F)


def checked_step(exe, work, cfg, wts, name, nets, pics, setting, tag, fix):
    """one step of all three: float64 rule, float32 rule, compiled reference (from the float32 picture).  Returns the pictures
    (float64, float32 = the rule on the reference's gradient) after it, or None when the float64 run breaks a margin."""
    net64, net32 = nets
    pic64, pic32 = pics
    spec = R.NETS[name]
    max_layer, octave, dx, dy, flip, thresh, norm = setting
    net64.min_preact = net64.min_gap = net64.min_margin = np.inf
    r64 = R.step(net64, pic64, setting)
    if min(net64.min_preact, net64.min_gap, net64.min_margin) < R.KINK:
        print("  %s %s: rejected: |pre-activation| %.2e, maxpool gap %.2e, threshold margin %.2e" %
              (name, tag, net64.min_preact, net64.min_gap, net64.min_margin))
        return None
    x32 = R.picture_to_input(pic32, R.scale_of(octave), dx, dy, flip, F)
    r32 = R.step(net32, pic32, setting)
    assert np.array_equal(r32["input"], x32)
    get = reference_step(exe, work, cfg, wts, name, x32, setting, tag)
    worst = 0.0
    for i in range(max_layer + 1):
        for a in ("output", "delta"):
            key = "l%d_%s" % (i, a)
            got = get(key)
            want = r64[key]
            assert got.size == want.size, "%s %s: %s has %d values, the rule %d" % (name, tag, key, got.size, want.size)
            for r, form in ((r64, "float64"), (r32, "float32")):
                e = R.err(got, r[key].reshape(-1))
                assert e <= RULE_BOUND, "%s %s: the %s rule differs from the reference in %s: %.3g" % (name, tag, form, key, e)
                worst = max(worst, e)
            if a == "output" and spec["layers"][i][0] == "conv" and spec["layers"][i][5] in ("leaky", "relu"):
                assert np.array_equal(got > 0, want.reshape(-1) > 0), "%s %s: %s: the reference's signs differ" % (name, tag, key)
            fix["%s_%s" % (tag, key)] = got.copy()
    last = get("l%d_output" % max_layer)
    kept, selected, _, _, margin = R.calculate_loss(last, thresh, F)
    kept64 = R.calculate_loss(r64["l%d_output" % max_layer], thresh, np.float64)[0]
    assert margin >= R.KINK, "%s %s: the reference has an element %.2e from the threshold" % (name, tag, margin)
    assert selected == r64["selected"] and np.array_equal(kept != 0, kept64.reshape(-1) != 0), \
        "%s %s: the reference selects %d, the float64 rule %d, or other elements" % (name, tag, selected, r64["selected"])
    grad = get("grad").reshape(x32.shape)
    for r, form in ((r64, "float64"), (r32, "float32")):
        e = R.err(grad, r["gradient"])
        assert e <= RULE_BOUND, "%s %s: the %s rule differs from the reference in the image gradient: %.3g" % (name, tag, form, e)
        worst = max(worst, e)
    fix[tag + "_grad"] = grad.copy()
    c, h, w = pic32.shape
    after32 = R.apply_update(pic32, R.gradient_to_update(grad, w, h, dx, dy, flip, F), R.RATE, norm, F)
    fix["_worst"] = max(fix.get("_worst", 0.0), worst)
    return r64["picture"], after32


def margins_ok(net64, pic32, settings):
    """the float64 forward passes of a chain of settings from one picture (a lone setting is a chain of one)"""
    net64.min_preact = net64.min_gap = net64.min_margin = np.inf
    pic = pic32.astype(np.float64)
    for n, setting in enumerate(settings):
        if n + 1 < len(settings):
            pic = R.step(net64, pic, setting)["picture"]
        else:
            max_layer, octave, dx, dy, flip, thresh, _ = setting
            net64.forward(R.picture_to_input(pic, R.scale_of(octave), dx, dy, flip, np.float64), max_layer, thresh)
        if min(net64.min_preact, net64.min_gap, net64.min_margin) < R.KINK:
            return False
    return True


def picture_seed(net64, name, seed, k, settings):
    """the weights have the fixture's seed; every setting (and the chain) searches a picture of its own, since one picture
    that keeps thousands of values clear of every kink in a dozen settings at once does not turn up"""
    for attempt in range(20000):
        pseed = seed * 1000 + k * 100003 + attempt
        if margins_ok(net64, R.picture(name, pseed), settings):
            return pseed
    sys.exit("%s setting %d: no picture keeps every kink %g away" % (name, k, R.KINK))


def fixture(exe, tmp, name):
    spec = R.NETS[name]
    seed = SEED0[name]
    work = os.path.join(tmp, "%s_%d" % (name, seed))
    os.makedirs(work, exist_ok=True)
    cfg, wts, params = R.materialize(work, name, seed)
    nets = (R.Net(spec, params, np.float64), R.Net(spec, params, F))
    fix = {"seed": np.int64(seed)}
    for k, setting in enumerate(R.SETTINGS[name]):
        pseed = picture_seed(nets[0], name, seed, k, [setting])
        fix["s%d_pseed" % k] = np.int64(pseed)
        pic32 = R.picture(name, pseed)
        assert checked_step(exe, work, cfg, wts, name, nets, (pic32.astype(np.float64), pic32), setting, "s%d" % k, fix) is not None
    chain = R.CHAIN.get(name, [])
    if chain:
        pseed = picture_seed(nets[0], name, seed, len(R.SETTINGS[name]), chain)
        fix["c_pseed"] = np.int64(pseed)
        pic32 = R.picture(name, pseed)
        pics = (pic32.astype(np.float64), pic32)
        for k, setting in enumerate(chain):
            pics = checked_step(exe, work, cfg, wts, name, nets, pics, setting, "c%d" % k, fix)
            assert pics is not None
            fix["c%d_picture" % k] = pics[1].copy()
    print("%s: seed %d, %d exact maxpool ties on repeated edge pixels, rule vs reference <= %.3g" %
          (name, seed, nets[0].exact_ties, fix.pop("_worst")))
    return fix


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    if "--driver-only" in sys.argv:
        print("built " + build_dream_ref(REF_DIR, "$ORIGIN"))
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_dream_ref(tmp)
        for name in sorted(R.NETS):
            out = os.path.join(ROOT, "tests", "golden", "dream_%s.npz" % name)
            write_npz(out, fixture(exe, tmp, name))
            print("wrote %s (%d KB)" % (out, os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
