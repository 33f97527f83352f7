#!/usr/bin/env python3
"""Reference-run fixture of the tracker's one piece with a compiled reference, fHOG: tests/golden/kcf_fhog.npz.

piotr_fhog/gradientMex.cpp of the reference checkout is compiled as it stands into a temporary directory (g++ -O2 -msse2,
with empty SDKDDKVer.h / tchar.h for its stdafx.h) and called as FHoG::extract(patch, 2, 4, 9) calls it (fhog.hpp:22-97):
I/255 column by column, gradMag with full = true, fhog with binSize 4, nOrients 9, softBin -1, clip 0.2; the first 31 of
the 32 channels are kept, row by row.  Stored: the 8-bit patches and those outputs, nothing else.

The orientation bins are hard, and the reference reads its angle from a 10000-entry arc-cosine table behind 12-bit
reciprocals, which moves it by up to 0.07 bin away from the boundaries.  A pixel that changes bin between two correct
implementations would need a tolerance that hides real errors, so every patch is edited by 1-2 grey levels at single
pixels until, under the float64 rule (tests/kcf_rule.py), no pixel with a non-zero gradient lies within MARGIN = 0.02 bin
of a boundary.  The generator ASSERTS that, that the compiled reference then picks the float64 bin at every such pixel,
and that the float64 rule reproduces the reference's features within RULE_BOUND (measured, printed, stored as
`rule_bound`); it exits non-zero rather than write a fixture that breaks any of them.

    python tests/golden/gen_kcf_golden.py
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kcf_rule as K  # noqa: E402
from tests.golden.gen_hier_golden import reference_sources, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kcf_fhog.npz")
PATCHES = {"48x64": (48, 64, 7001), "50x37": (50, 37, 7002), "21x26": (21, 26, 7003), "8x8": (8, 8, 7004)}
MARGIN = 0.02
# how far the reference's fp32 features (SSE reciprocals in gradMag, its own summation order) may lie from the float64
# rule, as max|ref - T64| / max|T64|: the generator measures it and refuses a fixture beyond this
RULE_BOUND = 1e-3


def build_reference(tmp):
    src = os.path.join(reference_sources(), "piotr_fhog")
    for name in ("SDKDDKVer.h", "tchar.h"):
        open(os.path.join(tmp, name), "w").close()
    so = os.path.join(tmp, "libfhog_ref.so")
    subprocess.check_call(["g++", "-O2", "-msse2", "-w", "-I", tmp, "-I", src, "-shared", "-fPIC",
                           os.path.join(src, "gradientMex.cpp"), "-o", so])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    grad_mag = getattr(lib, re.search(r"\b(_Z7gradMag\w+)", syms).group(1))
    grad_mag.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_bool]
    grad_mag.restype = None
    fhog = getattr(lib, re.search(r"\b(_Z4fhog\w+)", syms).group(1))
    fhog.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    fhog.restype = None
    return grad_mag, fhog


def reference_fhog(fns, patch):
    """-> (features [31][hb][wb], the reference's own hard bin per pixel [h][w])"""
    grad_mag, fhog = fns
    h, w = patch.shape
    fp = C.POINTER(C.c_float)
    img = (patch.astype(np.float32) / np.float32(255)).T.copy()              # column by column: I[x*h + y]
    M, O = np.zeros((w, h), np.float32), np.zeros((w, h), np.float32)
    grad_mag(img.ctypes.data_as(fp), M.ctypes.data_as(fp), O.ctypes.data_as(fp), h, w, 1, True)
    hb, wb = h // K.CELL, w // K.CELL
    H = np.zeros((3 * K.NORIENT + 5, wb, hb), np.float32)
    fhog(M.ctypes.data_as(fp), O.ctypes.data_as(fp), H.ctypes.data_as(fp), h, w, K.CELL, K.NORIENT, -1, np.float32(K.CLIP))
    o = O.T * np.float32(2 * K.NORIENT / (2 * np.float32(3.14159265)))
    bins = (o + np.float32(0.5)).astype(np.int64)
    bins[bins >= 2 * K.NORIENT] = 0
    return H[:K.CHANNELS].transpose(0, 2, 1).copy(), bins


def offenders(patch):
    M, O = K.grad_mag(patch.astype(np.float64), np.float64)
    _, dist = K.orient_bin(O)
    return (M > 0) & (dist < MARGIN)


def repair(patch, rng):
    """single-pixel edits of 1-2 grey levels until no pixel with a gradient lies within MARGIN of a bin boundary"""
    p = patch.astype(np.int64)
    h, w = p.shape
    edits = 0
    for _ in range(20000):
        bad = offenders(p)
        n = int(bad.sum())
        if n == 0:
            return p.astype(np.uint8), edits
        ys, xs = np.nonzero(bad)
        k = int(rng.integers(len(ys)))
        y, x = int(ys[k]), int(xs[k])
        best = None
        for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            yy, xx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
            for delta in (1, -1, 2, -2):
                v = p[yy, xx] + delta
                if v < 0 or v > 255:
                    continue
                q = p.copy()
                q[yy, xx] = v
                m = int(offenders(q).sum())
                if best is None or m < best[0]:
                    best = (m, yy, xx, v)
        if best is None:
            break
        _, yy, xx, v = best
        if best[0] >= n:                                     # no candidate helps: a random nudge out of the corner
            yy, xx = int(rng.integers(h)), int(rng.integers(w))
            v = min(max(p[yy, xx] + int(rng.choice((-1, 1))), 0), 255)
        p[yy, xx] = v
        edits += 1
    sys.exit("the repair did not converge")


def make_patch(h, w, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2)).astype(np.float64)
    img = np.kron(coarse, np.ones((4, 4)))[:h, :w] * 0.6 + rng.integers(0, 256, (h, w)) * 0.4
    return repair(np.clip(np.rint(img), 0, 255), rng)


def main():
    out = {}
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        fns = build_reference(tmp)
        for name, (h, w, seed) in PATCHES.items():
            patch, edits = make_patch(h, w, seed)
            assert not offenders(patch).any(), name
            ref, ref_bins = reference_fhog(fns, patch)
            M, O = K.grad_mag(patch.astype(np.float64), np.float64)
            bins, _ = K.orient_bin(O)
            mism = int(((bins != ref_bins) & (M > 0)).sum())
            t64 = K.fhog(patch.astype(np.float64), np.float64)
            e = K.err(ref, t64)
            worst = max(worst, e)
            print("%-6s edits %4d  bin mismatches %d  err(ref vs T64) %.3g  cells %d x %d" % (name, edits, mism, e, h // 4, w // 4))
            if mism:
                sys.exit("%s: the compiled reference picks another bin at %d pixels" % (name, mism))
            if not e <= RULE_BOUND:
                sys.exit("%s: the float64 rule is %g from the reference, beyond RULE_BOUND %g" % (name, e, RULE_BOUND))
            out["patch_" + name] = patch
            out["fhog_" + name] = ref
    out["rule_bound"] = np.float64(RULE_BOUND)
    out["measured"] = np.float64(worst)
    out["margin"] = np.float64(MARGIN)
    write_npz(OUT, out)
    print("wrote %s (%d bytes), worst err %.3g" % (OUT, os.path.getsize(OUT), worst))


if __name__ == "__main__":
    main()
