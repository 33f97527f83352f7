#!/usr/bin/env python3
"""Reference-run fixture for the detection loader's draws and truth: tests/golden/aug_truth.npz.

Everything stored under c<k>_* comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by
oracle/build_ref.sh where the reference checkout exists) through tests/native/aug_ref.c, compiled here into a temporary
directory with the link line of gen_train_det_golden.py plus -rdynamic and -ldl: the shared object binds the driver's
recording stubs for the image.c symbols (and its logging rand), so the reference's load_data_detection runs WHOLE --
get_random_paths, the window arithmetic, read_boxes, randomize_boxes, correct_boxes, fill_truth_detection are its compiled
code.  Per case: srand(seed), one load_data_detection of n images over the label files written here; per image the chosen
path, the crop window, the flip, dhue / dsat / dexp, the randomize_boxes indices and the 150 truth floats.

The label values are multiples of 1/1024 written with ten decimals, so the text the reference parses and the float32 stored
here are the same numbers.

The generator ASSERTS that the cases the tests are about occur: jitter .2 and .3; frames 37x53, 64x48 and 500x375; images
with 0, 1, 7 and 35 label rows (35 > 30); a row with x == y == 0 (-> 999999); a box the crop cuts below .01, leaving a hole in
the list in front of a kept box; a box clipped on each of the four sides; both flip values.  It also asserts, from a float64
recomputation of correct_boxes, that no corrected w or h lies within 1e-5 of .01, and exits non-zero rather than write a
fixture that breaks any of it.

    python tests/golden/gen_aug_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "aug_truth.npz")
NET_W, NET_H = 416, 416
HUE, SATURATION, EXPOSURE = .1, 1.5, 1.5
N = 16
CASES = ((4001, .2), (4002, .3), (4003, .2))                 # (seed, jitter)
SIZES = ((37, 53), (64, 48), (500, 375), (500, 375), (64, 48), (500, 375))     # (ow, oh) per path
ROWS = (0, 1, 7, 35, 7, 1)                                   # label rows per path
MAX_SWAPS = 35
FORBIDDEN = ("images", "JPEGImages", "raw", ".jpg", ".png", ".JPG", ".JPEG", "labels")   # find_replace would rewrite the directory


def label_rows(seed):
    """per path float32 [rows][5] = id x y w h, every value k/1024"""
    rng = np.random.RandomState(seed)
    out = []
    for p, n in enumerate(ROWS):
        rows = np.zeros((n, 5), np.float32)
        for i in range(n):
            w, h = rng.randint(60, 400, 2) / 1024.
            x, y = rng.randint(120, 904, 2) / 1024.
            rows[i] = (rng.randint(0, 20), x, y, w, h)
        if p == 2:                      # boxes that stick out of the frame on each side, and one the crop can cut away
            rows[0, 1:] = (40 / 1024., .5, 120 / 1024., .25)           # left
            rows[1, 1:] = (990 / 1024., .5, 120 / 1024., .25)          # right
            rows[2, 1:] = (.5, 36 / 1024., .25, 110 / 1024.)           # top
            rows[3, 1:] = (.5, 1000 / 1024., .25, 110 / 1024.)         # bottom
            rows[4, 1:] = (16 / 1024., .5, 30 / 1024., .25)            # 0 .. .03 of the width: cut by pleft > 15
        if p == 4:
            rows[3, 1:] = (0, 0, .25, .25)                             # x == y == 0
            rows[5, 1:] = (1010 / 1024., .5, 26 / 1024., .25)          # cut by pright
        out.append(rows)
    return out


def build_driver(tmp):
    exe = os.path.join(tmp, "aug_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-rdynamic", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "aug_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + REF_DIR, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread", "-ldl"])
    return exe


def write_tree(tmp, labels):
    """<tmp>/w/images/p<i>.jpg (named only) and <tmp>/w/labels/p<i>.txt -> the list file"""
    base = os.path.join(tmp, "w")
    assert not any(k in base for k in FORBIDDEN), "the temporary directory's name would be rewritten by find_replace: " + base
    os.makedirs(os.path.join(base, "labels"))
    lst = os.path.join(base, "paths.list")
    with open(lst, "w") as f:
        for i, ((ow, oh), rows) in enumerate(zip(SIZES, labels)):
            f.write("%s %d %d\n" % (os.path.join(base, "images", "p%d.jpg" % i), ow, oh))
            with open(os.path.join(base, "labels", "p%d.txt" % i), "w") as g:
                for r in rows:
                    g.write("%d %.10f %.10f %.10f %.10f\n" % (int(r[0]), r[1], r[2], r[3], r[4]))
    return lst


def bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint32).view(np.float32)


def run_case(exe, lst, tmp, seed, jitter):
    out = os.path.join(tmp, "case_%d.txt" % seed)
    subprocess.check_call([exe, lst, str(seed), str(N), str(NET_W), str(NET_H), repr(jitter), repr(HUE), repr(SATURATION),
                           repr(EXPOSURE), out])
    res = dict(path=[], window=[], flip=[], distort=[], swaps=[], truth=[])
    for line in open(out):
        head, tail = line.split("|")
        h = head.split()
        res["path"].append(int(h[0]))
        res["window"].append([int(v) for v in h[1:5]])
        res["flip"].append(int(h[5]))
        res["distort"].append(bits(h[6:9]))
        nd = int(h[9])
        rows = ROWS[int(h[0])]
        assert nd == rows, "path %d: %d draws behind random_distort_image for %d label rows" % (int(h[0]), nd, rows)
        sw = np.full(MAX_SWAPS, -1, np.int32)
        sw[:nd] = [int(v) % rows for v in h[10:10 + nd]]
        res["swaps"].append(sw)
        res["truth"].append(bits(tail.split()))
    return {k: np.array(v) for k, v in res.items()}


def corrected64(rows, swaps, size, window, flip):
    """randomize_boxes + correct_boxes in float64: per row (x, y, w, h, left_raw, right_raw, top_raw, bottom_raw), None for x == y == 0"""
    ow, oh = size
    pleft, ptop, sw, sh = window
    b = [list(map(float, r)) for r in rows]
    for i in range(len(b)):
        j = int(swaps[i])
        b[i], b[j] = b[j], b[i]
    sx, sy = sw / ow, sh / oh
    dx, dy = (pleft / ow) / sx, (ptop / oh) / sy
    out = []
    for _, x, y, w, h in b:
        if x == 0 and y == 0:
            out.append(None)
            continue
        l, r, t, bo = (x - w / 2) / sx - dx, (x + w / 2) / sx - dx, (y - h / 2) / sy - dy, (y + h / 2) / sy - dy
        if flip:
            l, r = 1 - r, 1 - l
        raw = (l, r, t, bo)
        l, r, t, bo = (min(max(v, 0.), 1.) for v in raw)
        out.append(((l + r) / 2, (t + bo) / 2, min(max(r - l, 0.), 1.), min(max(bo - t, 0.), 1.)) + raw)
    return out


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    labels = label_rows(977)
    fix = {"net": np.array([NET_W, NET_H], np.int32), "distortion": np.array([HUE, SATURATION, EXPOSURE], np.float32),
           "seeds": np.array([c[0] for c in CASES], np.int32), "jitter": np.array([c[1] for c in CASES], np.float32),
           "sizes": np.array(SIZES, np.int32), "label_count": np.array(ROWS, np.int32),
           "label_rows": np.concatenate(labels, axis=0).astype(np.float32)}
    seen = dict(flips=set(), paths=set(), sentinel=0, hole=0, left=0, right=0, top=0, bottom=0, over30=0)
    margin = np.inf
    with tempfile.TemporaryDirectory(prefix="augfix") as tmp:
        exe = build_driver(tmp)
        lst = write_tree(tmp, labels)
        for k, (seed, jitter) in enumerate(CASES):
            res = run_case(exe, lst, tmp, seed, jitter)
            for key, v in res.items():
                fix["c%d_%s" % (k, key)] = v
            for i in range(N):
                p = int(res["path"][i])
                truth = res["truth"][i].reshape(30, 5)
                seen["flips"].add(int(res["flip"][i]))
                seen["paths"].add(p)
                seen["sentinel"] += int((truth[:, 0] == 999999).any())
                seen["over30"] += int(ROWS[p] > 30)
                kept = truth[:, 0] != 0
                for j, c in enumerate(corrected64(labels[p], res["swaps"][i], SIZES[p], res["window"][i], res["flip"][i])[:30]):
                    if c is None:
                        continue
                    margin = min(margin, abs(c[2] - .01), abs(c[3] - .01))
                    if (c[2] < .01 or c[3] < .01):
                        assert not kept[j], "case %d image %d row %d: the rule skips a box the reference kept" % (k, i, j)
                        seen["hole"] += int(kept[j + 1:].any())
                        continue
                    assert kept[j]
                    seen["left"] += int(c[4] < 0)
                    seen["right"] += int(c[5] > 1)
                    seen["top"] += int(c[6] < 0)
                    seen["bottom"] += int(c[7] > 1)
    assert seen["flips"] == {0, 1}, "both flip values must occur"
    assert seen["paths"] == set(range(len(SIZES))), "every path must be chosen: %s" % sorted(seen["paths"])
    for key in ("sentinel", "hole", "left", "right", "top", "bottom", "over30"):
        assert seen[key] > 0, "the fixture has no case of: " + key
    assert margin > 1e-5, "a corrected w or h lies within %.3g of .01" % margin
    write_npz(OUT, fix)
    print("wrote %s (%d KB): %s, closest corrected size to .01: %.3g" % (OUT, os.path.getsize(OUT) // 1024,
                                                                         {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()}, margin))


if __name__ == "__main__":
    main()
