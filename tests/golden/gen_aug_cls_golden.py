#!/usr/bin/env python3
"""Reference-run fixture for the classifier loader's draws and label rows: tests/golden/aug_cls.npz.

Everything stored under c<k>_* comes out of the COMPILED REFERENCE (oracle/_ref/libdarknet_ref.so, built by
oracle/build_ref.sh where the reference checkout exists) through tests/native/aug_cls_ref.c, compiled here into a temporary
directory with the link line of gen_aug_golden.py: the shared object binds the driver's recording stubs for the image.c
symbols, so the reference's load_data_augment runs WHOLE -- get_random_paths, load_image_augment_paths' call order with the
flip draw between random_augment_image and random_distort_image, load_labels_paths with fill_truth and fill_hierarchy are
its compiled code, and the stubs draw through its compiled rand_scale / rand_int / rand_uniform / rand_uniform_strong.
What the stubs RESTATE (image.c has no compiled form): the order of the five draws of random_augment_image and the three of
random_distort_image, and the arithmetic between them.

Per case: srand(seed), one load_data_augment of n images; per image the chosen path, what rotate_crop_image would be handed
(aspect, scale, rad, dx, dy), the flip, dhue / dsat / dexp, and the truth row.  The fixture holds only these recorded
numbers, the path strings, the frame sizes, the label names and the tree's parent column.

The generator ASSERTS that the cases the tests are about occur: aspect .75 and 1; angle 0 and 7; saturation / exposure .75
(a bound below 1) and 1.5; frames 37x53, 64x48 and 500x375; both flip values; a dx clamped at 0 and a dx not clamped; a
path that matches exactly one label, one that matches none, one that matches two; a tree of 4 groups in which some group is
filled with SECRET_NUM and some set leaf has two ancestors.  It exits non-zero rather than write a fixture without them.

    python tests/golden/gen_aug_cls_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "aug_cls.npz")
N = 16
HUE = .1
#        seed  aspect angle saturation exposure min  max  size tree
CASES = ((5001, .75, 7., .75, .75, 224, 320, 224, 0),        # tiny.cfg's values
         (5002, 1., 0., 1.5, 1.5, 16, 32, 16, 1),
         (5003, .75, 7., 1.5, .75, 224, 448, 224, 1))
PATHS = (("set/tabby_a.jpg", 37, 53), ("set/plain_b.jpg", 64, 48), ("set/dog_bus_c.jpg", 500, 375),
         ("set/siamese_d.jpg", 500, 375), ("set/car_e.jpg", 64, 48), ("set/vehicle_f.jpg", 37, 53))
LABELS = ("animal", "vehicle", "cat", "dog", "car", "bus", "tabby", "siamese")
PARENT = (-1, -1, 0, 0, 1, 1, 2, 2)          # groups: {animal, vehicle} {cat, dog} {car, bus} {tabby, siamese}
SECRET_NUM = -1234


def build_driver(tmp):
    exe = os.path.join(tmp, "aug_cls_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-rdynamic", "-iquote", reference_sources(),
                           os.path.join(ROOT, "tests", "native", "aug_cls_ref.c"), "-o", exe, "-L" + REF_DIR, "-ldarknet_ref",
                           "-Wl,-rpath," + REF_DIR, "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-lm", "-lpthread", "-ldl"])
    return exe


def bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint32).view(np.float32)


def run_case(exe, tmp, files, case):
    seed, aspect, angle, sat, exp, lo, hi, size, tree = case
    out = os.path.join(tmp, "case_%d.txt" % seed)
    subprocess.check_call([exe, files["list"], files["labels"], files["tree"] if tree else "-", str(seed), str(N), str(lo), str(hi),
                           str(size), repr(angle), repr(aspect), repr(HUE), repr(sat), repr(exp), out], stdout=subprocess.DEVNULL)
    res = dict(path=[], crop=[], flip=[], distort=[], truth=[])
    for line in open(out):
        head, tail = line.split("|")
        h = head.split()
        res["path"].append(int(h[0]))
        res["crop"].append(bits(h[1:6]))
        res["flip"].append(int(h[6]))
        res["distort"].append(bits(h[7:10]))
        res["truth"].append(bits(tail.split()))
    return {k: np.array(v) for k, v in res.items()}


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    fix = {"cases": np.array([c[:5] for c in CASES], np.float32), "crop": np.array([c[5:] for c in CASES], np.int32),
           "hue": np.float32(HUE), "paths": np.array([p[0] for p in PATHS]), "sizes": np.array([p[1:] for p in PATHS], np.int32),
           "labels": np.array(LABELS), "parent": np.array(PARENT, np.int32)}
    seen = dict(flips=set(), paths=set(), matches=set(), dx_at_0=0, dx_free=0, below_one=0, above_one=0, secret=0, deep=0)
    with tempfile.TemporaryDirectory(prefix="augcls") as tmp:
        exe = build_driver(tmp)
        files = {k: os.path.join(tmp, k + ".txt") for k in ("list", "labels", "tree")}
        with open(files["list"], "w") as f:
            f.writelines("%s %d %d\n" % p for p in PATHS)
        with open(files["labels"], "w") as f:
            f.writelines(l + "\n" for l in LABELS)
        with open(files["tree"], "w") as f:
            f.writelines("%s %d\n" % lp for lp in zip(LABELS, PARENT))
        for k, case in enumerate(CASES):
            res = run_case(exe, tmp, files, case)
            for key, v in res.items():
                fix["c%d_%s" % (k, key)] = v
            seen["flips"] |= set(res["flip"].tolist())
            seen["paths"] |= set(res["path"].tolist())
            for p, (a, s, _, dx, _) in zip(res["path"], res["crop"].astype(np.float64)):
                room = (PATHS[p][1] * s / a - case[7]) / 2.          # the scaled frame's width beyond `size`, in float64
                assert abs(dx) <= max(room, 0) * (1 + 1e-6) + 1e-4, "dx %g outside its limit %g" % (dx, room)
                seen["dx_at_0"] += int(room < -1e-3 and dx == 0)
                seen["dx_free"] += int(room > 1e-3 and dx != 0)
            seen["below_one"] += int(case[3] < 1 and case[4] < 1)
            seen["above_one"] += int(case[3] > 1 and case[4] > 1)
            for p, t in zip(res["path"], res["truth"]):
                flat = [int(l in PATHS[p][0]) for l in LABELS]
                seen["matches"].add(min(sum(flat), 2))
                if case[8]:
                    seen["secret"] += int((t == SECRET_NUM).any())
                    seen["deep"] += int(any(flat[j] and PARENT[j] >= 0 and PARENT[PARENT[j]] >= 0 for j in range(len(LABELS))))
                else:
                    assert t.tolist() == flat, "a flat truth row is not the strstr row"
    assert {c[1] for c in CASES} == {.75, 1.} and {c[2] for c in CASES} == {0., 7.}, "aspect .75 and 1, angle 0 and 7"
    assert {tuple(s) for s in fix["sizes"].tolist()} == {(37, 53), (64, 48), (500, 375)}
    assert seen["flips"] == {0, 1}, "both flip values must occur"
    assert seen["paths"] == set(range(len(PATHS))), "every path must be chosen: %s" % sorted(seen["paths"])
    assert seen["matches"] == {0, 1, 2}, "paths matching no, one and two labels: %s" % sorted(seen["matches"])
    assert len(set(PARENT)) - 1 + 1 >= 3, "a tree of at least 3 groups"
    for key in ("dx_at_0", "dx_free", "below_one", "above_one", "secret", "deep"):
        assert seen[key] > 0, "the fixture has no case of: " + key
    write_npz(OUT, fix)
    print("wrote %s (%d KB): %s" % (OUT, os.path.getsize(OUT) // 1024, {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()}))


if __name__ == "__main__":
    main()
