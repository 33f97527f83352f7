"""The detection loader's host half, without a device: the draws and the truth against tests/golden/aug_truth.npz (the
COMPILED reference's load_data_detection, run whole: tests/golden/gen_aug_golden.py), y2_net_augment against the cfg text,
every refusal of y2_train_load_detection / y2_train_step_loaded, the exports, and csrc/host/y2_aug.c as a stand-alone program
under -fsanitize=address,undefined over windows that hang over every edge."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_det_rule as D
from tests import train_rule as T
from tests.helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fix():
    f = load_golden("aug_truth")
    f["offsets"] = np.concatenate([[0], np.cumsum(f["label_count"])])
    return f


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def replay(fix, k):
    """srand(seed), the batch's paths, then image by image the draws: what the reference's single thread does"""
    hue, sat, exp = (float(v) for v in fix["distortion"])
    darknet.srand(int(fix["seeds"][k]))
    n = len(fix["c%d_path" % k])
    paths = darknet.aug_random_paths(n, len(fix["sizes"]))
    draws = []
    for p in paths:
        ow, oh = (int(v) for v in fix["sizes"][p])
        draws.append(darknet.aug_draw_detection(ow, oh, float(fix["jitter"][k]), hue, sat, exp, int(fix["label_count"][p])))
    return paths, draws


def test_fixture_holds_the_cases_it_is_about(fix):
    assert set(fix["jitter"].tolist()) == {float(np.float32(.2)), float(np.float32(.3))}
    assert {tuple(s) for s in fix["sizes"].tolist()} == {(37, 53), (64, 48), (500, 375)}
    assert set(fix["label_count"].tolist()) == {0, 1, 7, 35}
    flips, sentinel, holes = set(), 0, 0
    for k in range(len(fix["seeds"])):
        flips |= set(fix["c%d_flip" % k].tolist())
        t = fix["c%d_truth" % k].reshape(-1, 30, 5)
        sentinel += int((t[:, :, 0] == 999999).sum())
        for rows in t:
            zero = np.flatnonzero(rows[:, 0] == 0)
            holes += int(len(zero) > 0 and (rows[zero[0]:, 0] != 0).any())
    assert flips == {0, 1} and sentinel > 0 and holes > 0


@pytest.mark.parametrize("k", range(3))
def test_draws_follow_the_reference_rand_order(fix, k):
    paths, draws = replay(fix, k)
    assert np.array_equal(paths, fix["c%d_path" % k])
    for i, (p, d) in enumerate(zip(paths, draws)):
        assert [d["pleft"], d["ptop"], d["swidth"], d["sheight"]] == fix["c%d_window" % k][i].tolist(), (k, i)
        assert d["flip"] == fix["c%d_flip" % k][i], (k, i)
        assert np.array_equal(bits([d["dhue"], d["dsat"], d["dexp"]]), bits(fix["c%d_distort" % k][i])), (k, i)
        assert np.array_equal(d["swaps"], fix["c%d_swaps" % k][i][:fix["label_count"][p]]), (k, i)


@pytest.mark.parametrize("k", range(3))
def test_truth_is_the_reference_bit_for_bit(fix, k):
    off = fix["offsets"]
    for i, p in enumerate(fix["c%d_path" % k]):
        ow, oh = (int(v) for v in fix["sizes"][p])
        win = fix["c%d_window" % k][i]
        item = dict(frame=np.zeros((oh, ow, 3), np.uint8), pleft=int(win[0]), ptop=int(win[1]), swidth=int(win[2]), sheight=int(win[3]),
                    flip=int(fix["c%d_flip" % k][i]), boxes=fix["label_rows"][off[p]:off[p + 1]],
                    swaps=fix["c%d_swaps" % k][i][:fix["label_count"][p]])
        got = darknet.aug_truth_detection(item)
        assert np.array_equal(bits(got), bits(fix["c%d_truth" % k][i])), (k, i)


def test_a_skipped_box_keeps_its_slot():
    """fill_truth_detection's quirk: the zero row stays in the list, in front of the boxes behind it"""
    boxes = np.array([[3, .5, .5, .25, .25], [1, 1 / 256., .5, 1 / 128., .25], [2, .25, .75, .125, .125]], np.float32)
    t = darknet.aug_truth_detection(dict(frame=np.zeros((20, 20, 3), np.uint8), boxes=boxes)).reshape(30, 5)
    assert t[0].tolist() == [.5, .5, .25, .25, 3]
    assert not t[1].any()
    assert t[2].tolist() == [.25, .75, .125, .125, 2] and not t[3:].any()


def test_random_dim_is_the_multi_scale_draw():
    libc_rand = darknet.C.CDLL(None).rand
    darknet.srand(5)
    want = [(libc_rand() % 10 + 10) * 32 for _ in range(8)]
    darknet.srand(5)
    assert [darknet.aug_random_dim() for _ in range(8)] == want
    assert all(320 <= d <= 608 for d in want)


@pytest.mark.parametrize("name, want", [("tiny-yolo-voc.cfg", dict(jitter=.2, hue=.1, saturation=1.5, exposure=1.5, random=1)),
                                        ("yolo.cfg", dict(jitter=.3, hue=.1, saturation=1.5, exposure=1.5, random=1))])
def test_net_augment_reports_the_cfg(name, want):
    path = os.path.join(GOLDEN, "ref_cfg", name)
    text = open(path).read()
    for key, v in want.items():                         # the expectation is what the cfg text says
        assert "\n%s=%s" % (key, ("%g" % v).lstrip("0") if isinstance(v, float) else v) in text.replace(" ", ""), (name, key)
    net = darknet.Network.parse_network_cfg(path)
    got = net.net_augment()
    net.free()
    assert got["random"] == want["random"]
    for key in ("jitter", "hue", "saturation", "exposure"):
        assert np.float32(got[key]) == np.float32(want[key]), (name, key, got)


def test_net_augment_defaults_and_refusal(tmp_path):
    cfg, _, _ = D.materialize(str(tmp_path), "E", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    assert net.net_augment() == dict(jitter=np.float32(.2), hue=0., saturation=1., exposure=1., random=0)
    net.free()
    cfg, _, _ = T.materialize(str(tmp_path), "A", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    with pytest.raises(darknet.Y2Error, match=r"must end in \[region\]"):
        net.net_augment()
    net.free()


def good_items(batch, h=9, w=7):
    return [dict(frame=np.full((h, w, 3), 40 + i, np.uint8), boxes=np.array([[1, .5, .5, .25, .25]], np.float32)) for i in range(batch)]


REFUSALS = {
    "too_few_items": (lambda it: it[:-1], r"2 items for a batch-3 network"),
    "too_many_items": (lambda it: it + it[:1], r"4 items for a batch-3 network"),
    "two_channels": (lambda it: it[:1] + [dict(it[1], frame=np.zeros((9, 7, 2), np.uint8))] + it[2:], r"item 1: the frame has 2 channels"),
    "no_width": (lambda it: it[:2] + [dict(it[2], swidth=0)], r"item 2: the window is 0 x 9"),
    "no_height": (lambda it: [dict(it[0], sheight=-4)] + it[1:], r"item 0: the window is 7 x -4"),
    "swap_outside": (lambda it: it[:1] + [dict(it[1], swaps=np.array([1], np.int32))] + it[2:], r"item 1: swap 0 is 1, outside its 1 label rows"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_load_refuses_before_the_device(tmp_path, what):
    """without a device a refusal that came after a device call would carry HIP's message instead; with one, preparing the
    trainer would have waited for its uploads (the wait counter stands still)"""
    cfg, _, _ = D.materialize(str(tmp_path), "E", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    change, pattern = REFUSALS[what]
    waits = darknet.stream_syncs()
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_load_detection(change(good_items(net.net.batch)))
    with pytest.raises(darknet.Y2Error, match=r"nothing is loaded"):
        net.train_step_loaded()
    with pytest.raises(darknet.Y2Error, match=r"nothing is loaded"):
        net.train_pull_input()
    assert darknet.stream_syncs() == waits
    net.free()


def raw_item(**kw):
    """an AugItem built field by field, for what darknet.aug_items cannot express"""
    frame = np.zeros((9, 7, 3), np.uint8)
    boxes = np.array([[1, .5, .5, .25, .25]], np.float32)
    f = dict(data=frame.ctypes.data, h=9, w=7, c=3, step=21, pleft=0, ptop=0, swidth=7, sheight=9, flip=0, dhue=0., dsat=1., dexp=1.,
             boxes=boxes.ctypes.data, nboxes=1, swaps=None)
    f.update(kw)
    return darknet.AugItem(**f), (frame, boxes)


@pytest.mark.parametrize("kw, pattern", [(dict(data=None), r"item 1: data is NULL"), (dict(step=20), r"item 1: step 20 is less than w\*c = 21"),
                                         (dict(nboxes=-1), r"item 1: nboxes is -1"), (dict(boxes=None, nboxes=2), r"item 1: 2 label rows and boxes is NULL"),
                                         (dict(h=0), r"item 1: bad frame geometry")])
def test_load_refuses_a_bad_item_by_number(tmp_path, kw, pattern):
    cfg, _, _ = D.materialize(str(tmp_path), "E", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    arr = (darknet.AugItem * 3)()
    keep = []
    for i in range(3):
        arr[i], k = raw_item(**(kw if i == 1 else {}))
        keep.append(k)
    assert darknet.lib().y2_train_load_detection(darknet.C.byref(net.net), arr, 3, 0) == -1
    import re
    assert re.search(pattern, darknet._check())
    net.free()


NOT_A_DETECTOR = {
    "classifier": (lambda tmp: T.materialize(tmp, "A", 1)[0], None, r"must end in \[region\]"),
    "one_channel": (None, "[net]\nbatch=2\nwidth=6\nheight=6\nchannels=1\n[convolutional]\nfilters=12\nsize=1\nstride=1\npad=1\nactivation=linear\n"
                          "[region]\nanchors=1,1,2,2\nclasses=1\ncoords=4\nnum=2\nsoftmax=1\n", r"reads 1 channels"),
    "trainer_refuses": (None, "[net]\nbatch=2\nwidth=12\nheight=12\nchannels=3\n[convolutional]\nfilters=12\nsize=3\nstride=2\npad=1\nactivation=linear\n"
                              "[region]\nanchors=1,1,2,2\nclasses=1\ncoords=4\nnum=2\nsoftmax=1\n", r"layer 0 \(convolutional\).*stride 2"),
}


@pytest.mark.parametrize("what", sorted(NOT_A_DETECTOR))
def test_load_refuses_a_network_it_cannot_feed(tmp_path, what):
    make, text, pattern = NOT_A_DETECTOR[what]
    if make:
        cfg = make(str(tmp_path))
    else:
        cfg = str(tmp_path / "n.cfg")
        with open(cfg, "w") as f:
            f.write(text)
    net = darknet.Network.parse_network_cfg(cfg)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_load_detection(good_items(net.net.batch))
    net.free()


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"y2h_augment_to_input", "y2_aug_draw_detection", "y2_aug_random_paths", "y2_aug_random_dim", "y2_aug_truth_detection",
            "y2_net_augment", "y2_train_load_detection", "y2_train_step_loaded", "y2_train_pull_input", "y2_train_load_times"}
    assert want <= have, sorted(want - have)


def test_host_half_stand_alone_under_sanitizers(tmp_path):
    """csrc/host/y2_aug.c + tests/native/aug_host_main.c as one program with its own main, nothing preloaded: the packer over
    windows that hang over every edge of exactly-sized heap frames, the truth and the draws"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "aug_host")
    src = os.path.join(ROOT, "sr_object_detection_amd", "csrc", "host")
    # the sanitizers' runtimes are linked into the program itself, so they come first whatever else a host loads
    build = subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + src,
                            os.path.join(src, "y2_aug.c"), os.path.join(ROOT, "tests", "native", "aug_host_main.c"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler cannot link the sanitizers here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "aug_host ok" in run.stdout, run.stdout + run.stderr
