"""CPU-only checks of the multi-view classifier evaluations (y2_classifier_view_sums and the three
y2_validate_classifier_*_frames): the library exports them and the two device functions, the Python mirror of y2h_view
has the C layout, every refusal happens before any device work (so it is seen here, without a GPU) and names what it
should, and the rule of tests/tta_rule.py pushed through the CPU oracle -- which is pinned to the reference --
reproduces the reference-run fixture tests/golden/tta_mini.npz bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import tta_rule as R
from tests.conftest import has_gpu
from tests.helpers import load_golden

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ENTRIES = ("y2_classifier_view_sums", "y2_validate_classifier_10_frames", "y2_validate_classifier_multi_frames",
           "y2_validate_classifier_full_frames")


def test_library_exports_the_view_entries():
    L = darknet.lib()
    for name in ENTRIES + ("y2h_views_to_input", "y2h_accumulate_rows", "y2_set_view_block_bytes", "y2_view_resizes"):
        assert hasattr(L, name), name
    for name in ("classifier_view_sums", "validate_classifier_10", "validate_classifier_multi", "validate_classifier_full"):
        assert hasattr(darknet.Network, name), name


def test_view_struct_layout_matches_c(workdir):
    src = os.path.join(workdir, "view_layout.c")
    exe = os.path.join(workdir, "view_layout")
    fields = [f for f, _ in darknet.View._fields_]
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "y2_hip.h"\n#include "sr_yolo2.h"\nint main(void) {\n')
        f.write('    printf("%zu\\n", sizeof(y2h_view));\n')
        for name in fields:
            f.write('    printf("%%zu\\n", offsetof(y2h_view, %s));\n' % name)
        f.write('    printf("%d %d %d\\n", Y2_VIEWS_CROP10, Y2_VIEWS_MULTI, Y2_VIEWS_FULL);\n')
        f.write("    return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", INCLUDE, src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[0] == C.sizeof(darknet.View)
    assert got[1:-3] == [getattr(darknet.View, name).offset for name in fields]
    assert got[-3:] == [darknet.VIEWS_CROP10, darknet.VIEWS_MULTI, darknet.VIEWS_FULL] == [R.CROP10, R.MULTI, R.FULL]


def _net(workdir, spec=None, tag="mini", batch=2):
    cfg, wts = R.write_mini(workdir, 5, batch=batch, spec=spec, tag=tag)
    return darknet.Network.parse_network_cfg(cfg)


FRAMES = [np.zeros((3, 40, 50), np.float32), np.zeros((4, 50, 40), np.float32), np.zeros((3, 64, 64), np.float32)]


def _sums_refused(net, mode, frames, scales=None, n=None, nscales=None, sums=True):
    arr, keep = darknet.images(frames)
    sc = np.ascontiguousarray(scales, dtype=np.int32) if scales is not None else None
    out = np.zeros((max(len(frames), 1), net.output_size), np.float32)
    rc = darknet.lib().y2_classifier_view_sums(C.byref(net.net), mode, arr if frames is not None else None,
                                               len(frames) if n is None else n, darknet._ptr(sc) if sc is not None else None,
                                               (sc.size if sc is not None else 0) if nscales is None else nscales,
                                               darknet._ptr(out) if sums else None)
    assert rc != 0
    return darknet._check()


@pytest.mark.parametrize("mode", [R.CROP10, R.MULTI, R.FULL])
def test_refusals_come_before_device_work_and_name_the_argument(workdir, mode):
    net = _net(workdir)
    size = (net.net.w, net.net.h, net.net.batch)
    assert "n = 0" in _sums_refused(net, mode, FRAMES, n=0)
    assert "n = -2" in _sums_refused(net, mode, FRAMES, n=-2)
    arr, keep = darknet.images(FRAMES)
    out = np.zeros((3, net.output_size), np.float32)
    fn = darknet.lib().y2_classifier_view_sums
    assert fn(C.byref(net.net), mode, None, 3, None, 0, darknet._ptr(out)) != 0
    assert "frames is NULL" in darknet._check()
    assert "sums is NULL" in _sums_refused(net, mode, FRAMES, sums=False)
    arr[1].data = None
    assert fn(C.byref(net.net), mode, arr, 3, None, 0, darknet._ptr(out)) != 0
    msg = darknet._check()
    assert "frame 1" in msg and "NULL" in msg, msg
    for bad, frag in (((3, 0, 50), "frame 2"), ((3, 40, 0), "frame 2")):
        arr, keep = darknet.images(FRAMES)
        arr[2].h, arr[2].w = bad[1], bad[2]
        assert fn(C.byref(net.net), mode, arr, 3, None, 0, darknet._ptr(out)) != 0
        msg = darknet._check()
        assert frag in msg and "size" in msg, msg
    msg = _sums_refused(net, mode, FRAMES[:1] + [np.zeros((2, 40, 50), np.float32)])
    assert "frame 1" in msg and "2 planes" in msg, msg
    assert "mode 7" in _sums_refused(net, 7, FRAMES)
    if mode == R.MULTI:
        assert "nscales = 0" in _sums_refused(net, mode, FRAMES, scales=[24, 32], nscales=0)
        assert "scales[1] = 0" in _sums_refused(net, mode, FRAMES, scales=[24, 0, 40])
        assert "scales[2] = -8" in _sums_refused(net, mode, FRAMES, scales=[24, 32, -8])
        msg = _sums_refused(net, mode, FRAMES, scales=[24, 1])               # a 1 x 1 image cannot pass two 2x2 pools
        assert "frame 0" in msg and "scale 1" in msg, msg
    # nothing was resized or re-batched by a refused call
    assert (net.net.w, net.net.h, net.net.batch) == size
    # a valid call is refused by nothing but the absence of a device
    if not has_gpu():
        msg = _sums_refused(net, mode, FRAMES, scales=[24, 32] if mode == R.MULTI else None)
        assert "frame" not in msg and "device" in msg.lower(), msg
    net.free()


def test_validate_refusals(workdir):
    net = _net(workdir)
    truth = [1, 2, 3]
    for call in (lambda **k: net.validate_classifier_10(FRAMES, **k), lambda **k: net.validate_classifier_multi(FRAMES, scales=[24], **k),
                 lambda **k: net.validate_classifier_full(FRAMES, **k)):
        with pytest.raises(darknet.Y2Error, match="classes = 11 against 10"):
            call(truth=truth, classes=11, topk=1)
        with pytest.raises(darknet.Y2Error, match="topk = 6 of 5"):
            call(truth=truth, classes=5, topk=6)
    with pytest.raises(darknet.Y2Error, match="frame 0"):
        net.validate_classifier_10([np.zeros((1, 8, 8), np.float32)], [0], 10, 3)
    with pytest.raises(darknet.Y2Error, match="y2_validate_classifier_multi_frames: scales"):
        net.validate_classifier_multi(FRAMES, truth, 10, 3, scales=[0])
    arr, keep = darknet.images(FRAMES)
    a, b = C.c_float(), C.c_float()
    assert darknet.lib().y2_validate_classifier_10_frames(net.net, arr, 3, None, 10, 3, C.byref(a), C.byref(b)) != 0
    assert "truth is NULL" in darknet._check()
    net.free()


def test_networks_the_modes_cannot_run_are_refused(workdir):
    # a dense head: resize_network refuses it, so MULTI and FULL do, naming the layer; CROP10 does not resize
    dense = _net(workdir, spec=R.DENSE_SPEC, tag="dense")
    for mode in (R.MULTI, R.FULL):
        msg = _sums_refused(dense, mode, FRAMES, scales=[24] if mode == R.MULTI else None)
        assert "layer 4" in msg and "[connected]" in msg and "resize" in msg, msg
    if not has_gpu():
        assert "layer" not in _sums_refused(dense, R.CROP10, FRAMES)
    dense.free()
    # a recurrent network
    cfg = os.path.join(workdir, "tta_rnn.cfg")
    with open(cfg, "w") as f:
        f.write(zoo.recurrent_cfg_text("rnn-mini", 2, 1))
    rnn = darknet.Network.parse_network_cfg(cfg)
    for mode in (R.CROP10, R.MULTI, R.FULL):
        assert "recurrent" in _sums_refused(rnn, mode, FRAMES)
    rnn.free()
    # a hierarchical classifier: worded like y2_validate_classifier_frames' refusal
    net = _net(workdir)
    tree = darknet.Tree()
    net.net.hierarchy = C.pointer(tree)
    for mode in (R.CROP10, R.MULTI, R.FULL):
        assert "hierarchical classifiers (softmax tree=) are not implemented on the device" in _sums_refused(net, mode, FRAMES)
    with pytest.raises(darknet.Y2Error, match="hierarchical classifiers"):
        net.validate_classifier_10(FRAMES, [0, 0, 0], 10, 3)
    net.net.hierarchy = None
    net.free()


def test_rule_helpers():
    assert R.resize_min_dims(50, 40, 24) == (30, 24) and R.resize_min_dims(40, 50, 24) == (24, 30)
    assert R.resize_min_dims(33, 47, 40) == (40, 56) and R.resize_min_dims(64, 64, 32) == (32, 32)
    im = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    assert R.flip_image(im)[1, 2].tolist() == im[1, 2, ::-1].tolist()
    got = R.crop_image(im, -1, 1, 4, 4)                                     # one column left of the image, one row below
    assert got[0].tolist() == [[4, 4, 5, 6], [8, 8, 9, 10], [8, 8, 9, 10], [8, 8, 9, 10]]
    assert R.view(im, 2, 0, 3, 1, 1)[0].tolist() == [[1, 0, 0]]
    acc = R.sequential_sum([np.float32(1), np.float32(2 ** -24), np.float32(2 ** -24)])
    assert acc == np.float32(1)                                             # rounded after every addition
    assert R.top_k(np.array([.1, .5, .5, .3], np.float32), 3).tolist() == [1, 2, 3]


@pytest.mark.parametrize("name,mode,scales", [("crop10", R.CROP10, None), ("multi", R.MULTI, R.MINI_SCALES), ("full", R.FULL, None)])
def test_rule_through_the_oracle_reproduces_the_reference_fixture(oracle, workdir, name, mode, scales):
    g = load_golden("tta_mini")
    frames = R.mini_frames(int(g["frame_seed"]))
    for i, f in enumerate(frames):
        assert f.tobytes() == g["frame_%d" % i].tobytes()
    seed = int(g["seed"])

    def predict(size, x):
        cfg, wts = R.write_mini(workdir, seed, size[0], size[1], len(x))
        on = oracle.OracleNet(cfg, wts)
        out = on.predict(x)
        on.close()
        return out

    views, per = R.mode_views(mode, frames, oracle.resize_image, scales)
    assert per == {R.CROP10: 10, R.MULTI: 2 * len(R.MINI_SCALES), R.FULL: 1}[mode]
    assert np.array([s for s, _ in views], np.int32).tobytes() == g[name + "_sizes"].tobytes()
    rows = R.rows_of(views, predict)
    assert rows.tobytes() == g[name + "_rows"].tobytes()
    sums = R.sums_of(rows, per)
    assert sums.tobytes() == g[name + "_sums"].tobytes()
    assert np.stack([R.top_k(s, 3) for s in sums]).tobytes() == g[name + "_top3"].tobytes()
    for s in sums:                                   # the margin the fixture promises
        top = np.sort(s.astype(np.float64))[::-1][:4]
        assert np.min(-np.diff(top)) >= 1e-3
    assert synth is not None
