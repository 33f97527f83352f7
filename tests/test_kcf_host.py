"""CPU-only checks of the KCF tracker (y2_kcf_*): the numpy rule tests/kcf_rule.py against the compiled reference's fHOG
(tests/golden/kcf_fhog.npz) and against itself, y2_kcf_plan against the rule, every refusal that needs no device before
any device work, the exports and the application-style caller.  The refusal of a frame whose size differs from the init
frame's needs initialised trackers, so it lives in tests/test_gpu_kcf.py."""
import ctypes as C
import math

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import kcf_rule as K
from tests import kcf_scenes as S
from tests.helpers import load_golden, materialize


@pytest.mark.parametrize("name", ["48x64", "50x37", "21x26", "8x8"])
def test_rule_reproduces_the_compiled_fhog(name):
    g = load_golden("kcf_fhog")
    patch, ref = g["patch_" + name], g["fhog_" + name]
    M, O = K.grad_mag(patch.astype(np.float64), np.float64)
    _, dist = K.orient_bin(O)
    assert not ((M > 0) & (dist < float(g["margin"]))).any()                # the fixture's condition on the patches
    t64 = K.fhog(patch.astype(np.float64), np.float64)
    e = K.err(ref, t64)
    print("%s: err(reference vs T64) %.3e, recorded bound %.3e" % (name, e, float(g["rule_bound"])))
    assert ref.shape == t64.shape == (31, patch.shape[0] // 4, patch.shape[1] // 4)
    assert e <= float(g["rule_bound"]) and float(g["measured"]) <= float(g["rule_bound"])
    assert K.err(K.fhog(patch.astype(np.float32), np.float32), t64) < 1e-5


PLAN_TABLE = [(50, 40, 100, 100), (50, 40, 100.01, 100), (50, 40, 200.02, 50), (3.5, 2.25, 24, 28), (64, 48, 30.5, 20.2), (10, 10, 33.33, 7.77),
              (0, 0, 2, 2), (-5.5, 7, 2.1, 2.9), (300, 300, 513.9, 513.9), (300, 300, 256.2, 2.0), (1e6, -1e6, 99.99, 100.01)]


@pytest.mark.parametrize("box", PLAN_TABLE)
def test_plan_matches_the_rule(box):
    assert darknet.kcf_plan(box) == K.plan(box)


def test_plan_halving_threshold_and_limits():
    assert darknet.kcf_plan((0, 0, 100, 100))["resized"] == 0 and darknet.kcf_plan((0, 0, 100, 100))["cells_w"] == 100
    assert darknet.kcf_plan((0, 0, 100.01, 100.0))["resized"] == 1
    assert darknet.kcf_plan((0, 0, 513.9, 513.9))["cells_w"] == 256        # floor(256.95 * 4) = 1027 px -> 256 cells
    assert darknet.kcf_plan((0, 0, 2.0, 64.24))["cells_h"] == 64
    for box, word in (((0, 0, 514.0, 514.0), "above"), ((0, 0, 5000, 2.0), "above"), ((0, 0, 1.99, 30), "below"), ((0, 0, 30, 1.9), "below"),
                      ((0, 0, 0.0, 5), "w <= 0"), ((0, 0, 5, -1.0), "h <= 0"), ((float("nan"), 0, 5, 5), "finite"),
                      ((0, 0, float("inf"), 5), "finite")):
        with pytest.raises(darknet.Y2Error, match=word):
            darknet.kcf_plan(box)


def test_refusals_come_before_any_device_work(workdir):
    cfg, _, _ = materialize(workdir, "mini", 32, 1, 5)
    net = darknet.Network.parse_network_cfg(cfg)
    L = darknet.lib()
    frame = np.zeros((40, 52, 3), np.uint8)
    ok = [(20.0, 20.0, 6.0, 6.0)]
    cases = [((frame, ok * 33), "Y2_KCF_MAX_TRACKERS"), ((frame, [(1, 1, 514.0, 514.0)]), "Y2_KCF_MAX_CELLS"),
             ((frame, [(1, 1, 0.4, 5)]), "below 2 x 2"), ((np.zeros((40, 52, 2), np.uint8), ok), "channels"),
             ((frame, [(1, 1, float("nan"), 5)]), "not finite"), ((frame, [(1, 1, 5, 0.0)]), "w <= 0 or h <= 0")]
    for args, word in cases:
        with pytest.raises(darknet.Y2Error, match=word):
            net.kcf_init(*args)
    box = darknet.KcfBox(20, 20, 6, 6)
    assert L.y2_kcf_init(net.net, None, 40, 52, 3, 156, C.byref(box), 1) != 0
    assert "NULL" in darknet._check()
    assert L.y2_kcf_init(net.net, frame.ctypes.data_as(C.c_void_p), 40, 52, 3, 155, C.byref(box), 1) != 0
    assert "step" in darknet._check()
    with pytest.raises(darknet.Y2Error, match="y2_kcf_init first"):
        net.kcf_track(frame)
    assert L.y2_kcf_track(net.net, None, 40, 52, 3, 156, 0, None, None) != 0
    assert "NULL" in darknet._check()
    out = np.zeros(4, np.float32)
    assert L.y2_kcf_fetch(net.net, 0, 0, darknet._ptr(out), 4) != 0
    assert "y2_kcf_init first" in darknet._check()
    objs = (darknet.Object * 1)()
    with pytest.raises(darknet.Y2Error, match="y2_kcf_init first"):
        net.kcf_track_objects(frame, objs)
    assert net.kcf_count() == 0
    net.kcf_free()                                                          # nothing to free: no fault, no message
    net.free()


def test_library_exports_the_tracker_and_the_caller_links(workdir):
    L = darknet.lib()
    for name in ("y2_kcf_plan", "y2_kcf_init", "y2_kcf_track", "y2_kcf_count", "y2_kcf_fetch", "y2_kcf_dft", "y2_kcf_free",
                 "y2_kcf_init_objects", "y2_kcf_track_objects", "y2h_kcf_patch", "y2h_kcf_fhog", "y2h_kcf_dft", "y2h_kcf_cross",
                 "y2h_kcf_gauss", "y2h_kcf_train", "y2h_kcf_apply", "y2h_kcf_argmax"):
        assert hasattr(L, name), name
    from tests.test_native_callers import build
    build(workdir, "kinect_kcf_like", "gcc", "kinect_kcf_like.c")


def test_struct_layouts_match_c(workdir):
    import os
    import subprocess
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src, exe = os.path.join(workdir, "kcf_layout.c"), os.path.join(workdir, "kcf_layout")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sr_yolo2.h"\nint main(void) {\n')
        for cname, cls in (("y2_kcf_box", darknet.KcfBox), ("y2_kcf_geometry", darknet.KcfGeometry)):
            f.write('    printf("%%zu\\n", sizeof(%s));\n' % cname)
            for name, _ in cls._fields_:
                f.write('    printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, name))
        f.write('    printf("%d %d\\n", Y2_KCF_MAX_TRACKERS, Y2_KCF_MAX_CELLS);\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", inc, src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    want = []
    for cls in (darknet.KcfBox, darknet.KcfGeometry):
        want += [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
    assert got == want + [darknet.KCF_MAX_TRACKERS, darknet.KCF_MAX_CELLS] == want + [K.MAX_TRACKERS, K.MAX_CELLS]


# ------------------------------------------------------------------ the rule's own checks
def test_labels_have_their_one_at_the_origin():
    for dim1, dim2 in ((24, 28), (25, 27), (2, 2), (7, 30)):
        lab = K.gaussian_labels(1.3, dim1, dim2)
        assert lab.shape == (dim2, dim1) and lab[0, 0] == 1.0 and lab.max() == 1.0
        assert np.argmax(lab) == 0
    assert np.array_equal(K.circshift(np.arange(12).reshape(3, 4), -1, 0), np.roll(np.arange(12).reshape(3, 4), -1, axis=1))


@pytest.mark.parametrize("dx,dy", [(2, -3), (-5, 4), (0, 0), (10, 0), (0, -9), (7, 6)])
def test_a_circular_shift_moves_the_peak_by_whole_cells(dx, dy):
    """A patch shifted circularly by (4*dx, 4*dy) px moves the response peak by (dx, dy) cells; (10, 0) and (0, -9) land
    beyond half of the 16 x 16 map and come back wrapped.  The window is flat here: the Hann window is what makes the
    tracker prefer the centre, and it is not invariant under the shift."""
    dt = np.float64
    rng = np.random.default_rng(77)
    patch = np.kron(rng.integers(0, 256, (16, 16)), np.ones((4, 4))) + rng.integers(0, 8, (64, 64))
    win = (np.ones(16, np.float32), np.ones(16, np.float32))
    yf = K.fft2(K.gaussian_labels(math.sqrt(16 * 16) * K.OUTPUT_SIGMA_FACTOR / K.CELL * 4, 16, 16), dt)
    xf = K.windowed_fft(K.fhog(patch, dt), win, dt)
    kf, _ = K.gaussian_correlation(xf, xf, dt, auto=True)
    alphaf = yf / (kf + K.LAMBDA)
    zf = K.windowed_fft(K.fhog(np.roll(patch, (4 * dy, 4 * dx), axis=(0, 1)), dt), win, dt)
    kzf, _ = K.gaussian_correlation(zf, xf, dt)
    resp = K.ifft2_real(alphaf * kzf, dt)
    my, mx = np.unravel_index(int(np.argmax(resp)), resp.shape)
    assert (mx, my) == (dx % 16, dy % 16)
    wrap = lambda v, n: v - n if v > n // 2 else v                          # noqa: E731
    want = lambda v: v if -8 < v <= 8 else (v - 16 if v > 0 else v + 16)    # noqa: E731
    assert (wrap(mx, 16), wrap(my, 16)) == (want(dx), want(dy))


def test_rule_tracker_follows_the_scene():
    t = K.Tracker(np.float64).init(S.scene(60, 50), S.BOX)
    box, peak = t.track(S.scene(68, 38), update=False)
    assert box == (68.0, 38.0, 24.0, 28.0) and t.max_loc == (2, -3) and (t.cx, t.cy) == (60.0, 50.0)
    box, _ = t.track(S.scene(68, 38), update=True)
    assert box == (68.0, 38.0, 24.0, 28.0) and (t.cx, t.cy) == (68.0, 38.0)
    assert t.track(S.scene(72, 46), update=True)[0] == (72.0, 46.0, 24.0, 28.0)
