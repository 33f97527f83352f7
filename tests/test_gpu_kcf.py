"""The batched KCF tracker on the device (y2_kcf_*, y2_kcf.hip) against the numpy rule tests/kcf_rule.py.

Bound: err(A) = max|A - T64| / max|T64| with T64 the rule in float64; a device tensor passes when
err(gpu) <= 4 * err(reference) + 4 * 2^-23.  For fHOG the reference is the compiled reference's golden
(tests/golden/kcf_fhog.npz); for every later stage it is the rule in float32 (scipy.fft in single precision).  Both errors
are printed before anything is asserted.  The patch is pure selection plus exact fp32 operations and is compared with
array_equal; boxes are compared for equality."""
import functools

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import kcf_rule as K
from tests import kcf_scenes as S
from tests.helpers import load_golden, materialize

pytestmark = pytest.mark.gpu

BOXES3 = [(40.0, 40.0, 24.0, 28.0), (90.0, 60.0, 30.5, 20.2), (64.0, 48.0, 104.0, 100.0)]     # the third is halved


@pytest.fixture(scope="module")
def net(workdir):
    cfg, wts, x = materialize(workdir, "mini-mfma", 64, 2, 7)
    n = darknet.Network.parse_network_cfg(cfg)
    n.load_weights(wts)
    n._x = x
    yield n
    n.free()


def under_bound(name, gpu, t64, ref):
    eg, er = K.err(gpu, t64), K.err(ref, t64)
    print("%-28s err(gpu) %.3e  err(reference) %.3e  bound %.3e" % (name, eg, er, K.bound(er)))
    return eg <= K.bound(er)


@functools.lru_cache(maxsize=None)
def rule_init(dt, frame_key, box):
    return K.Tracker(dt).init(FRAMES[frame_key](), box)


FRAMES = {"scene": lambda: S.scene(60, 50), "scene3": lambda: S.scene(60, 50, seed=23, ow=40, oh=36), "texture": S.texture}


def fresh(dt, frame_key, box):
    """a tracker the test may move: a copy of the cached initialised one"""
    import copy
    return copy.deepcopy(rule_init(dt, frame_key, box))


# ------------------------------------------------------------------ 1. patch
def _patch_boxes():
    boxes = []
    for bw, bh in ((6.0, 5.0), (5.3, 6.8)):                                   # windows 24 x 20 (even) and 21 x 27 (odd)
        for cx, cy in ((26, 20), (2.7, 20), (26, 1.2), (50, 20), (26, 39), (1, 1), (51, 39.9), (-40, -40), (200, 20), (26, 52.0)):
            boxes.append((cx, cy, bw, bh))
    for cx, cy in ((26, 20), (0, 0), (51.5, 10), (-300, 20)):                   # halved: the window covers the frame and more
        boxes.append((cx, cy, 120.0, 100.0))
    boxes.append((30.5, 21.5, 101.0, 100.0))
    return boxes


@pytest.mark.parametrize("c,padded", [(1, False), (3, False), (4, False), (3, True)])
def test_patch_equals_the_rule(net, c, padded):
    rng = np.random.default_rng(40 + c)
    store = rng.integers(0, 256, (40, 60, c), dtype=np.uint8)
    frame = store[:, :52] if padded else np.ascontiguousarray(store[:, :52])
    if c == 1:
        frame = frame[:, :, 0]
    boxes = _patch_boxes()
    net.kcf_init(frame, boxes)
    g32 = K.grey(frame)
    half = K.halve(g32, np.float32)
    kinds = set()
    for i, b in enumerate(boxes):
        p = K.plan(b)
        want = K.get_subwindow(half if p["resized"] else g32, p["cx"], p["cy"], p["win_w"], p["win_h"])
        got = net.kcf_fetch(i, darknet.KCF_PATCH)
        assert got.shape == want.shape and np.array_equal(got, want), (i, b)
        kinds.add((p["resized"], bool(want.any())))
    assert kinds == {(0, True), (0, False), (1, True), (1, False)}         # inside / outside, halved or not: all met
    assert np.array_equal(half, K.halve(g32.astype(np.float64), np.float64))   # the halving is exact in fp32
    net.kcf_free()


# ------------------------------------------------------------------ 2. fHOG
@pytest.mark.parametrize("name", ["48x64", "50x37", "21x26", "8x8"])
def test_fhog_on_the_golden_patches(net, name):
    g = load_golden("kcf_fhog")
    patch, ref = g["patch_" + name], g["fhog_" + name]
    h, w = patch.shape
    net.kcf_init(patch, [(w // 2, h // 2, w / 4.0, h / 4.0)])                   # the window is the whole patch
    assert np.array_equal(net.kcf_fetch(0, darknet.KCF_PATCH), patch.astype(np.float32))
    got = net.kcf_fetch(0, darknet.KCF_FEATURES)
    t64 = K.fhog(patch.astype(np.float64), np.float64)
    ok = under_bound("fhog " + name, got, t64, ref)
    t32 = K.fhog(patch.astype(np.float32), np.float32)
    print("%-28s err(rule fp32) %.3e, err(gpu vs rule fp32) %.3e" % ("", K.err(t32, t64), K.err(got, t32.astype(np.float64))))
    assert got.shape == ref.shape and ok
    net.kcf_free()


# ------------------------------------------------------------------ 3. DFT
@pytest.mark.parametrize("rows,cols", [(2, 2), (3, 5), (7, 31), (32, 32), (33, 31), (65, 12), (12, 65)])
def test_dft_alone(net, rows, cols):
    rng = np.random.default_rng(rows * 100 + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    t64 = np.fft.fft2(x.astype(np.float64))
    ok_f = under_bound("dft %dx%d forward" % (rows, cols), net.kcf_dft(x), K.planes(t64), K.planes(K.fft2(x, np.float32)))
    z = (rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols))).astype(np.complex64)
    i64 = np.fft.ifft2(z.astype(np.complex128)).real
    ok_i = under_bound("dft %dx%d inverse" % (rows, cols), net.kcf_dft(K.planes(z), inverse=True), i64, K.ifft2_real(z, np.float32))
    assert ok_f and ok_i


# ------------------------------------------------------------------ 4. init
def test_init_of_three_trackers_in_one_call(net):
    frame = FRAMES["scene3"]()
    net.kcf_init(frame, BOXES3)
    assert net.kcf_count() == 3
    batched, ok = [], True
    for i, b in enumerate(BOXES3):
        t64, t32 = rule_init(np.float64, "scene3", b), rule_init(np.float32, "scene3", b)
        xf, af = net.kcf_fetch(i, darknet.KCF_XF), net.kcf_fetch(i, darknet.KCF_ALPHAF)
        assert np.array_equal(net.kcf_fetch(i, darknet.KCF_PATCH), t32.patch.astype(np.float32))
        ok &= under_bound("init %d features" % i, net.kcf_fetch(i, darknet.KCF_FEATURES), t64.feat, t32.feat)
        ok &= under_bound("init %d xf" % i, xf, K.planes(t64.model_xf), K.planes(t32.model_xf))
        ok &= under_bound("init %d alphaf" % i, af, K.planes(t64.model_alphaf), K.planes(t32.model_alphaf))
        batched.append((xf, af))
    assert [K.plan(b)["resized"] for b in BOXES3] == [0, 0, 1]
    for i, b in enumerate(BOXES3):                                           # trackers do not see each other
        net.kcf_init(frame, [b])
        assert np.array_equal(net.kcf_fetch(0, darknet.KCF_XF), batched[i][0])
        assert np.array_equal(net.kcf_fetch(0, darknet.KCF_ALPHAF), batched[i][1])
    assert ok
    net.kcf_free()


# ------------------------------------------------------------------ 5. track, update = 0
def _decisive(t64, t32):
    """the T64 peak exceeds the runner-up by at least ten times the float32 rule's own error on the response"""
    e32 = float(np.max(np.abs(t32.response.astype(np.float64) - t64.response)))
    m = S.peak_margin(t64.response)
    print("peak margin %.3e, 10 x |T32 - T64| %.3e" % (m, 10 * e32))
    return m >= 10 * e32


def test_track_without_update(net):
    f1 = S.scene(68, 38)                                                     # the object moved by (+8, -12)
    net.kcf_init(FRAMES["scene"](), [S.BOX])
    before = (net.kcf_fetch(0, darknet.KCF_XF), net.kcf_fetch(0, darknet.KCF_ALPHAF))
    t64, t32 = fresh(np.float64, "scene", S.BOX), fresh(np.float32, "scene", S.BOX)
    want, wpeak = t64.track(f1, update=False)
    t32.track(f1, update=False)
    assert _decisive(t64, t32)
    boxes, peaks = net.kcf_track(f1, update=False)
    assert tuple(boxes[0]) == want == (68.0, 38.0, 24.0, 28.0)
    assert (boxes[0][0] - S.BOX[0], boxes[0][1] - S.BOX[1]) == (8.0, -12.0)
    resp = net.kcf_fetch(0, darknet.KCF_RESPONSE)
    ok = under_bound("response", resp, t64.response, t32.response)
    assert peaks[0] == resp.max() and abs(peaks[0] - wpeak) <= K.bound(K.err(t32.response, t64.response)) * abs(wpeak)
    assert np.array_equal(net.kcf_fetch(0, darknet.KCF_XF), before[0]) and np.array_equal(net.kcf_fetch(0, darknet.KCF_ALPHAF), before[1])
    again, _ = net.kcf_track(f1, update=False)                               # the stored pose did not move either
    assert np.array_equal(again, boxes) and ok
    net.kcf_free()


# ------------------------------------------------------------------ 6. track, update = 1
def test_track_with_update(net):
    f1, f2 = S.scene(68, 38), S.scene(72, 46)
    net.kcf_init(FRAMES["scene"](), [S.BOX, BOXES3[2]])                      # the halved tracker rides along
    t64 = [fresh(np.float64, "scene", b) for b in (S.BOX, BOXES3[2])]
    t32 = [fresh(np.float32, "scene", b) for b in (S.BOX, BOXES3[2])]
    ok = True
    for step, f in enumerate((f1, f2)):
        want = [t.track(f, update=True)[0] for t in t64]
        for t in t32:
            t.track(f, update=True)
        assert _decisive(t64[0], t32[0])
        boxes, _ = net.kcf_track(f, update=True)
        assert tuple(boxes[0]) == want[0] == ((68.0, 38.0, 24.0, 28.0), (72.0, 46.0, 24.0, 28.0))[step]
        if _decisive(t64[1], t32[1]):
            assert tuple(boxes[1]) == want[1]
        for i in range(2):
            ok &= under_bound("step %d tracker %d response" % (step, i), net.kcf_fetch(i, darknet.KCF_RESPONSE), t64[i].response, t32[i].response)
            ok &= under_bound("step %d tracker %d xf" % (step, i), net.kcf_fetch(i, darknet.KCF_XF), K.planes(t64[i].model_xf), K.planes(t32[i].model_xf))
            ok &= under_bound("step %d tracker %d alphaf" % (step, i), net.kcf_fetch(i, darknet.KCF_ALPHAF), K.planes(t64[i].model_alphaf),
                              K.planes(t32[i].model_alphaf))
    assert ok
    net.kcf_free()


# ------------------------------------------------------------------ 7. across the wrap
def test_track_across_the_wrap(net):
    """The texture rolled down by 64 rows: 16 of the window's 28 cell rows, more than half.  The rule's answer is a wrapped
    (negative) cell; the device gives the rule's box, whatever a correct track would be."""
    box = (64.0, 48.0, 24.0, 28.0)
    f0 = S.texture()
    f1 = np.roll(f0, 64, axis=0)
    t64, t32 = fresh(np.float64, "texture", box), fresh(np.float32, "texture", box)
    want, _ = t64.track(f1, update=False)
    t32.track(f1, update=False)
    assert _decisive(t64, t32) and t64.max_loc[1] < 0
    net.kcf_init(f0, [box])
    boxes, _ = net.kcf_track(f1, update=False)
    assert tuple(boxes[0]) == want
    assert under_bound("wrap response", net.kcf_fetch(0, darknet.KCF_RESPONSE), t64.response, t32.response)
    net.kcf_free()


# ------------------------------------------------------------------ 8. twice the same bytes
def _session(net):
    out = []
    net.kcf_init(FRAMES["scene3"](), BOXES3)
    for f, upd in ((S.scene(68, 38, seed=23, ow=40, oh=36), False), (S.scene(64, 54, seed=23, ow=40, oh=36), True),
                   (S.scene(70, 50, seed=23, ow=40, oh=36), True)):
        boxes, peaks = net.kcf_track(f, update=upd)
        out += [boxes.tobytes(), peaks.tobytes()]
        for i in range(3):
            out += [net.kcf_fetch(i, w).tobytes() for w in (darknet.KCF_PATCH, darknet.KCF_FEATURES, darknet.KCF_XF, darknet.KCF_ALPHAF,
                                                           darknet.KCF_RESPONSE)]
    net.kcf_free()
    return out


def test_a_session_run_twice_gives_the_same_bytes(net):
    assert _session(net) == _session(net)


# ------------------------------------------------------------------ 9. the application's two calls
def test_init_objects_and_track_objects(net):
    f0, f1 = FRAMES["scene"](), S.scene(68, 38)
    objs = (darknet.Object * 2)()
    for k, (cx, cy, w, h) in enumerate((S.BOX, (96.0, 30.0, 20.0, 24.0))):
        o = objs[k]
        o.x, o.y, o.w, o.h = cx / S.W, cy / S.H, w / S.W, h / S.H
        o.name, o.prob, o.objClass = b"cup%d" % k, 0.5 + 0.25 * k, 3 + k
        o.CameraX, o.CameraY, o.CameraZ, o.CameraWidth, o.CameraHeight = 0.1 + k, 0.2, 1.5, 0.07, 0.09
        o.flagBelong2Person, o.bodyId = 1, 4 + k
        o.boxRGB[0], o.boxRGB[1], o.boxRGB[2] = 1.0, 2.0, 3.0
    f32 = np.float32
    pix = [(float(f32(o.x) * f32(S.W)), float(f32(o.y) * f32(S.H)), float(f32(o.w) * f32(S.W)), float(f32(o.h) * f32(S.H))) for o in objs]
    net.kcf_init_objects(f0, objs)
    out = (darknet.Object * 4)()
    n = net.kcf_track_objects(f1, out)
    assert n == net.kcf_count() == 2
    for k in range(2):
        t64, t32 = K.Tracker(np.float64).init(f0, pix[k]), K.Tracker(np.float32).init(f0, pix[k])
        (cx, cy, w, h), _ = t64.track(f1, update=False)
        t32.track(f1, update=False)
        o, src = out[k], objs[k]
        if _decisive(t64, t32):
            assert (o.x, o.y, o.w, o.h) == (f32(cx / S.W), f32(cy / S.H), f32(w / S.W), f32(h / S.H))
        assert (o.name, o.prob, o.objClass, o.CameraX, o.CameraY, o.CameraZ, o.CameraWidth, o.CameraHeight, o.flagBelong2Person,
                o.bodyId, tuple(o.boxRGB)) == (src.name, src.prob, src.objClass, src.CameraX, src.CameraY, src.CameraZ, src.CameraWidth,
                                               src.CameraHeight, src.flagBelong2Person, src.bodyId, tuple(src.boxRGB))
    assert (out[0].x, out[0].y) == (f32(68.0 / S.W), f32(38.0 / S.H))
    net.kcf_free()


# ------------------------------------------------------------------ 10. the engine is left as it was found
def test_detect_is_untouched_by_a_tracker_session(net):
    before, cb = net.detect(net._x, 0.3, 0.4)
    _session(net)
    after, ca = net.detect(net._x, 0.3, 0.4)
    assert np.array_equal(cb, ca) and len(before) == len(after)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_track_refuses_another_frame_size(net):
    net.kcf_init(FRAMES["scene"](), [S.BOX])
    with pytest.raises(darknet.Y2Error, match="initialised on"):
        net.kcf_track(np.zeros((S.H, S.W + 2, 3), np.uint8))
    with pytest.raises(darknet.Y2Error, match="initialised on"):
        net.kcf_track(np.zeros((S.H, S.W), np.uint8))
    net.kcf_free()
    assert net.kcf_count() == 0
