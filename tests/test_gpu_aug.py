"""The detection loader on the device: y2h_augment_to_input through the C-ABI against tests/aug_rule.py, by np.array_equal --
every value is formed by single IEEE operations in a fixed order, so a tolerance would only hide a reordering (the bar
tests/test_gpu_ingest.py sets) -- and the trainer entries end to end on the network of fixture E.

Provenance: the pixel chain is held to a restatement of the reference's image.c (tests/aug_rule.py: parity with a run of the
reference unpinned); the truth is pinned to the compiled reference by tests/test_aug_host.py."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import aug_rule as R
from tests import train_det_rule as D

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = ((13, 11), (32, 32), (36, 20))          # output (w, h): a width that is no multiple of four with rows of odd alignment; whole groups; more than one block
IDENTITY = dict(flip=0, dhue=0., dsat=1., dexp=1.)
PALETTE = np.array([(255, 0, 0), (255, 200, 0), (255, 255, 0), (100, 255, 0), (0, 255, 0), (0, 255, 120), (0, 255, 255), (0, 90, 255),
                    (0, 0, 255), (130, 0, 255), (255, 0, 255), (255, 0, 20), (200, 40, 90), (30, 60, 20), (10, 10, 200), (250, 251, 252)], np.uint8)


def frame(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


def padded(f, pad):
    """the same pixels as a view of a wider buffer: rows `pad` bytes apart more than they need"""
    h, w, c = f.shape
    buf = np.full((h, w * c + pad), 0xEE, np.uint8)
    buf[:, :w * c] = f.reshape(h, w * c)
    return np.lib.stride_tricks.as_strided(buf, shape=(h, w, c), strides=(buf.strides[0], c, 1))


def launch(items, w, h, swap_rb):
    """items: dicts of frame + draws -> float32 [n][h][w][3] of one y2h_augment_to_input launch; every frame goes up whole,
    with its own pitch"""
    L = darknet.lib()
    n = len(items)
    desc = (darknet.Aug * n)()
    blobs, off = [], 0
    for i, it in enumerate(items):
        f = it["frame"]
        oh, ow, c = f.shape
        pitch = f.strides[0]
        raw = np.full(pitch * oh, 0xEE, np.uint8)
        raw.reshape(oh, pitch)[:, :ow * c] = np.ascontiguousarray(f).reshape(oh, ow * c)
        with np.errstate(all="ignore"):
            ws, hs = F(it["swidth"] - 1) / F(w - 1), F(it["sheight"] - 1) / F(h - 1)
        desc[i] = darknet.Aug(off, pitch, c, 0, 0, ow, oh, ow, oh, it["pleft"], it["ptop"], it["swidth"], it["sheight"], it["flip"],
                              it["dhue"], it["dsat"], it["dexp"], ws, hs)
        blobs.append(raw)
        off += raw.size
    pixels = np.concatenate(blobs)
    table = np.frombuffer(bytes(desc), np.uint8)
    d_desc, d_pix, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    out = np.full((n, h, w, 3), np.nan, F)
    assert L.y2h_malloc(C.byref(d_desc), table.size) == 0 and L.y2h_malloc(C.byref(d_pix), pixels.size) == 0
    assert L.y2h_malloc(C.byref(d_out), out.nbytes) == 0
    try:
        assert L.y2h_memcpy_h2d(d_desc, table.ctypes.data, table.size, None) == 0
        assert L.y2h_memcpy_h2d(d_pix, pixels.ctypes.data, pixels.size, None) == 0
        assert L.y2h_memcpy_h2d(d_out, out.ctypes.data, out.nbytes, None) == 0
        assert L.y2h_augment_to_input(d_desc, n, d_pix, int(swap_rb), h, w, d_out, None) == 0
        assert L.y2h_memcpy_d2h(out.ctypes.data, d_out, out.nbytes, None) == 0
    finally:
        L.y2h_free(d_desc); L.y2h_free(d_pix); L.y2h_free(d_out)
    return out


def rule(it, w, h, swap_rb):
    return R.augment(it["frame"], it["pleft"], it["ptop"], it["swidth"], it["sheight"], it["flip"], it["dhue"], it["dsat"], it["dexp"], w, h, swap_rb)


def whole(f, **kw):
    return dict(dict(frame=f, pleft=0, ptop=0, swidth=f.shape[1], sheight=f.shape[0], **IDENTITY), **kw)


def geometry_items(w, h):
    """sources 7x5, 1x9, 9x1, 37x53 with a padded pitch, four bytes per pixel; windows over every edge, one column wide,
    the whole frame at the output's own size; both flips; the distortion's scales either way"""
    big = padded(frame(53, 37, 3, 3), 5)
    return [
        whole(frame(5, 7, 3, 1)),
        whole(frame(9, 1, 3, 2), flip=1, dhue=.1),                                   # im.w == 1
        whole(frame(1, 9, 3, 4), dsat=1.5),                                          # im.h == 1
        dict(frame=big, pleft=-5, ptop=-7, swidth=50, sheight=70, flip=1, dhue=-.1, dsat=1 / 1.5, dexp=1.5),     # over all four edges
        dict(frame=big, pleft=20, ptop=30, swidth=30, sheight=40, flip=0, dhue=.1, dsat=1.5, dexp=1 / 1.5),      # past right and bottom
        dict(frame=big, pleft=-9, ptop=-4, swidth=20, sheight=21, flip=1, dhue=0., dsat=1.5, dexp=1.5),          # past left and top
        dict(frame=big, pleft=10, ptop=10, swidth=1, sheight=20, flip=0, dhue=.1, dsat=1., dexp=1.),             # swidth == 1
        dict(frame=big, pleft=-40, ptop=5, swidth=30, sheight=9, flip=0, dhue=0., dsat=1., dexp=1.),             # wholly left of the frame
        whole(frame(5, 7, 4, 5), flip=1, dexp=1.5),                                  # four bytes per pixel
        whole(frame(h, w, 3, 6)),                                                    # the output's own size, identity
        whole(frame(h, w, 4, 7), flip=1),
        whole(np.repeat(frame(h, w, 1, 8), 3, axis=2)),                              # the same, grey
        whole(np.repeat(frame(h, w, 1, 10), 4, axis=2), flip=1),
    ]


@pytest.mark.parametrize("swap_rb", (0, 1))
@pytest.mark.parametrize("w, h", SIZES)
def test_kernel_is_the_rule_on_every_geometry(w, h, swap_rb):
    """one launch of thirteen items of eight different sizes.

    Identity parameters at the output's own size give the plane value (float)(v / 255.) itself, bit for bit, exactly where the
    reference gives it: on grey pixels, whose saturation is 0, so that hsv_to_rgb hands v back.  A coloured pixel still goes
    through rgb_to_hsv and hsv_to_rgb (random_distort_image always calls distort_image), and v * (1 - delta / max) is not
    min in floating point: there the bar is the rule, as everywhere (on these frames the round trip lands up to 3e-7 from v / 255.; printed, not asserted)."""
    items = geometry_items(w, h)
    got = launch(items, w, h, swap_rb)
    for i, it in enumerate(items):
        assert np.array_equal(got[i], rule(it, w, h, swap_rb)), "item %d of %dx%d swap %d" % (i, w, h, swap_rb)
    assert np.array_equal(got[11], R.planes(items[11]["frame"], swap_rb))
    assert np.array_equal(got[12], R.planes(items[12]["frame"], swap_rb)[:, ::-1])
    for i in (9, 10):
        same = R.planes(items[i]["frame"], swap_rb)[:, ::-1 if items[i]["flip"] else 1]
        print("identity, coloured, %dx%d: max |out - v/255.| = %.3g" % (w, h, np.abs(got[i] - same).max()))


def colour_frame(w, h):
    """saturated colours around the whole hue circle, greys, black and white, one pixel each, then noise"""
    f = frame(h, w, 3, 9)
    flat = f.reshape(-1, 3)
    flat[:len(PALETTE)] = PALETTE
    greys = np.array([0, 255, 128, 1, 254, 77], np.uint8)
    flat[len(PALETTE):len(PALETTE) + len(greys)] = greys[:, None]
    return f


@pytest.mark.parametrize("w, h", SIZES)
def test_kernel_is_the_rule_on_every_colour_branch(w, h):
    f = colour_frame(w, h)
    grey = np.zeros((h, w, 3), np.uint8)
    grey[...] = (np.arange(h * w) % 256).astype(np.uint8).reshape(h, w, 1)      # delta 0 everywhere, max 0 where the byte is 0
    items = [whole(f, dhue=d, dsat=s, dexp=e) for d, s, e in ((.1, 1.5, 1 / 1.5), (-.1, 1 / 1.5, 1.5), (.5, 1.5, 1.5), (-.5, 1 / 1.5, 1 / 1.5))]
    items += [whole(grey, dhue=.5, dsat=1.5, dexp=1.5), whole(grey, flip=1, dhue=-.1, dsat=1 / 1.5, dexp=1 / 1.5)]
    # the frame is built to reach every branch: say so before the comparison means anything
    hh, s, v = R.rgb_to_hsv(R.planes(f))
    coloured = s > 0
    seen, up, down, clamped = set(), False, False, False
    for it in items[:4]:
        moved = (hh + F(it["dhue"])).astype(F)
        up |= bool((moved[coloured] > 1).any())
        down |= bool((moved[coloured] < 0).any())
        seen |= set(np.floor(6 * R.shift_hue(hh, it["dhue"])[coloured].astype(np.float64)).astype(int).tolist())
        clamped |= bool(((v * F(it["dexp"])) > 1).any())
    assert up and down and clamped and {0, 1, 2, 3, 4, 5} <= seen, (up, down, clamped, seen)
    got = launch(items, w, h, 0)
    for i, it in enumerate(items):
        assert np.array_equal(got[i], rule(it, w, h, 0)), "item %d of %dx%d" % (i, w, h)
    assert not np.isnan(got).any()                      # a grey pixel's 0/0 hue is carried and never read
    assert (got[:4] == 1).any() and (got[:4] == 0).any()


# ---- the trainer entries, end to end on the network of fixture E (12 x 10, batch 3) ----
BOXES = (np.array([[2, .30, .45, .35, .40], [0, .31, .47, .30, .42], [3, .78, .27, .30, .25]], F),
         np.zeros((0, 5), F),
         np.array([[1, .58, .71, .22, .30], [2, 0, 0, .2, .2], [0, .02, .5, .03, .4], [3, .5, .5, .3, .3]], F))
FRAMES = (frame(53, 37, 3, 21), frame(16, 20, 4, 22), padded(frame(10, 12, 3, 23), 3))


def batch_items(step):
    """three frames of three sizes with the draws the reference would make after srand(700 + step)"""
    darknet.srand(700 + step)
    items = []
    for f, boxes in zip(FRAMES, BOXES):
        d = darknet.aug_draw_detection(f.shape[1], f.shape[0], .3, .1, 1.5, 1.5, len(boxes))
        items.append(dict(d, frame=f, boxes=boxes))
    return items


def params(net):
    out = {}
    for i in range(net.net.n):
        if darknet.LAYER_TYPES[net.net.layers[i].type] != "CONVOLUTIONAL":
            continue
        names = ["weights", "biases", "weight_updates", "bias_updates"]
        if net.net.layers[i].batch_normalize:
            names += ["scales", "scale_updates", "rolling_mean", "rolling_variance"]
        for a in names:
            out[(i, a)] = net.train_pull(i, a).copy()
    return out


def test_loaded_steps_are_train_network_datum_on_the_pulled_batch(workdir):
    cfg, wts, _ = D.materialize(workdir, "E", 7103)
    a = darknet.Network.parse_network_cfg(cfg)
    b = darknet.Network.parse_network_cfg(cfg)
    a.load_weights(wts)
    b.load_weights(wts)
    w, h = a.net.w, a.net.h
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        a.train_step_loaded()
    for step in (1, 2, 3):
        items = batch_items(step)
        a.train_load_detection(items, swap_rb=bool(step == 2))
        x, y = a.train_pull_input()
        for i, it in enumerate(items):                  # the input is the rule's, the truth the host function's
            assert np.array_equal(x[i], rule(it, w, h, step == 2).transpose(2, 0, 1)), (step, i)
            assert np.array_equal(y[i].view(np.uint32), darknet.aug_truth_detection(it).view(np.uint32)), (step, i)
        la = a.train_step_loaded()
        lb = b.train_step(x, y)
        assert np.isfinite(la) and F(la).tobytes() == F(lb).tobytes(), (step, la, lb)
    pa, pb = params(a), params(b)
    assert pa.keys() == pb.keys() and len(pa) > 0
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    # multi-scale: a resize drops the trainer and the load with it
    a.train_load_detection(batch_items(4))
    a.resize_network(16, 14)
    with pytest.raises(darknet.Y2Error, match="nothing is loaded"):
        a.train_step_loaded()
    items = batch_items(5)
    a.train_load_detection(items)
    x, _ = a.train_pull_input()
    assert x.shape == (3, 3, 14, 16)
    for i, it in enumerate(items):
        assert np.array_equal(x[i], rule(it, 16, 14, False).transpose(2, 0, 1)), i
    assert np.isfinite(a.train_step_loaded())
    assert np.isfinite(a.train_step_loaded())           # a second step on the same load
    a.free()
    b.free()
