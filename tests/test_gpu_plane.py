"""The table-plane removal of the Grasp branch on the device (y2_depth_set_plane_removal / y2_depth_plane /
y2_depth_grasp_aligned / y2_depth_set_event / y2_depth_set_grasp_filter) against tests/plane_rule.py: array_equal with the
restatement of include/y2_plane_rule.h (doubles included: the sums go through one fixed tree), an equal mask and
coefficients within 1e-6 against the independent solver.  1e-6 is three orders below the fixtures' 1 mm margin, so it
cannot move a pixel, and far above double rounding at these magnitudes."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import depth_rule
from tests import plane_rule as pr
from tests.test_gpu_regions import _mini

pytestmark = pytest.mark.gpu

# name: depth dh x dw, colour H x W, with a map, scene seed
SHAPES = {"64x48": (48, 64, 72, 96, True, 11),
          "67x53": (53, 67, 77, 101, True, 12),          # tails of the vector loads, the last workgroup partly full
          "128x106": (106, 128, 106, 128, False, 13),
          "512x424": (424, 512, 424, 512, False, 14),     # the tree across 212 workgroups
          "640x480": (480, 640, 480, 640, False, 15)}     # 300 chunks: two groups in the tree's last level
PLANE_KEYS = ("found", "best", "valid_points", "best_count", "removed", "a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def _case(name):
    """the inputs of a shape and what the restatement gives for them; computed once, never changed"""
    dh, dw, H, W, with_map, seed = SHAPES[name]
    depth, tab, label = pr.scene(dh, dw, seed)
    body = np.random.default_rng(seed + 100).choice(np.array([0, 1, 2, 3, 6, 7, 255], np.uint8), (dh, dw))
    m = pr.color_map(H, W, dh, dw, seed + 200) if with_map else None
    triples = pr.samples(depth, pr.FAR_M, pr.ITERS, pr.SEED)
    rec, grasp = pr.remove_plane(depth, tab, pr.FAR_M, pr.DIST_M, triples)
    planes = depth_rule.align(depth, body, m)
    g16 = pr.register(grasp, planes[3])
    for a in (depth, tab, label, body, triples, grasp, g16) + tuple(planes):
        a.setflags(write=False)
    return dict(depth=depth, tab=tab, label=label, body=body, map=m, triples=triples, rec=rec, grasp=grasp, planes=planes,
                g16=g16, dh=dh, dw=dw, H=H, W=W)


def _same(a, b):
    assert a.shape == b.shape
    for k in depth_rule.FIELDS:
        x, y = a[k], b[k]
        ok = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert ok, (k, x, y)


def _box(left, top, right, bot, w, h):
    l, r, t, b = (left + 0.25) / w, (right + 0.25) / w, (top + 0.25) / h, (bot + 0.25) / h
    return np.array([(l + r) / 2, (t + b) / 2, r - l, b - t], np.float32)


def _boxes(c):
    """a handful of boxes: an empty ROI, a ROI with no grasp depth (GetImgAvg's sumAll fallback), the full frame, a box
    over the first object, a box half off the frame"""
    H, W, g16, d16 = c["H"], c["W"], c["g16"], c["planes"][0]
    side = max(3, H // 16)
    bare = next(((x, y) for y in range(0, H - side, 2) for x in range(0, W - side, 2)
                 if not g16[y:y + side, x:x + side].any() and d16[y:y + side, x:x + side].any()), None)
    assert bare is not None, "the scene has a patch of bare table"
    ys, xs = np.nonzero(g16)
    oy, ox = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    return np.array([np.array([1.4, 0.5, 0.2, 0.2], np.float32),
                     _box(bare[0], bare[1], bare[0] + side, bare[1] + side, W, H),
                     _box(0, 0, W, H, W, H),
                     _box(max(0, ox - side), max(0, oy - side), min(W, ox + side), min(H, oy + side), W, H),
                     np.array([0.97, 0.2, 0.3, 0.35], np.float32)])


def _want_boxes(c, boxes, table):
    return depth_rule.as_records([pr.box_stats_grasp(b, *c["planes"], table, c["g16"]) for b in boxes], darknet.DET3D_DTYPE)


@pytest.fixture(scope="module")
def net3(workdir):
    net, _, _ = _mini(workdir, 3, tag="plane")
    yield net
    net.free()


@pytest.fixture()
def clean(net3):
    """every test leaves the engine as it found it: removal off, Demo_what, no grasp filter, no table"""
    yield net3
    net3.depth_set_event(darknet.EVENT_DEMO_WHAT)
    net3.depth_set_grasp_filter(False)
    net3.depth_set_plane_removal(iters=0)
    net3.depth_set_camera_table(None)


def _upload(net, c, **opts):
    net.depth_set_camera_table(c["tab"])
    net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, opts.pop("iters", pr.ITERS), pr.SEED, **opts)
    net.depth_upload(c["depth"], c["body"], c["map"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_plane_equals_the_restatement(clean, name):
    net, c = clean, _case(name)
    _upload(net, c)
    got = net.depth_plane()
    print(name, got)
    assert [got[k] for k in PLANE_KEYS] == [c["rec"][k] for k in PLANE_KEYS], (got, c["rec"])
    assert got["found"] == 1 and got["removed"] > 0.4 * c["dh"] * c["dw"]
    gd, g16 = net.depth_grasp_aligned((c["dh"], c["dw"]))
    assert np.array_equal(gd, c["grasp"]) and np.array_equal(g16, c["g16"])
    assert np.array_equal(net.depth_aligned()[0], c["planes"][0])            # the Demo_what planes are untouched
    # the Grasp statistics
    boxes = _boxes(c)
    want = _want_boxes(c, boxes, c["tab"])
    assert want["valid"].tolist() == [0, 1, 1, 1, 1] and want[1]["avg_mm"] == 0 and want[1]["mean_all_mm"] > 0
    assert (want["otsu"][1:] == 255).all() and want[3]["avg_mm"] > 0
    net.depth_set_event(darknet.EVENT_GRASP)
    _same(net.depth_boxes(boxes), want)
    # and the Demo_what branch on the same frame is what it was
    net.depth_set_event(darknet.EVENT_DEMO_WHAT)
    demo = depth_rule.as_records([depth_rule.box_stats(b, *c["planes"], c["tab"]) for b in boxes], darknet.DET3D_DTYPE)
    _same(net.depth_boxes(boxes), demo)
    assert not np.array_equal(demo["avg_mm"], want["avg_mm"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_plane_agrees_with_the_independent_solver(clean, name):
    net, c = clean, _case(name)
    found, coef, mask, dist = pr.solve_independent(c["depth"], c["tab"], pr.FAR_M, pr.DIST_M, c["triples"])
    valid = (c["label"] == pr.TABLE) | (c["label"] == pr.OBJECT)
    # the condition on the inputs (tests/test_plane_host.py checks it for the first three; the fourth is checked here)
    assert found == 1 and mask[c["label"] == pr.TABLE].all() and not mask[c["label"] == pr.OBJECT].any()
    assert np.abs(dist[valid] - pr.DIST_M).min() >= 1e-3
    _upload(net, c)
    got = net.depth_plane()
    gd, _ = net.depth_grasp_aligned((c["dh"], c["dw"]))
    clipped = pr.clip(c["depth"], pr.FAR_M)
    assert np.array_equal((gd == 0) & (clipped > 0), mask)
    assert np.array_equal(gd[~mask], clipped[~mask])
    err = np.abs(np.array([got[k] for k in "abcd"]) - coef).max()
    print(name, "max |coefficient - independent| = %.3g" % err)
    assert err < 1e-6


def _edge(net, depth, tab, iters=pr.ITERS, samples=None):
    net.depth_set_camera_table(tab)
    net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, iters, pr.SEED, samples=samples)
    net.depth_upload(depth, None, None)
    gd, g16 = net.depth_grasp_aligned(depth.shape)
    assert np.array_equal(gd, g16)                            # an identity frame: one plane
    return net.depth_plane(), gd


def test_frames_without_a_plane(clean):
    c = _case("64x48")
    dh, dw, tab = c["dh"], c["dw"], c["tab"]
    zero = np.zeros((dh, dw), np.uint16)
    beyond = np.full((dh, dw), 1001, np.uint16)
    two = zero.copy(); two[5, 7] = 700; two[30, 40] = 650
    for depth in (zero, beyond, two):
        got, gd = _edge(clean, depth, tab)
        rec, grasp = pr.remove_plane(depth, tab, pr.FAR_M, pr.DIST_M, pr.samples(depth, pr.FAR_M, pr.ITERS, pr.SEED))
        assert [got[k] for k in PLANE_KEYS] == [rec[k] for k in PLANE_KEYS]
        assert got["found"] == 0 and got["removed"] == 0 and got["valid_points"] == int((pr.clip(depth, pr.FAR_M) > 0).sum())
        assert np.array_equal(gd, pr.clip(depth, pr.FAR_M)) and np.array_equal(gd, grasp)
    # caller triples that are all void: no index, a repeat, a pixel without depth, a pixel beyond far_m, out of range
    depth = c["depth"]
    flat = depth.ravel()
    ok = np.flatnonzero((flat > 0) & (flat <= 1000))
    bad = [(-1, -1, -1), (ok[0], ok[1], ok[0]), (ok[0], ok[1], np.flatnonzero(flat == 0)[0]),
           (ok[0], np.flatnonzero(flat > 1000)[0], ok[2]), (ok[0], ok[1], dh * dw), (ok[3], ok[3], ok[3])]
    got, gd = _edge(clean, depth, tab, iters=len(bad), samples=bad)
    assert got["found"] == 0 and got["removed"] == 0 and got["best"] == -1 and np.array_equal(gd, pr.clip(depth, pr.FAR_M))
    assert got["valid_points"] == c["rec"]["valid_points"]


def test_a_tie_goes_to_the_lowest_hypothesis(clean):
    c = _case("64x48")
    g = pr.clip(c["depth"], pr.FAR_M)
    P = pr.points(g, c["tab"])
    valid = g.ravel() > 0
    counts = [int((pr.inliers(pr.plane_of_triple(g, P, t)[1], P, pr.DIST_M) & valid).sum()) for t in c["triples"]]
    top = int(np.argmax(counts))
    worse = [t for t, n in zip(c["triples"].tolist(), counts) if 3 <= n < counts[top]]
    assert len(worse) >= 8
    smp = worse[:3] + [c["triples"][top].tolist()] + worse[3:6] + [c["triples"][top].tolist()] + worse[6:8]
    got, gd = _edge(clean, c["depth"], c["tab"], iters=10, samples=smp)
    rec, grasp = pr.remove_plane(c["depth"], c["tab"], pr.FAR_M, pr.DIST_M, smp)
    assert got["best"] == rec["best"] == 3 and got["best_count"] == counts[top]
    assert [got[k] for k in PLANE_KEYS] == [rec[k] for k in PLANE_KEYS] and np.array_equal(gd, grasp)
    # a poor hypothesis alone: the refit moves the plane and the re-selection takes pixels the hypothesis did not count
    poor = [min(zip(counts, c["triples"].tolist()), key=lambda v: v[0] if v[0] >= 100 else 10 ** 9)[1]]
    got, gd = _edge(clean, c["depth"], c["tab"], iters=1, samples=poor)
    rec, grasp = pr.remove_plane(c["depth"], c["tab"], pr.FAR_M, pr.DIST_M, poor)
    assert [got[k] for k in PLANE_KEYS] == [rec[k] for k in PLANE_KEYS] and np.array_equal(gd, grasp)
    assert got["found"] == 1 and got["removed"] != got["best_count"]


@pytest.mark.parametrize("iters", [1, 256])
def test_fewest_and_most_hypotheses(clean, iters):
    c = _case("64x48")
    got, gd = _edge(clean, c["depth"], c["tab"], iters=iters)
    tri = pr.samples(c["depth"], pr.FAR_M, iters, pr.SEED)
    rec, grasp = pr.remove_plane(c["depth"], c["tab"], pr.FAR_M, pr.DIST_M, tri)
    assert [got[k] for k in PLANE_KEYS] == [rec[k] for k in PLANE_KEYS] and np.array_equal(gd, grasp)
    assert got["found"] == 1 and 0 <= got["best"] < iters


def test_the_same_upload_twice_gives_the_same_bytes(clean):
    c = _case("67x53")
    boxes = _boxes(c)
    runs = []
    for _ in range(2):
        _upload(clean, c)
        clean.depth_set_event(darknet.EVENT_GRASP)
        p = darknet.Plane()
        assert darknet.lib().y2_depth_plane(clean.net, p) == 0
        gd, g16 = clean.depth_grasp_aligned((c["dh"], c["dw"]))
        runs.append((bytes(p)[:20] + bytes(p)[24:], gd.tobytes(), g16.tobytes(), clean.depth_boxes(boxes).tobytes(),
                     b"".join(a.tobytes() for a in clean.depth_aligned())))
    assert runs[0] == runs[1]


FRAME = np.random.default_rng(7).integers(0, 255, size=(72, 96, 4), dtype=np.uint8)       # BGRA, no 255 of its own
RECTS = [None, (5, 3, 40, 44), (50, 10, 37, 53)]
FAR = [0.0, 0.8, 1.3]


def test_off_means_off(workdir):
    """with removal never set, or set and then cleared, the depth stage returns what it returned before
    y2_depth_set_plane_removal was ever called"""
    c = _case("64x48")
    net, _, _ = _mini(workdir, 3, tag="planeoff")
    items = [(FRAME, r) for r in RECTS]
    boxes = _boxes(c)

    def run():
        net.depth_upload(c["depth"], c["body"], c["map"])
        out = [a.tobytes() for a in net.depth_aligned()] + [net.depth_boxes(boxes).tobytes()]
        dets, d3, counts = net.detect_regions_depth(items, FAR, 0.05, 0.4)
        return out + [counts.tobytes()] + [d.tobytes() for d in dets] + [d.tobytes() for d in d3]

    net.depth_set_camera_table(c["tab"])
    never = run()
    assert np.frombuffer(never[4], np.int32).sum() > 0
    with pytest.raises(darknet.Y2Error, match="plane removal"):
        net.depth_plane()
    net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, pr.ITERS, pr.SEED)
    assert run() == never                                     # on, in the Demo_what event: the same planes and statistics
    assert net.depth_plane()["found"] == 1
    net.depth_set_plane_removal(iters=0)
    assert run() == never
    with pytest.raises(darknet.Y2Error, match="plane removal"):
        net.depth_plane()                                     # the frame uploaded since did not go through it
    net.free()


@pytest.fixture(scope="module")
def plain(workdir):
    net, _, _ = _mini(workdir, 3, tag="planeplain")
    net.set_fusion(False)                                     # every layer's output is stored
    yield net
    net.free()


def _layers(net):
    assert darknet.lib().y2_forward_device(net.net, None) == 0
    return [net.pull_layer_output(i) for i in range(net.n)]


@pytest.mark.parametrize("letterbox", [False, True])
def test_grasp_filter_equals_host_whitened_crops(plain, letterbox):
    c = _case("64x48")
    items = [(FRAME, r) for r in RECTS]
    try:
        plain.depth_set_camera_table(c["tab"])
        plain.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, pr.ITERS, pr.SEED)
        plain.depth_upload(c["depth"], c["body"], c["map"])
        d8 = c["planes"][1]
        # filter off: the ingest is y2_ingest_regions_depth's, removal on or not
        plain.ingest_regions_depth(items, FAR, swap_rb=True, letterbox=letterbox)
        off = _layers(plain)
        plain.ingest_regions([(depth_rule.whiten(FRAME, r, d8, f), r) for r, f in zip(RECTS, FAR)], swap_rb=True, letterbox=letterbox)
        for a, b in zip(off, _layers(plain)):
            assert np.array_equal(a, b)
        # filter on: far_m's rule first, then every pixel of a filtered item's crop whose grasp16 is 0
        white = []
        for r, f in zip(RECTS, FAR):
            w = depth_rule.whiten(FRAME, r, d8, f)
            if f > 0:
                x, y, rw, rh = r
                w[y:y + rh, x:x + rw][c["g16"][y:y + rh, x:x + rw] == 0] = 255
            white.append((w, r))
        assert (white[0][0] == FRAME).all() and (white[2][0] != depth_rule.whiten(FRAME, RECTS[2], d8, FAR[2])).any()
        plain.ingest_regions(white, swap_rb=True, letterbox=letterbox)
        want = _layers(plain)
        plain.depth_set_grasp_filter(True)
        plain.ingest_regions_depth(items, FAR, swap_rb=True, letterbox=letterbox)
        got = _layers(plain)
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), "layer %d" % i
        assert not np.array_equal(got[0], off[0])
        # a frame uploaded without removal has no grasp16 to filter by: refused
        plain.depth_set_plane_removal(iters=0)
        plain.depth_upload(c["depth"], c["body"], c["map"])
        with pytest.raises(darknet.Y2Error, match="grasp filter"):
            plain.ingest_regions_depth(items, FAR, swap_rb=True, letterbox=letterbox)
        plain.depth_set_grasp_filter(False)
        plain.ingest_regions_depth(items, FAR, swap_rb=True, letterbox=letterbox)
        for a, b in zip(_layers(plain), off):
            assert np.array_equal(a, b)
    finally:
        plain.depth_set_grasp_filter(False)
        plain.depth_set_plane_removal(iters=0)
        plain.depth_set_camera_table(None)


def test_grasp_event_end_to_end_tiny_yolo_voc(workdir):
    """tiny-yolo-voc 416 with synthetic weights: y2_detect_regions_depth in the Grasp event gives the records that
    y2_depth_boxes gives for the returned boxes, and test_detector_img_for_grasping(im, imFilter) fills the objects that
    test_detector_img(imFilter) fills"""
    from tests.helpers import load_golden, materialize
    g = load_golden("tiny_yolo_voc_416_b1_kinect")
    cfg, wts, x = materialize(workdir, "tiny-yolo-voc", 416, 1, int(g["seed"]), float(g["head_gain"]))
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    c = _case("128x106")
    frame = np.ascontiguousarray((np.clip(x[0], 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1])     # BGR 416 x 416
    m = pr.color_map(416, 416, c["dh"], c["dw"], 31)
    net.depth_set_camera_table(c["tab"])
    net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, pr.ITERS, pr.SEED)
    net.depth_upload(c["depth"], c["body"], m)
    plane = net.depth_plane()
    assert [plane[k] for k in PLANE_KEYS] == [c["rec"][k] for k in PLANE_KEYS]       # the map does not enter the plane
    thresh = float(g["thresh"])
    demo_d, demo3, demo_c = net.detect_regions_depth([(frame, None)], None, thresh, 0.1)
    net.depth_set_event(darknet.EVENT_GRASP)
    dets, d3, counts = net.detect_regions_depth([(frame, None)], None, thresh, 0.1)
    assert int(counts[0]) > 0 and dets[0].tobytes() == demo_d[0].tobytes()
    host = net.depth_boxes(np.stack([dets[0][k] for k in ("x", "y", "w", "h")], axis=-1))
    _same(d3[0], host)
    assert (d3[0]["otsu"][d3[0]["valid"] == 1] == 255).all() and not np.array_equal(d3[0]["avg_mm"], demo3[0]["avg_mm"])
    # the reference's entry: the detection runs on imFilter
    filt = x[0].copy()
    filt[:, 100:300, 50:250] = 1.0
    a = net.test_detector_img_for_grasping(x[0], filt, thresh)
    b = net.test_detector_img(filt, thresh)
    assert a == b and len(a) > 0
    assert a != net.test_detector_img(x[0], thresh)
    net.free()


def test_refusals_leave_the_previous_state_usable(clean):
    net, c = clean, _case("64x48")
    boxes = _boxes(c)
    _upload(net, c)
    before = net.depth_plane()
    net.depth_set_event(darknet.EVENT_GRASP)
    stats = net.depth_boxes(boxes).tobytes()
    # more than 256 hypotheses: refused, and the options in force stay
    with pytest.raises(darknet.Y2Error, match="at most 256"):
        net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, 257, pr.SEED)
    # a table of another size, then no table: the upload is refused before any copy, the last frame stays
    net.depth_set_camera_table(np.zeros((c["dh"] + 1, c["dw"], 2), np.float32))
    with pytest.raises(darknet.Y2Error, match="camera table"):
        net.depth_upload(c["depth"], c["body"], c["map"])
    net.depth_set_camera_table(None)
    with pytest.raises(darknet.Y2Error, match="camera table"):
        net.depth_upload(c["depth"], c["body"], c["map"])
    assert net.depth_plane() == before and np.array_equal(net.depth_grasp_aligned((c["dh"], c["dw"]))[1], c["g16"])
    net.depth_set_camera_table(c["tab"])
    assert net.depth_boxes(boxes).tobytes() == stats
    net.depth_upload(c["depth"], c["body"], c["map"])         # 50 hypotheses still
    assert net.depth_plane() == before
    # the Grasp statistics of a frame that did not go through the removal
    net.depth_set_plane_removal(iters=0)
    net.depth_upload(c["depth"], c["body"], c["map"])
    with pytest.raises(darknet.Y2Error, match="Grasp event"):
        net.depth_boxes(boxes)
    with pytest.raises(darknet.Y2Error, match="Grasp event"):
        net.detect_regions_depth([(FRAME, None)], None, 0.05, 0.4)
    net.depth_set_event(darknet.EVENT_DEMO_WHAT)
    want = depth_rule.as_records([depth_rule.box_stats(b, *c["planes"], c["tab"]) for b in boxes], darknet.DET3D_DTYPE)
    _same(net.depth_boxes(boxes), want)
