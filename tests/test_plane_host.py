"""The rule of the table-plane removal on the host: the exported functions of include/y2_plane_rule.h against its numpy
restatement (array_equal), the independent solver on the fixture scenes (the condition on the inputs that the GPU tests
rely on, checked here and not assumed), and the refusals that need no device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import plane_rule as pr


@pytest.fixture(scope="module", params=pr.SCENES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def fixture_scene(request):
    dh, dw, seed = request.param
    depth, tab, label = pr.scene(dh, dw, seed)
    triples = pr.samples(depth, pr.FAR_M, pr.ITERS, pr.SEED)
    return depth, tab, label, triples


def test_sampler_equals_the_restatement(fixture_scene):
    depth, tab, label, triples = fixture_scene
    got = darknet.plane_samples(depth, pr.FAR_M, pr.ITERS, pr.SEED)
    assert np.array_equal(got, triples) and (triples >= 0).all()
    g = pr.clip(depth, pr.FAR_M).ravel()
    assert (g[triples] > 0).all() and all(len(set(t)) == 3 for t in triples.tolist())
    # the state runs on from one hypothesis to the next: the second half is not a restart of the first
    assert not np.array_equal(got[:25], got[25:])


def test_sampler_gives_up_after_64_draws():
    depth = np.zeros((8, 8), np.uint16)
    depth[3, 4] = 700; depth[5, 1] = 650                       # two valid pixels can never fill a triple
    got = darknet.plane_samples(depth, 1.0, 4, 5)
    assert np.array_equal(got, pr.samples(depth, 1.0, 4, 5)) and (got == -1).all()
    depth[:] = 2000                                            # everything beyond far_m
    assert (darknet.plane_samples(depth, 1.0, 3, 5) == -1).all()


def test_plane_from_points_equals_the_restatement(fixture_scene):
    depth, tab, label, triples = fixture_scene
    g = pr.clip(depth, pr.FAR_M)
    P = pr.points(g, tab)
    for t in triples:
        ok, want = pr.plane_of_points(P[t[0]], P[t[1]], P[t[2]])
        got_ok, got = darknet.plane_from_points(P[t[0]], P[t[1]], P[t[2]])
        assert got_ok == ok == 1 and np.array_equal(got, want), (t, got, want)
    # degenerate: collinear points, a repeated point
    for pts in ([[0, 0, 1], [1, 1, 2], [2, 2, 3]], [[0.5, 0.25, 1], [0.5, 0.25, 1], [0, 1, 1]]):
        ok, want = pr.plane_of_points(*pts)
        got_ok, got = darknet.plane_from_points(*pts)
        assert got_ok == ok == 0 and not got.any()


def test_plane_fit_equals_the_restatement(fixture_scene):
    depth, tab, label, triples = fixture_scene
    g = pr.clip(depth, pr.FAR_M)
    P = pr.points(g, tab)
    valid = g.ravel() > 0
    rec, _ = pr.remove_plane(depth, tab, pr.FAR_M, pr.DIST_M, triples)
    assert rec["found"] == 1
    _, h = pr.plane_of_triple(g, P, triples[rec["best"]])
    S = pr.tree_sums(P, pr.inliers(h, P, pr.DIST_M) & valid)
    assert S[0] == rec["best_count"]
    ok, want = pr.fit(S)
    got_ok, got = darknet.plane_fit(S)
    assert got_ok == ok == 1 and np.array_equal(got, want)
    assert np.array_equal(want, [rec[k] for k in "abcd"]) and want[3] > 0
    assert abs(np.linalg.norm(want[:3]) - 1) < 1e-12
    # any other subset fits the same way; fewer than three points do not fit
    for k in range(3):
        sel = valid & (np.arange(len(P)) % 3 == k)
        S = pr.tree_sums(P, sel)
        assert np.array_equal(darknet.plane_fit(S)[1], pr.fit(S)[1])
    assert darknet.plane_fit(np.array([2.0] + [0.0] * 9))[0] == 0


def test_fixture_scenes_meet_the_condition(fixture_scene):
    """the independent solver removes every table pixel and no object pixel, and no valid point is within 1 mm of the
    threshold -- which is what lets the GPU tests ask for an equal mask from two different arithmetics"""
    depth, tab, label, triples = fixture_scene
    found, coef, mask, dist = pr.solve_independent(depth, tab, pr.FAR_M, pr.DIST_M, triples)
    assert found == 1
    assert (label == pr.TABLE).sum() > 0.4 * label.size and (label == pr.OBJECT).any() and (label == pr.FAR).any() and (label == pr.NONE).any()
    assert mask[label == pr.TABLE].all()
    assert not mask[label == pr.OBJECT].any() and not mask[(label == pr.FAR) | (label == pr.NONE)].any()
    valid = (label == pr.TABLE) | (label == pr.OBJECT)
    margin = np.abs(dist[valid] - pr.DIST_M).min()
    assert margin >= 1e-3, margin
    # and the restatement agrees with it: the same mask, coefficients within 1e-6
    rec, grasp = pr.remove_plane(depth, tab, pr.FAR_M, pr.DIST_M, triples)
    assert rec["found"] == 1 and np.array_equal(grasp == 0, mask | ~valid)
    assert np.abs(np.array([rec[k] for k in "abcd"]) - coef).max() < 1e-6
    assert rec["removed"] == int(mask.sum()) == int((label == pr.TABLE).sum())


def test_refusals_that_need_no_device():
    net = darknet.CNetwork()                                   # an empty network: every option check comes first
    L = darknet.lib()
    for far, dist, iters in ((1.0, 0.02, 257), (0.0, 0.02, 50), (-1.0, 0.02, 50), (float("nan"), 0.02, 50), (float("inf"), 0.02, 50),
                             (1.0, 0.0, 50), (1.0, float("nan"), 50), (1.0, float("inf"), 50)):
        o = darknet.PlaneOpts(far, dist, iters, 1, None)
        assert L.y2_depth_set_plane_removal(net, C.byref(o)) != 0
        assert L.y2_last_error().decode().startswith("y2_depth_set_plane_removal"), L.y2_last_error()
        L.y2_failed_and_clear()
    assert L.y2_depth_set_event(net, 2) != 0 and b"unknown event" in L.y2_last_error()
    L.y2_failed_and_clear()
    depth = np.zeros((4, 4), np.uint16)
    out = np.zeros((2, 3), np.int32)
    assert L.y2_plane_samples(None, 4, 4, 1.0, 2, 1, out.ctypes.data) == -1
    assert L.y2_plane_samples(depth.ctypes.data, 0, 4, 1.0, 2, 1, out.ctypes.data) == -1


def test_grasping_entry_is_exported():
    L = darknet.lib()
    for name in ("test_detector_img_for_grasping", "y2_depth_set_plane_removal", "y2_depth_plane", "y2_depth_grasp_aligned",
                 "y2_depth_set_event", "y2_depth_set_grasp_filter", "y2_plane_samples", "y2_plane_from_points", "y2_plane_fit"):
        assert hasattr(L, name), name
