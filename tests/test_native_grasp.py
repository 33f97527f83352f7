"""The Grasp event from a C program written as the Kinect application would write it (tests/native/kinect_grasp_like.c):
it compiles against include/ and links without a GPU; on the GPU its plane record and objects equal the Python path's."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from tests import plane_rule as pr
from tests.test_native_callers import build


def test_grasp_caller_compiles_and_links(workdir):
    build(workdir, "kinect_grasp_like", "gcc", "kinect_grasp_like.c")


@pytest.mark.gpu
def test_grasp_caller_equals_the_python_path(workdir):
    from sr_object_detection_amd import darknet
    from tests.helpers import load_golden, materialize

    g = load_golden("mini_64_b3")
    cfg, wts, _ = materialize(workdir, "mini", 64, 1, int(g["seed"]), float(g["head_gain"]), tag="graspc")
    dh, dw, seed = pr.SCENES[0]
    H, W = 72, 96
    depth, table, _ = pr.scene(dh, dw, seed)
    body = np.random.default_rng(5).choice(np.array([0, 1, 2, 255], np.uint8), (dh, dw))
    m = pr.color_map(H, W, dh, dw, 6)
    frame = np.random.default_rng(7).integers(0, 255, size=(H, W, 3), dtype=np.uint8)
    fpath, dpath = os.path.join(workdir, "grasp_frame.u8"), os.path.join(workdir, "grasp_scene.bin")
    with open(fpath, "wb") as f:
        np.array(frame.shape, dtype=np.int32).tofile(f)
        frame.tofile(f)
    with open(dpath, "wb") as f:
        np.array(depth.shape, dtype=np.int32).tofile(f)
        for a in (depth, body, m, table):
            np.ascontiguousarray(a).tofile(f)
    thresh = 0.05
    exe = build(workdir, "kinect_grasp_like", "gcc", "kinect_grasp_like.c")
    out = subprocess.run([exe, cfg, wts, fpath, dpath, repr(thresh), repr(pr.FAR_M), repr(pr.DIST_M), str(pr.ITERS), str(pr.SEED)],
                         capture_output=True, text=True, timeout=600, check=True, env=dict(os.environ, Y2_STRICT="1")).stdout.splitlines()
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    net.depth_set_camera_table(table)
    net.depth_set_plane_removal(pr.FAR_M, pr.DIST_M, pr.ITERS, pr.SEED)
    net.depth_set_event(darknet.EVENT_GRASP)
    net.depth_upload(depth, body, m)
    dets, d3, counts = net.detect_regions_depth([(frame, None)], None, thresh, 0.1, swap_rb=True, letterbox=False)
    plane = net.depth_plane()
    net.free()
    pl = [l.split()[1:] for l in out if l.startswith("PLANE ")]
    assert len(pl) == 1
    assert [int(v) for v in pl[0][:5]] == [plane[k] for k in ("found", "best", "valid_points", "best_count", "removed")]
    assert [float(v) for v in pl[0][5:]] == [plane[k] for k in "abcd"] and plane["found"] == 1
    objs = [l.split()[1:] for l in out if l.startswith("OBJ ")]
    assert ("COUNT %d" % counts[0]) in out and len(objs) == int(counts[0]) > 0
    for o, d, s in zip(objs, dets[0], d3[0]):
        assert (int(o[0]), o[1]) == (int(d["obj_id"]), "class%d" % d["obj_id"])
        want = [d["prob"], d["x"], d["y"], d["w"], d["h"], s["cam_x"], s["cam_y"], s["cam_z"], s["cam_w"], s["cam_h"]]
        assert np.array_equal(np.array([float(v) for v in o[2:12]], np.float32), np.array(want, np.float32), equal_nan=True), (o, want)
        assert (int(o[12]), int(o[13])) == (int(s["belongs"]), int(s["body_id"]))
