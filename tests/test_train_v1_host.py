"""YOLOv1 training without a device: what the trainer accepts and refuses, the truth layout, the dense weight permutation,
the dense plan's ranges and the exports.  Refusals touch no device: they are decided before any allocation."""
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_v1_rule as V

NET = "[net]\nbatch=%d\nwidth=6\nheight=6\nchannels=3\n"
CONV4 = "[convolutional]\nfilters=4\nsize=3\nstride=1\npad=1\nactivation=leaky\n"
DENSE = "[connected]\noutput=%d\nactivation=linear\n"
DET = "[detection]\nclasses=1\ncoords=4\nside=1\nnum=1\n"           # 1 * (5 * 1 + 1) = 6 inputs

V1_REFUSALS = {
    "random": (NET % 2 + CONV4 + DENSE % 6 + DET + "random=1\n", r"layer 2 \(detection\).*random=1"),
    "detection_in_the_middle": (NET % 2 + CONV4 + DENSE % 6 + DET + DET, r"layer 2 \(detection\).*last layer"),
    "coords5": (NET % 2 + CONV4 + DENSE % 7 + DET.replace("coords=4", "coords=5"), r"layer 2 \(detection\).*coords=5"),
    "bn_dense_batch1": (NET % 1 + CONV4 + "[connected]\noutput=6\nbatch_normalize=1\nactivation=leaky\n" + DET,
                        r"layer 1 \(connected\).*divides by zero"),
    "dense_activation": (NET % 2 + CONV4 + DENSE.replace("linear", "tanh") % 6 + DET, r"layer 1 \(connected\).*activation"),
    "dropout_first": (NET % 2 + "[dropout]\nprobability=.5\n" + DENSE % 6 + DET, r"layer 0 \(dropout\).*in front"),
    # the head behind an image: the device holds it by pixel, the reference's row is by channel (7x7x30 in front of side=7 alike)
    "detection_behind_an_image": (NET % 2 + "[convolutional]\nfilters=13\nsize=3\nstride=1\npad=1\nactivation=linear\n"
                                  "[detection]\nclasses=3\ncoords=4\nside=6\nnum=2\n", r"layer 1 \(detection\).*\[connected\] in front"),
    "detection_behind_a_maxpool": (NET % 2 + "[convolutional]\nfilters=13\nsize=3\nstride=1\npad=1\nactivation=linear\n[maxpool]\nsize=2\nstride=2\n"
                                   "[detection]\nclasses=3\ncoords=4\nside=3\nnum=2\n", r"layer 2 \(detection\).*\[connected\] in front"),
    # the carve-out: outside a [detection] network both stay refused, by layer
    "dense_in_classifier": (NET % 2 + CONV4 + DENSE % 4 + "[softmax]\n[cost]\n", r"layer 1 \(connected\).*\[detection\]"),
    "dropout_in_classifier": (NET % 2 + CONV4 + "[dropout]\nprobability=.5\n[avgpool]\n[softmax]\n[cost]\n", r"layer 1 \(dropout\).*\[detection\]"),
    "strided_conv": (NET % 2 + CONV4.replace("stride=1", "stride=2") + DENSE % 6 + DET, r"layer 0 \(convolutional\).*stride 2"),
    "local": (NET % 2 + CONV4 + "[local]\nsize=3\nstride=1\npad=1\nfilters=2\nactivation=leaky\n" + DENSE % 6 + DET, r"layer 1 \(local\)"),
}


def parse(tmp_path, text):
    cfg = str(tmp_path / "v1.cfg")
    with open(cfg, "w") as f:
        f.write(text)
    return darknet.Network.parse_network_cfg(cfg)


@pytest.mark.parametrize("what", sorted(V1_REFUSALS))
def test_refusals_name_the_layer(tmp_path, what):
    text, pattern = V1_REFUSALS[what]
    net = parse(tmp_path, text)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.truth_floats()
    net.free()


def test_a_detection_head_on_the_wrong_input_size_is_refused(tmp_path):
    """side*side*((1+coords)*num+classes) must be what the layer in front gives: the parser already says so, for every cfg;
    the trainer's own check of the count only guards a network whose layer fields were set by hand"""
    with pytest.raises(darknet.Y2Error, match=r"side\*side\*\(\(1\+coords\)\*num\+classes\) = 6"):
        parse(tmp_path, NET % 2 + CONV4 + DENSE % 7 + DET).train_prepare()


@pytest.mark.parametrize("name,want", [("H", 72), ("I", 72)])
def test_truth_floats_of_a_detection_network(tmp_path, name, want):
    cfg, _, _ = V.materialize(str(tmp_path), name, 1)
    net = darknet.Network.parse_network_cfg(cfg)
    assert net.truth_floats() == want == V.truths(name, 1)[0].size          # side*side*(1+coords+classes), no device touched
    net.free()


@pytest.mark.parametrize("outputs,c,h,w", [(5, 6, 6, 6), (3, 4, 2, 5), (4, 31, 1, 1), (1, 1, 1, 1)])
def test_dense_weight_layout_is_a_permutation_and_round_trips(outputs, c, h, w):
    L = darknet.lib()
    k = c * h * w
    ref = np.arange(outputs * k, dtype=np.float32) + 0.5
    packed, back = np.zeros_like(ref), np.zeros_like(ref)
    L.y2_train_pack_dense_weights(ref.ctypes.data, packed.ctypes.data, outputs, c, h, w)
    L.y2_train_unpack_dense_weights(packed.ctypes.data, back.ctypes.data, outputs, c, h, w)
    assert np.array_equal(back, ref) and np.array_equal(np.sort(packed), ref)
    want = ref.reshape(outputs, c, h, w).transpose(0, 2, 3, 1).reshape(-1)      # K in (y, x, c) order, rows unchanged
    assert np.array_equal(packed, want)
    if h * w == 1:
        assert np.array_equal(packed, ref)


@pytest.mark.parametrize("product", [darknet.DENSE_FORWARD, darknet.DENSE_DINPUT])
def test_dense_plan_ranges_cover_the_reduction(product):
    step = 32 if product == darknet.DENSE_FORWARD else 64
    for rows in (1, 3, 33, 64, 65):
        for inputs in (1, 31, 216, 1000, 12544):
            for outputs in (1, 5, 117, 130, 1470):
                total = inputs if product == darknet.DENSE_FORWARD else outputs
                cols = outputs if product == darknet.DENSE_FORWARD else inputs
                most = darknet.train_dense_plan(rows, inputs, outputs, product, 1 << 20)[0]
                assert most == (total + step - 1) // step
                for forced in (0, 1, 3, most):
                    n, ws, bounds = darknet.train_dense_plan(rows, inputs, outputs, product, forced)
                    assert 1 <= n <= most and (forced == 0 or n == min(forced, most))
                    assert bounds[0] == 0 and bounds[-1] == total and np.all(np.diff(bounds) > 0)      # no gap, no overlap, none empty
                    assert np.all(bounds[:-1] % step == 0)
                    assert ws == (n * rows * cols * 4 if n > 1 else 0)
                # a function of the shape alone: asked twice, answered alike
                assert darknet.train_dense_plan(rows, inputs, outputs, product)[0] == darknet.train_dense_plan(rows, inputs, outputs, product)[0]
    with pytest.raises(darknet.Y2Error):
        darknet.train_dense_plan(0, 4, 4, product)
    # the weights dwarf the partial sums at tiny-yolo-v1's shape
    n, ws, _ = darknet.train_dense_plan(32, 12544, 1470, product)
    assert n > 1 and ws < 0.15 * 1470 * 12544 * 4


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"y2h_train_dense_plan", "y2h_train_dense_forward", "y2h_train_dense_dweight", "y2h_train_dense_dinput",
            "y2_train_pack_dense_weights", "y2_train_unpack_dense_weights", "y2h_train_detection_loss",
            "y2h_train_detection_scratch_bytes", "y2_train_detection_stats", "y2h_train_dropout", "y2h_train_bn_stats_rate"}
    assert want <= have, want - have
