"""[normalization] / [activation] networks on the GPU against the reference's own CPU path (tests/golden/
gen_lrn_golden.py): the output and every dumped layer within 1e-4 of the largest reference value, bit for bit in strict
mode; the planned kernel names; an item of a batch equals a batch-1 run; graph replay, set_batch_network and
resize_network behave as for the other layers ([activation] refuses a resize, as the reference does); fp16 storage."""
from __future__ import annotations

import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

NETS = ["lrn_mini", "lrn_route", "act_flat", "lrn_mini_f16"]
NORMALIZATION, ACTIVE = 10, 14                              # LAYER_TYPES


def _net(tmp, name, wseed, batch=None, width=None, height=None, spec=None, tag=""):
    cfg = os.path.join(str(tmp), "%s%s_b%s_%sx%s.cfg" % (name, tag, batch, width, height))
    with open(cfg, "w") as f:
        f.write(zoo.lrn_cfg_text(name, batch, width, height, spec))
    wts = os.path.join(str(tmp), "%s%s_s%d.weights" % (name, tag, wseed))
    if not os.path.exists(wts):
        synth.write_weights(wts, zoo.lrn_resolve(name, width, height, spec), wseed, 1.0)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    return net


def _close(got, ref, what, strict):
    got = np.asarray(got, np.float32).reshape(ref.shape)
    if strict:
        assert np.array_equal(got, ref), "%s: strict mode differs from the reference (max %.3g)" % (what, float(np.abs(got - ref).max()))
        return
    bar = 1e-4 * float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    assert err <= bar, "%s: max error %.3g > %.3g" % (what, err, bar)


def _expected_kernel(net, i, strict):
    l = net.layer(i)
    if l.type == NORMALIZATION:
        return "lrn_ref" if strict else "lrn_nhwc"
    return "activation(%s)" % ["logistic", "relu", "relie", "linear", "ramp", "tanh", "plse", "leaky", "elu", "loggy", "stair",
                               "hardtan", "lhtan"][l.activation]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", NETS)
def test_golden(tmp_path, name, strict):
    g = load_golden(name)
    net = _net(tmp_path, name, int(g["seeds"][0]))
    net.set_strict(strict)
    out = net.network_predict(g["x"])
    _close(out, g["out"], name + " output", strict)
    seen = 0
    for i in range(net.n):
        if net.layer(i).type in (NORMALIZATION, ACTIVE):
            assert net.layer_kernel(i) == _expected_kernel(net, i, strict), (i, net.layer_kernel(i))
            seen += 1
        _close(net.pull_layer_output(i), g["layer_%02d" % i], "%s layer %d (%s)" % (name, i, net.layer_kernel(i)), strict)
    assert seen >= 1
    if name == "lrn_route":
        # no copy kernel: layer 0 writes into the route's buffer, so the first [normalization], checked against its dump
        # above, read 8 channels at a pixel stride of 14
        assert net.layer_kernel(3) == "route(zero-copy)", net.layer_kernel(3)
    net.set_timing(True)                                    # both types have their slot in the per-layer times
    net.network_predict(g["x"])
    ms = net.layer_times_ms()
    assert len(ms) == net.n and all(ms[i] > 0 for i in range(net.n) if net.layer(i).type in (NORMALIZATION, ACTIVE))
    net.free()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", ["lrn_mini", "lrn_route"])
def test_batch_item_equals_a_batch_of_one(tmp_path, name, strict):
    g = load_golden(name)
    ws, B = int(g["seeds"][0]), zoo.LRN[name][2]
    net = _net(tmp_path, name, ws)
    net.set_strict(strict)
    full = net.network_predict(g["x"]).reshape(B, -1)
    lrn = [i for i in range(net.n) if net.layer(i).type == NORMALIZATION]
    full_l = {i: net.pull_layer_output(i).reshape(B, -1) for i in lrn}
    one = _net(tmp_path, name, ws, batch=1)
    one.set_strict(strict)
    for b in range(B):
        out = one.network_predict(g["x"][b:b + 1])
        assert np.array_equal(out, full[b]), "item %d differs from its batch-1 run by %.3g" % (b, float(np.abs(out - full[b]).max()))
        for i in lrn:
            assert np.array_equal(one.pull_layer_output(i).reshape(-1), full_l[i][b]), (b, i)
    # the same through set_batch_network on the batch-B network
    net.set_batch_network(1)
    assert np.array_equal(net.network_predict(g["x"][B - 1:B]), full[B - 1])
    net.free(); one.free()


@pytest.mark.parametrize("name", NETS)
def test_graph_replay_equals_eager(tmp_path, name):
    g = load_golden(name)
    net = _net(tmp_path, name, int(g["seeds"][0]))
    eager = net.network_predict(g["x"])
    net.set_graph(True)
    first = net.network_predict(g["x"])                     # records
    again = net.network_predict(g["x"])                     # replays
    assert np.array_equal(first, eager) and np.array_equal(again, eager)
    net.free()


def test_resize_network(tmp_path):
    """[normalization] resizes (network.c:354).  lrn_mini itself cannot: its [activation] sits in front of the [avgpool]
    (the next test), so this runs lrn_mini without that layer"""
    spec = [e for e in zoo.LRN["lrn_mini"][3] if e[0] != "activation"]
    x = synth.image_batch(3, 3, 14, 16, 77) * np.float32(2) - np.float32(1)
    net = _net(tmp_path, "lrn_mini", 401, spec=spec, tag="_noact")
    net.network_predict(load_golden("lrn_mini")["x"])       # a plan at the first size
    net.resize_network(16, 14)
    got = net.network_predict(x)
    fresh = _net(tmp_path, "lrn_mini", 401, width=16, height=14, spec=spec, tag="_noact")
    want = fresh.network_predict(x)
    assert np.array_equal(got, want)
    assert np.array_equal(net.pull_layer_output(1), fresh.pull_layer_output(1)) and net.layer_kernel(1) == "lrn_nhwc"
    net.free(); fresh.free()


def test_activation_refuses_resize(tmp_path):
    g = load_golden("lrn_mini")
    net = _net(tmp_path, "lrn_mini", int(g["seeds"][0]))
    before = net.network_predict(g["x"])
    with pytest.raises(darknet.Y2Error, match="Cannot resize this type of layer"):
        net.resize_network(16, 14)
    assert np.array_equal(net.network_predict(g["x"]), before)      # refused before anything changed
    net.free()


def test_fp16_mode(tmp_path):
    """lrn_mini_f16 (32 filters in front, a [activation] the half kernels have) under y2_set_half: the fp32 golden's top-1,
    probabilities within 1e-2; the half kernels are the ones planned"""
    g = load_golden("lrn_mini_f16")
    net = _net(tmp_path, "lrn_mini_f16", int(g["seeds"][0]))
    net.set_half(True)
    out = net.network_predict(g["x"]).reshape(g["out"].shape)
    assert net.layer_kernel(1) == "lrn_nhwc_f16" and net.layer_kernel(4) == "activation_f16(leaky)", [net.layer_kernel(i) for i in range(net.n)]
    err = float(np.abs(out - g["out"]).max())
    print("fp16 mode: max |p - p_ref| = %.3g" % err)
    assert np.array_equal(out.argmax(1), g["out"].argmax(1)) and err <= 1e-2
    net.free()


def test_fp16_mode_refusals(tmp_path):
    """an activation the half kernels lack (lrn_mini's hardtan), as for convolutions"""
    spec = [("conv", 32, 3, 1, "leaky")] + zoo.LRN["lrn_mini"][3][1:]
    net = _net(tmp_path, "lrn_mini", 401, spec=spec, tag="_c32")
    net.set_half(True)
    with pytest.raises(darknet.Y2Error, match="fp16 mode: layer 4: activation .* has no half-precision form"):
        net.network_predict(load_golden("lrn_mini")["x"])
    net.set_half(False)
    assert np.isfinite(net.network_predict(load_golden("lrn_mini")["x"])).all()
    net.free()
