"""[normalization] / [activation] without a GPU: the sections parse with the reference's options, defaults, aliases and
stderr lines; what the reference cannot run is refused with a message; the numpy rules of tests/lrn_rule.py reproduce
every [normalization] / [activation] layer the compiled reference dumped (tests/golden/gen_lrn_golden.py) -- the
sequential rule bit for bit, the closed form the device kernel evaluates within a quarter of the GPU tests' tolerance;
weights saved from such a network load back unchanged."""
from __future__ import annotations

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import lrn_rule
from tests.helpers import load_golden

NETS = ["lrn_mini", "lrn_route", "act_flat", "lrn_mini_f16"]
HARDTAN, LOGISTIC, ELU, LINEAR = 11, 0, 8, 3                # ACTIVATION (include/sr_yolo2.h)


def _parse(tmp_path, text):
    cfg = tmp_path / "n.cfg"
    cfg.write_text(text)
    return darknet.Network.parse_network_cfg(str(cfg))


def test_lrn_mini_parses(tmp_path, capfd):
    net = _parse(tmp_path, zoo.lrn_cfg_text("lrn_mini"))
    err = capfd.readouterr().err
    types = [darknet.LAYER_TYPES[net.layer(i).type] for i in range(net.n)]
    assert types == ["CONVOLUTIONAL", "NORMALIZATION", "MAXPOOL", "CONVOLUTIONAL", "ACTIVE", "AVGPOOL", "SOFTMAX"]
    n = net.layer(1)
    assert (n.w, n.h, n.c, n.out_w, n.out_h, n.out_c, n.inputs, n.outputs, n.batch) == (12, 10, 12, 12, 10, 12, 1440, 1440, 3)
    assert (n.size, n.alpha, n.beta, n.kappa) == (5, np.float32(.05), np.float32(.75), 1.0)
    a = net.layer(4)
    assert (a.w, a.h, a.c, a.out_w, a.out_h, a.out_c, a.inputs, a.outputs, a.activation) == (6, 5, 10, 6, 5, 10, 300, 300, HARDTAN)
    assert "Local Response Normalization Layer: 12 x 10 x 12 image, 5 size\n" in err
    assert "Activation Layer: 300 inputs\n" in err
    assert "beta: Using default '0.750000'\n" in err and "kappa: Using default '1.000000'\n" in err
    assert "alpha: Using default" not in err
    assert net.output_size == 10
    net.free()


@pytest.mark.parametrize("name", NETS)
def test_parse_matches_the_zoo_resolver(tmp_path, name):
    net = _parse(tmp_path, zoo.lrn_cfg_text(name))
    want = zoo.lrn_resolve(name)
    assert net.n == len(want)
    for i, l in enumerate(want):
        got = net.layer(i)
        assert got.outputs == l["outputs"], i
        if l["type"] in ("normalization", "activation"):
            assert (got.out_w, got.out_h, got.out_c) == (l["out_w"], l["out_h"], l["out_c"]), i
        if l["type"] == "normalization":
            assert (got.size, got.alpha, got.beta, got.kappa) == (l["size"], np.float32(l["alpha"]), np.float32(l["beta"]), np.float32(l["kappa"]))
    net.free()


def test_defaults_aliases_and_flat_activation(tmp_path, capfd):
    net = _parse(tmp_path, "[net]\nbatch=2\nwidth=4\nheight=3\nchannels=7\n\n[lrn]\n\n[connected]\noutput=5\nactivation=linear\n\n[activation]\n")
    err = capfd.readouterr().err
    n, a = net.layer(0), net.layer(2)
    assert darknet.LAYER_TYPES[n.type] == "NORMALIZATION" and darknet.LAYER_TYPES[a.type] == "ACTIVE"
    assert (n.size, n.alpha, n.beta, n.kappa) == (5, np.float32(.0001), np.float32(.75), 1.0)
    for line in ("alpha: Using default '0.000100'\n", "beta: Using default '0.750000'\n", "kappa: Using default '1.000000'\n",
                 "size: Using default '5'\n", "Local Response Normalization Layer: 4 x 3 x 7 image, 5 size\n",
                 "activation: Using default 'linear'\n", "Activation Layer: 5 inputs\n"):
        assert line in err, line
    assert (a.activation, a.inputs, a.outputs, a.batch, a.out_h, a.out_w, a.out_c) == (LINEAR, 5, 5, 2, 1, 1, 5)
    net.free()


def test_flat_net_activation_shapes(tmp_path):
    net = _parse(tmp_path, zoo.lrn_cfg_text("act_flat"))
    a = net.layer(2)
    assert (a.activation, a.inputs, a.outputs) == (ELU, 20, 20) and net.layer(3).inputs == 20
    net.free()


@pytest.mark.parametrize("text,msg", [
    # size/2 = 4 channels are read before c = 3 is looked at
    ("[net]\nbatch=1\nwidth=4\nheight=4\nchannels=3\n\n[normalization]\nsize=8\n", "reads 4 channels but the input has 3"),
    ("[net]\nbatch=1\nwidth=4\nheight=4\nchannels=3\n\n[normalization]\nsize=0\n", "size=0"),
    # a flat input: [softmax] leaves no image shape behind, nor does a [net] with inputs= only
    ("[net]\nbatch=1\nwidth=4\nheight=4\nchannels=3\n\n[connected]\noutput=8\n\n[softmax]\n\n[normalization]\n", "must output image"),
    ("[net]\nbatch=1\ninputs=8\n\n[lrn]\n", "must output image"),
    ("[net]\nbatch=1\ninputs=8\n\n[activation]\nactivation=relu\n", "activation layer 0 needs an image-shaped network input"),
    ("[net]\nbatch=1\nwidth=8\nheight=8\nchannels=3\n\n[crnn]\noutput_filters=4\nhidden_filters=4\n", r"\[crnn\].*faults"),
    ("[net]\nbatch=1\nwidth=8\nheight=8\nchannels=3\n\n[deconvolutional]\n", "outside"),
])
def test_refusals(tmp_path, text, msg):
    cfg = tmp_path / "bad.cfg"
    cfg.write_text(text)
    with pytest.raises(darknet.Y2Error, match=msg):
        darknet.Network.parse_network_cfg(str(cfg))


def test_size_half_equal_to_channels_is_accepted(tmp_path):
    net = _parse(tmp_path, "[net]\nbatch=1\nwidth=4\nheight=4\nchannels=3\n\n[normalization]\nsize=7\n")
    assert net.layer(0).size == 7 and net.layer(0).c == 3
    net.free()


def _lrn_and_activation_layers(name):
    w, h, b, spec = zoo.LRN[name]
    layers = zoo.lrn_resolve(name)
    for i, (e, l) in enumerate(zip(spec, layers)):
        if e[0] in ("lrn", "activation"):
            yield i, e, l, b


@pytest.mark.parametrize("name", NETS)
def test_rules_against_the_reference_dumps(name):
    g = load_golden(name)
    seen = 0
    for i, e, l, b in _lrn_and_activation_layers(name):
        x, ref = g["layer_%02d" % (i - 1)], g["layer_%02d" % i]
        if e[0] == "activation":
            assert np.array_equal(lrn_rule.activate(x, e[1]), ref), (name, i, e[1])
        else:
            x4 = x.reshape(b, l["c"], l["h"], l["w"])           # the reference's layout
            args = (l["size"], l["alpha"], l["beta"], l["kappa"])
            seq = lrn_rule.lrn_sequential(x4, *args, axis=1).reshape(-1)
            assert np.array_equal(seq, ref), "%s layer %d: the sequential rule differs from the reference by %.3g" % (
                name, i, float(np.abs(seq - ref).max()))
            clo = lrn_rule.lrn_closed(x4, *args, axis=1).reshape(-1)
            err, bar = float(np.abs(clo - ref).max()), 0.25e-4 * float(np.abs(ref).max())
            print("%s layer %d: closed form max error %.3g, bar %.3g" % (name, i, err, bar))
            assert err <= bar, (name, i, err, bar)
            assert float(np.abs(ref - x).max()) > 1e-3 * float(np.abs(x).max()), "the layer does nothing on this fixture"
        seen += 1
    assert seen >= 2 or name == "act_flat"


def test_non_finite_where_the_norm_is_not_positive():
    """size=4 alpha=1 kappa=.1 and a large value in channel 2 = size/2: once channel 2 has left the window its square is
    subtracted though it was never added, and the reference writes NaN (4 of them here, in channels 4 and 5)"""
    x = np.full((2, 6), .25, np.float32)
    x[:, 2] = 3
    seq = lrn_rule.lrn_sequential(x, 4, 1.0, .75, .1)
    clo = lrn_rule.lrn_closed(x, 4, 1.0, .75, .1)
    assert np.isnan(seq).sum() == 4 and np.isnan(seq[:, 4:]).all() and np.isfinite(seq[:, :4]).all()
    assert np.array_equal(np.isfinite(seq), np.isfinite(clo))


def test_activation_rule_formulas():
    x = np.array([-5, -1.5, -1, -.25, 0, .25, 1, 1.5, 3, 5], np.float32)
    assert np.array_equal(lrn_rule.activate(x, "hardtan"), np.clip(x, -1, 1))
    assert np.array_equal(lrn_rule.activate(x, "relu"), np.maximum(x, 0))
    assert np.allclose(lrn_rule.activate(x, "tanh"), np.tanh(x), atol=1e-6)
    assert np.allclose(lrn_rule.activate(x, "elu"), np.where(x >= 0, x, np.expm1(x)), atol=1e-6)
    assert np.array_equal(lrn_rule.activate(x, "stair"), np.array([-3, -1, -1, -.25, 0, 0, 0, .5, 1, 2], np.float32))   # activations.h:21-26 by hand
    assert sorted(lrn_rule.ACT_CODE) == sorted(lrn_rule.ACTIVATIONS) and len(lrn_rule.ACTIVATIONS) == 13


@pytest.mark.parametrize("name", NETS)
def test_weights_round_trip(tmp_path, name):
    """neither layer has weights: load_weights / save_weights pass over them as the reference does (parser.c:1009-1082)"""
    w, back = str(tmp_path / "n.weights"), str(tmp_path / "back.weights")
    synth.write_weights(w, zoo.lrn_resolve(name), 5, 1.0)
    net = _parse(tmp_path, zoo.lrn_cfg_text(name))
    net.load_weights(w)
    net.save_weights(back)
    assert open(w, "rb").read() == open(back, "rb").read()
    again = _parse(tmp_path, zoo.lrn_cfg_text(name))
    again.load_weights(back)
    for i in range(net.n):
        a, b = net.layer(i), again.layer(i)
        if darknet.LAYER_TYPES[a.type] == "CONVOLUTIONAL":
            k = a.n * a.c * a.size * a.size
            assert np.array_equal(np.ctypeslib.as_array(a.weights, (k,)), np.ctypeslib.as_array(b.weights, (k,)))
            assert np.array_equal(np.ctypeslib.as_array(a.biases, (a.n,)), np.ctypeslib.as_array(b.biases, (a.n,)))
    net.free(); again.free()


def test_resize_follows_the_reference(tmp_path):
    """network.c:340-360: NORMALIZATION resizes; ACTIVE is 'Cannot resize this type of layer' -- refused before anything
    changed, and not visited behind an [avgpool]"""
    spec = [e for e in zoo.LRN["lrn_mini"][3] if e[0] != "activation"]
    net = _parse(tmp_path, zoo.lrn_cfg_text("lrn_mini", spec=spec))
    net.resize_network(16, 14)
    n = net.layer(1)
    assert (n.w, n.h, n.out_w, n.out_h, n.c, n.inputs, n.outputs) == (16, 14, 16, 14, 12, 16 * 14 * 12, 16 * 14 * 12)
    assert (net.layer(2).out_w, net.layer(2).out_h) == (8, 7)
    net.free()
    net = _parse(tmp_path, zoo.lrn_cfg_text("lrn_mini"))
    with pytest.raises(darknet.Y2Error, match="Cannot resize this type of layer"):
        net.resize_network(16, 14)
    assert (net.net.w, net.net.h, net.layer(0).w) == (12, 10, 12)
    net.free()
    behind = [("conv", 4, 3, 1, "leaky"), ("avg",), ("activation", "relu"), ("softmax",)]
    net = _parse(tmp_path, zoo.lrn_cfg_text("lrn_mini", spec=behind))
    net.resize_network(16, 14)
    assert net.layer(1).w == 16
    net.free()
