"""char-rnn training without a device: the rule of tests/train_rnn_rule.py against the compiled reference's fixtures
(tests/golden/train_rnn_J.npz, _K.npz, _L.npz), what the trainer accepts and refuses, and get_rnn_data.

Refusals are decided before any device allocation: on a machine without a GPU a refusal that came after a device call would
carry HIP's message, not the layer's name, and an accepted network fails at its first allocation with HIP's.
"""
import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_rule as T
from tests import train_rnn_rule as R
from tests.helpers import load_golden

RULE_BOUND = 1e-5          # the generator's: the fp32 rule against every stored array
_RULE = {}


def golden_keys(g):
    out = []
    for key in sorted(g):
        if key.startswith("s") and "_l" in key and not key.endswith("_loss"):
            out.append((int(key[1]), int(key.split("_")[1][1:]), key.split("_", 2)[2], key))
    return out


def rule32(name, **how):
    key = (name,) + tuple(sorted(how.items()))
    if key not in _RULE:
        g = load_golden("train_rnn_" + name)
        _RULE[key] = R.rule_snapshots(R.NETS[name], int(g["seed"]), np.float32, **how)
    return _RULE[key]


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_the_rule_reproduces_the_reference(name):
    g = load_golden("train_rnn_" + name)
    _, snaps, losses = rule32(name)
    keys = golden_keys(g)
    worst = (0.0, "")
    for (k, i, a, key) in keys:
        e = T.err(g[key], snaps[k - 1][i][a].reshape(-1))
        worst = max(worst, (e, key))
        assert e <= RULE_BOUND, (key, e)
    for k in range(1, R.STEPS + 1):
        assert abs(float(g["s%d_loss" % k][0]) - losses[k - 1]) <= RULE_BOUND * abs(losses[k - 1])
    print("%s: fp32 rule against the reference <= %.3g at %s" % (name, worst[0], worst[1]))
    # every array of every sub-layer and the state after step 1; parameters and update buffers after the later steps
    rnn = [i for i, l in enumerate(R.NETS[name]["layers"]) if l[0] == "rnn"]
    for i in rnn:
        have = {a for (k, ii, a, _) in keys if k == 1 and ii == i}
        want = {"state", "output", "delta"} | {"%s.%s" % (s, a) for s in R.SUBS for a in
                                              ("output", "delta", "weights", "biases", "weight_updates", "bias_updates")}
        if R.NETS[name]["layers"][i][3]:
            want |= {"%s.%s" % (s, a) for s in R.SUBS for a in T.CONV_ARRAYS}
        assert want <= have, sorted(want - have)
        later = {a for (k, ii, a, _) in keys if k == 3 and ii == i}
        assert "self.weights" in later and "input.weight_updates" in later and "self.delta" not in later
    assert float(g["min_preact"]) >= T.KINK


def test_k_tells_the_last_steps_statistics_from_each_steps_own():
    """increment_layer does not advance mean and variance: the fixture must differ from a backward that uses every step's own"""
    g = load_golden("train_rnn_K")
    _, own, _ = rule32("K", per_step_stats=True)
    _, last, _ = rule32("K")
    for key in ("s1_l1_self.delta", "s1_l1_input.weight_updates", "s1_l0_output.delta", "s1_l0_self.weight_updates"):
        _, i, a = int(key[1]), int(key.split("_")[1][1:]), key.split("_", 2)[2]
        e_own, e_last = T.err(g[key], own[0][i][a].reshape(-1)), T.err(g[key], last[0][i][a].reshape(-1))
        print("%-28s reference against the rule with the last step's statistics %.3g, with each step's own %.3g" % (key, e_last, e_own))
        assert e_last <= RULE_BOUND and e_own > 1000 * RULE_BOUND
    # the forward does not depend on it
    assert np.array_equal(own[0][1]["state"], last[0][1]["state"])


def test_j_tells_the_copy_point_from_the_gpu_twins():
    """input.delta is self.delta AFTER the self sub-layer's backward (rnn_layer.c:161), not before it (:258, the GPU twin)"""
    g = load_golden("train_rnn_J")
    _, twin, _ = rule32("J", copy_point="before")
    _, cpu, _ = rule32("J")
    for key in ("s1_l1_input.delta", "s1_l1_input.weight_updates", "s1_l0_output.weight_updates"):
        i, a = int(key.split("_")[1][1:]), key.split("_", 2)[2]
        e_twin, e_cpu = T.err(g[key], twin[0][i][a].reshape(-1)), T.err(g[key], cpu[0][i][a].reshape(-1))
        print("%-28s reference against the CPU path's copy point %.3g, against the twin's %.3g" % (key, e_cpu, e_twin))
        assert e_cpu <= RULE_BOUND and e_twin > 1000 * RULE_BOUND


# ---- refusals, by name ----
NET = "[net]\nbatch=4\ninputs=8\ntime_steps=2\n"
RNN = "[rnn]\nbatch_normalize=%d\noutput=8\nhidden=8\nactivation=%s\n"
TAIL = "[connected]\noutput=8\nactivation=linear\n[softmax]\n[cost]\ntype=sse\n"
REFUSALS = {
    "gru": (NET + "[gru]\noutput=8\n" + TAIL, r"layer 0 \(gru\).*\[gru\] layer cannot be trained"),
    "shortcut": (NET + RNN % (0, "leaky") + "shortcut=1\n" + TAIL, r"layer 0 \(rnn\).*shortcut=1"),
    "loggy": (NET + RNN % (0, "leaky") + "logistic=2\n" + TAIL, r"layer 0 \(rnn\).*logistic=2"),
    "activation": (NET + RNN % (0, "tanh") + TAIL, r"layer 0 \(rnn\).*activation \d+ is not trainable"),
    "bn_one_row": ("[net]\nbatch=1\ninputs=8\ntime_steps=2\n" + RNN % (1, "leaky") + TAIL, r"layer 0 \(rnn\).*divides by zero"),
    "successor": (NET + RNN % (0, "leaky") + "[softmax]\n[cost]\ntype=sse\n", r"layer 0 \(rnn\).*must feed an \[rnn\] or a \[connected\]"),
    "second_successor": (NET + RNN % (0, "leaky") + RNN % (0, "leaky") + "[softmax]\n[cost]\ntype=sse\n", r"layer 1 \(rnn\).*must feed"),
    "last": (NET + RNN % (0, "leaky"), r"layer 0 \(rnn\).*must feed"),
    "adam": (NET.replace("inputs=8", "inputs=8\nadam=1") + RNN % (0, "leaky") + TAIL, r"adam=1"),
    "random": (NET.replace("inputs=8", "inputs=8\npolicy=random") + RNN % (0, "leaky") + TAIL, r"policy=random"),
    # a [connected] without an [rnn] in the network still trains only in front of [detection]
    "connected_alone": ("[net]\nbatch=2\nwidth=4\nheight=4\nchannels=1\n" + TAIL, r"layer 0 \(connected\) trains only in a network that ends in \[detection\]"),
    "dropout": (NET + RNN % (0, "leaky") + "[connected]\noutput=8\nactivation=linear\n[dropout]\nprobability=.5\n[softmax]\n[cost]\ntype=sse\n",
                r"layer 2 \(dropout\) trains only in a network that ends in \[detection\]"),
}


def parse(tmp_path, text):
    cfg = str(tmp_path / "r.cfg")
    with open(cfg, "w") as f:
        f.write(text)
    return darknet.Network.parse_network_cfg(cfg)


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["fp16"])
def test_refusals_name_the_layer(tmp_path, what):
    text, pattern = REFUSALS["successor" if what == "fp16" else what]
    net = parse(tmp_path, text)
    if what == "fp16":
        net.set_half(True)
        pattern = r"fp16 mode"
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    with pytest.raises(darknet.Y2Error, match=pattern):      # train_network_datum prepares lazily and refuses alike
        net.train_step(np.zeros(net.net.batch * net.net.inputs, np.float32), np.zeros(net.net.batch * 8, np.float32))
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_load_chars(bytes([1, 2, 3]), np.zeros(net.net.batch // net.net.time_steps, np.uint64))
    net.free()


@pytest.mark.parametrize("head", ["[net]\nbatch=4\nheight=4\nwidth=4\nchannels=3\ntime_steps=2\n",
                                  "[net]\nbatch=4\nheight=4\nwidth=4\nchannels=3\ntime_steps=2\n[convolutional]\nfilters=4\nsize=3\nstride=1\npad=1\nactivation=leaky\n"])
def test_an_rnn_behind_an_image_never_reaches_the_trainer(tmp_path, head):
    """The input sub-layer's weights are in the reference's column order and an image is ordered by pixel on the device: such a
    network must not train with permuted inputs.  The parser refuses it (a recurrent layer needs a flat input); the trainer
    guards the same for a network whose fields were set by hand."""
    with pytest.raises(darknet.Y2Error, match=r"recurrent layer needs a flat input"):
        parse(tmp_path, head + RNN % (0, "leaky") + TAIL)


def test_the_old_refusal_of_rnn_into_softmax_still_matches(tmp_path):
    """tests/test_train_host.py pins `layer 0 \\(rnn\\).*recurrent` for [rnn] -> [softmax] -> [cost]"""
    net = parse(tmp_path, "[net]\nbatch=2\ninputs=8\ntime_steps=2\n[rnn]\nbatch_normalize=0\noutput=8\nhidden=8\nactivation=leaky\n[softmax]\n[cost]\n")
    with pytest.raises(darknet.Y2Error, match=r"layer 0 \(rnn\).*recurrent"):
        net.train_prepare()
    net.free()


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_the_fixture_networks_are_accepted(tmp_path, name):
    """a flat input (inputs= without an image shape) in front of an [rnn], [connected] behind it: truth_floats answers"""
    net = parse(tmp_path, R.net_text(R.NETS[name]))
    assert net.truth_floats() == R.widths(R.NETS[name])[-1][1]
    assert net.net.batch == R.NETS[name]["B"] * R.NETS[name]["T"]
    net.free()


def test_train_pull_names(tmp_path):
    net = parse(tmp_path, R.net_text(R.NETS["J"]))
    with pytest.raises(darknet.Y2Error, match=r"no \[rnn\] layer"):
        net.train_pull(2, "self.delta")
    with pytest.raises(darknet.Y2Error, match=r"unknown array"):
        net.train_pull(0, "middle.delta")
    with pytest.raises(darknet.Y2Error, match=r"no trainer"):
        net.train_pull(0, "self.delta")
    net.free()


# ---- get_rnn_data ----
def test_get_rnn_data_equals_its_restatement():
    text = bytes([1, 2, 3, 4, 5, 6, 7, 3, 2, 1, 5])
    for start, batch, steps in (([0, 5], 2, 4), ([9, 10, 3], 3, 7), ([10], 1, 25)):     # wraps at len, more than once
        off, ref = np.array(start, np.uint64), list(start)
        for _ in range(3):
            x, y = darknet.get_rnn_data(text, off, 8, batch, steps)
            xr, yr = R.get_rnn_data(text, ref, 8, batch, steps)
            assert np.array_equal(x, xr) and np.array_equal(y, yr) and off.tolist() == ref
            assert x.sum() == y.sum() == batch * steps
    # rows are step-major and y is x one character on
    off = np.array([9], np.uint64)
    x, y = darknet.get_rnn_data(text, off, 8, 1, 4)
    assert x.argmax(axis=1).tolist() == [1, 5, 1, 2] and y.argmax(axis=1).tolist() == [5, 1, 2, 3] and off[0] == 2


@pytest.mark.parametrize("text, chars", [(bytes([1, 2, 0, 3]), 8), (bytes([1, 2, 9, 3]), 8)])
def test_get_rnn_data_refuses_a_bad_char(text, chars):
    off = np.array([0], np.uint64)
    with pytest.raises(darknet.Y2Error, match=r"Bad char"):
        darknet.get_rnn_data(text, off, chars, 1, 3)
    assert off[0] == 0                      # refused before an offset moved


def test_the_fused_forms_rule():
    """y2h_train_rnn_fused_fits, pinned: at most 128 rows (four 32-row accumulator tiles in a 16-wave workgroup), the backward
    partials ceil(hidden / 32) * B * hidden floats within 256 MiB; rnn.train.cfg's 128 x 1024 is inside"""
    L = darknet.lib()
    # at 128 rows the partials are within 256 MiB while ceil(hidden / 32) * hidden <= 2^28 / (128 * 4) = 524 288: 128 * 4096 is that
    # very number, 129 * 4128 is past it
    table = {(1, 1): 1, (2, 24): 1, (40, 96): 1, (128, 1024): 1, (129, 1024): 0, (128, 4096): 1, (128, 4128): 0, (64, 4128): 1,
             (16, 8192): 1, (128, 8192): 0, (0, 32): 0, (32, 0): 0}
    assert {k: L.y2h_train_rnn_fused_fits(*k) for k in table} == table
    assert L.y2h_train_rnn_fused_ws_bytes(128, 1024) == 32 * 128 * 1024 * 4
