"""[rnn] / [gru] on the GPU against the reference's own CPU path (tests/golden/gen_rnn_golden.py): every output row and
every dumped layer within 1e-4 of the largest reference value, bit for bit in strict mode; the hidden state carries
from one call to the next (one step per call, two 8-step calls against one 16-step reference call, graph replay), and
reset_rnn_state restarts one sequence only."""
from __future__ import annotations

import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

CASES = {"rnn_ref_b2_t8": "rnn", "gru_ref_b2_t8": "gru", "rnn_mini_b3_t16": "rnn-mini", "gru_mini_b3_t16": "gru-mini",
         # the step kernel's other row counts: 4 and 8 rows in full, 5 of 8, 9 (the first count past the skinny kernel)
         "rnn_mini_b4_t2": "rnn-mini", "gru_mini_b5_t3": "gru-mini", "rnn_mini_b8_t2": "rnn-mini", "gru_mini_b9_t2": "gru-mini",
         "gru_ref_b8_t2": "gru", "rnn_ref_b5_t2": "rnn"}
MINI = ["rnn_mini_b3_t16", "gru_mini_b3_t16"]              # the 16-step cases
COST = 9
RECURRENT = (15, 16)                                        # LAYER_TYPES: RNN, GRU
SKINNY_ROWS = 8


def _net(tmp, name, B, T, wseed, strict=False):
    cfg = os.path.join(str(tmp), "%s_b%d_t%d.cfg" % (name, B, T))
    with open(cfg, "w") as f:
        f.write(zoo.recurrent_cfg_text(name, B, T))
    wts = os.path.join(str(tmp), "%s_s%d.weights" % (name, wseed))
    if not os.path.exists(wts):
        synth.write_recurrent_weights(wts, name, wseed)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(strict)
    return net


def _golden(case):
    g = load_golden(case)
    B, T = (int(v) for v in g["bt"])
    return g, B, T, int(g["seeds"][0])


def _close(got, ref, what, strict):
    got = np.asarray(got, np.float32).reshape(ref.shape)
    if strict:
        assert np.array_equal(got, ref), "%s: strict mode differs from the reference (max %.3g)" % (what, float(np.abs(got - ref).max()))
        return
    bar = 1e-4 * float(np.abs(ref).max())
    err = np.abs(got - ref).max(axis=-1)
    assert float(err.max()) <= bar, "%s: per-row max error %s > %.3g" % (what, np.array2string(err, precision=3), bar)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_golden(tmp_path, case, strict):
    g, B, T, ws = _golden(case)
    net = _net(tmp_path, CASES[case], B, T, ws, strict)
    out = net.network_predict(g["x"])
    _close(out, g["out"], case + " output", strict)
    for i in range(net.n):
        key = "layer_%02d" % i
        l = net.layer(i)
        if l.type in RECURRENT and not strict:                  # the plan's choice: the skinny kernel while the rows fit it
            name = net.layer_kernel(i)
            assert ("step:skinny" in name) if B <= SKINNY_ROWS else ("skinny" not in name), name
        if key not in g or l.type == COST:
            continue
        got = net.pull_layer_output(i).reshape(B * T, -1)
        ref = g[key].reshape(-1, got.shape[1])
        _close(got[:ref.shape[0]], ref, "%s layer %d (%s)" % (case, i, net.layer_kernel(i)), strict)   # the reference dumps step 0
    net.free()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_step_per_call(tmp_path, case, strict):
    g, B, T, ws = _golden(case)
    net = _net(tmp_path, CASES[case], B, 1, ws, strict)
    for t in range(T):
        out = net.network_predict(g["x"][t * B:(t + 1) * B])
        if not strict:                                          # at T = 1 the hoisted products have B rows as well
            name = net.layer_kernel(0)
            assert name.count("skinny") == (3 if B <= SKINNY_ROWS else 0), name      # the layer's three blocks
        _close(out, g["out"][t * B:(t + 1) * B], "%s step %d" % (case, t), strict)
    net.free()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("case", MINI)
def test_two_calls_of_eight_steps(tmp_path, case, strict):
    g, B, T, ws = _golden(case)
    net = _net(tmp_path, CASES[case], B, T // 2, ws, strict)
    half = B * T // 2
    a = net.network_predict(g["x"][:half])
    b = net.network_predict(g["x"][half:])
    _close(np.concatenate([a, b]), g["out"], case + " 2 x 8 steps", strict)
    net.free()


@pytest.mark.parametrize("case", MINI)
def test_reset_one_item(tmp_path, case):
    g, B, T, ws = _golden(case)
    ref = _net(tmp_path, CASES[case], B, 1, ws, True)
    full = [ref.network_predict(g["x"][t * B:(t + 1) * B]).reshape(B, -1) for t in range(9)]
    net = _net(tmp_path, CASES[case], B, 1, ws, True)
    for t in range(5):
        net.network_predict(g["x"][t * B:(t + 1) * B])
    net.reset_rnn_state(1)
    for t in range(5, 9):
        x = g["x"][t * B:(t + 1) * B].copy()
        x[1] = g["x"][(t - 5) * B + 1]                       # item 1 starts its sequence again
        out = net.network_predict(x).reshape(B, -1)
        assert np.array_equal(out[[0, 2]], full[t][[0, 2]]), "step %d: the other items did not continue" % t
        assert np.array_equal(out[1], full[t - 5][1]), "step %d: item 1 did not restart as on a fresh network" % t
    with pytest.raises(darknet.Y2Error):
        net.reset_rnn_state(B)
    ref.free(); net.free()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("case", ["rnn_ref_b2_t8"] + MINI)
def test_graph_replay_keeps_the_state(tmp_path, case, T):
    g, B, _, ws = _golden(case)
    eager = _net(tmp_path, CASES[case], B, T, ws)
    graph = _net(tmp_path, CASES[case], B, T, ws)
    graph.set_graph(True)
    for c in range(4):
        x = g["x"][(c % 2) * B * T:(c % 2 + 1) * B * T]
        assert np.array_equal(graph.network_predict(x), eager.network_predict(x)), "call %d differs under graph replay" % c
    eager.free(); graph.free()


@pytest.mark.parametrize("case", MINI + ["rnn_mini_b8_t2"])     # 8 sequences: sequence 7 is the last accumulator of MB = 8
def test_items_are_independent(tmp_path, case):
    g, B, T, ws = _golden(case)
    for strict in (True, False):
        both = _net(tmp_path, CASES[case], B, T, ws, strict).network_predict(g["x"]).reshape(T, B, -1)
        for b in range(B):
            one = _net(tmp_path, CASES[case], 1, T, ws, strict).network_predict(g["x"].reshape(T, B, -1)[:, b]).reshape(T, -1)
            if strict:
                assert np.array_equal(one, both[:, b]), "item %d differs from a batch-1 run" % b
            else:
                _close(one, both[:, b], "item %d" % b, False)


@pytest.mark.parametrize("form", ["skinny", "mfma"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_forms(tmp_path, monkeypatch, case, form):
    g, B, T, ws = _golden(case)
    monkeypatch.setenv("Y2_RNN_STEP", form)
    net = _net(tmp_path, CASES[case], B, T, ws)
    if form == "skinny" and B > SKINNY_ROWS:                    # a forced skinny step that does not fit is refused
        with pytest.raises(darknet.Y2Error, match="skinny"):
            net.network_predict(g["x"])
        net.free()
        return
    out = net.network_predict(g["x"])
    # the name says what runs: the matrix-core kernels do not take the mini nets' 30- / 36-wide rows, which then run on
    # the reference-order kernel
    ran = form if (form == "skinny" or "_ref_" in case) else "ref"
    assert ("step:%s" % ran) in net.layer_kernel(0), net.layer_kernel(0)
    _close(out, g["out"], "%s step form %s" % (case, form), False)
    net.free()


def test_forced_skinny_that_does_not_fit_is_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("Y2_RNN_STEP", "skinny")
    net = _net(tmp_path, "rnn", 32, 1, 201)
    with pytest.raises(darknet.Y2Error, match="skinny"):
        net.network_predict(np.zeros(32 * 256, np.float32))
    net.free()


def test_temperature_between_calls(tmp_path):
    g, B, T, ws = _golden("gru_mini_b3_t16")
    a = _net(tmp_path, "gru-mini", B, 1, ws)
    b = _net(tmp_path, "gru-mini", B, 1, ws)
    a.set_graph(True); b.set_graph(True)
    x0, x1 = g["x"][:B], g["x"][B:2 * B]
    a.network_predict(x0)
    b.set_temperature(.5)
    b.network_predict(x0)
    a.set_temperature(.5)                 # written between calls: the next call uses it
    assert np.array_equal(a.network_predict(x1), b.network_predict(x1))
    a.set_temperature(1.)
    assert not np.array_equal(a.network_predict(x1), b.network_predict(x1))
    a.free(); b.free()


def test_fp16_is_refused(tmp_path):
    net = _net(tmp_path, "gru-mini", 3, 1, 231)
    net.set_half(True)
    with pytest.raises(darknet.Y2Error, match="half"):
        net.network_predict(np.zeros(3 * 30, np.float32))
    net.free()


def test_resize_is_refused(tmp_path):
    net = _net(tmp_path, "rnn-mini", 3, 1, 221)
    with pytest.raises(darknet.Y2Error, match="resize"):
        net.resize_network(32, 32)
    net.free()


@pytest.mark.parametrize("case", ["rnn_ref_b2_t8", "gru_ref_b2_t8"])
def test_two_fresh_runs_are_bitwise_equal(tmp_path, case):
    g, B, T, ws = _golden(case)
    a = _net(tmp_path, CASES[case], B, T, ws).network_predict(g["x"])
    b = _net(tmp_path, CASES[case], B, T, ws).network_predict(g["x"])
    assert np.array_equal(a, b)


def test_set_batch_zeroes_the_state(tmp_path):
    g, B, T, ws = _golden("rnn_mini_b3_t16")
    net = _net(tmp_path, "rnn-mini", B, 1, ws, True)
    first = net.network_predict(g["x"][:B])
    net.network_predict(g["x"][B:2 * B])
    net.set_batch_network(B)
    assert np.array_equal(net.network_predict(g["x"][:B]), first)
    net.free()


def test_rnn_train_shape(tmp_path):
    """rnn.train.cfg's shape: 128 sequences x 576 steps in one forward (matrix-core step form, 73 728 hoisted rows);
    sequences 0 and 127 over their first 16 steps equal a 2-sequence, 16-step run of the same rows"""
    B, T = 128, 576
    big = _net(tmp_path, "rnn", B, T, 201)
    x = synth.char_rows(401, B, T, 256, True)
    out = big.network_predict(x).reshape(T, B, -1)
    assert "step:mfma" in big.layer_kernel(0), big.layer_kernel(0)
    assert np.isfinite(out).all()
    big.free()
    small = _net(tmp_path, "rnn", 2, 16, 201)
    xs = x.reshape(T, B, -1)[:16][:, [0, B - 1]]
    ref = small.network_predict(xs).reshape(16, 2, -1)
    _close(out[:16][:, [0, B - 1]].reshape(32, -1), ref.reshape(32, -1), "rnn.train shape, sequences 0 and 127", False)
    small.free()

