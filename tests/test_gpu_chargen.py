"""Text generation and scoring on the GPU against text the reference's own CPU path generated (tests/golden/
gen_chargen_golden.py): the device sampling kernel is the rule of rnn.c:273-276 / sample_array on the engine's own rows;
strict mode reproduces the reference's characters and rows bit for bit, default mode the characters where the fixture's
margins allow the claim; teacher-forced scoring, perplexity, time_steps > 1, state and batching, and no host round trip
inside the loop."""
from __future__ import annotations

import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests.chargen_rule import perplexity, sample_rule
from tests.helpers import load_golden
from tests.test_chargen_host import CASES, MINI, REFUSALS, refusal, scalar, text_of

pytestmark = pytest.mark.gpu


def _net(tmp, name, B, T, wseed, strict=False, temp=None):
    cfg = os.path.join(str(tmp), "%s_b%d_t%d.cfg" % (name, B, T))
    with open(cfg, "w") as f:
        f.write(zoo.recurrent_cfg_text(name, B, T))
    wts = os.path.join(str(tmp), "%s_s%d.weights" % (name, wseed))
    if not os.path.exists(wts):
        synth.write_recurrent_weights(wts, name, wseed)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(strict)
    if temp is not None:
        net.set_temperature(temp)
    return net


def _case(tmp, case, strict=False, B=1, T=1):
    g = load_golden(case)
    return g, _net(tmp, CASES[case], B, T, scalar(g["wseed"]), strict, scalar(g["temp"]))


def _gen_rows(g):
    """the reference's row each draw sampled from"""
    return g["rows"][len(g["seed"]) - 1:]


def _rows_close(got, ref, what, strict):
    got = np.asarray(got, np.float32).reshape(ref.shape)
    if strict:
        assert np.array_equal(got, ref), "%s: strict mode differs from the reference (max %.3g)" % (what, float(np.abs(got - ref).max()))
        return
    bar = 1e-4 * np.abs(ref).max(axis=-1)
    err = np.abs(got - ref).max(axis=-1)
    assert (err <= bar).all(), "%s: per-row max error %s > %s" % (what, np.array2string(err, precision=3), np.array2string(bar, precision=3))


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_sampling_is_the_rule(tmp_path, case, strict):
    g, net = _case(tmp_path, case, strict)
    inputs = zoo.RECURRENT[CASES[case]][0]
    u = g["uniforms"]
    tokens, rows = net.rnn_generate(g["seed"], len(u), u, probs=True)
    for i in range(len(u)):
        assert sample_rule(rows[i, 0], u[i], inputs)[0] == tokens[i, 0], "draw %d" % i
    if strict:                                  # and the reference's text, the flat full-size rows included
        assert np.array_equal(tokens[:, 0], g["tokens"])
        assert np.array_equal(rows[:, 0], _gen_rows(g))
    net.free()


@pytest.mark.parametrize("case", MINI)
def test_default_mode_reproduces_the_reference_text(tmp_path, case):
    g, net = _case(tmp_path, case)
    assert scalar(g["claim"]) == 1
    tokens, rows = net.rnn_generate(g["seed"], len(g["tokens"]), g["uniforms"], probs=True)
    _rows_close(rows[:, 0], _gen_rows(g), case, False)
    assert np.array_equal(tokens[:, 0], g["tokens"])
    net.free()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_teacher_forced_scoring(tmp_path, case, strict):
    g, net = _case(tmp_path, case, strict)
    text = text_of(g)
    ref = g["rows"]
    p, rows = net.rnn_score(text, probs=True)
    _rows_close(rows[:, 0], ref, case, strict)
    at = np.arange(len(text) - 1)
    assert np.array_equal(p[:, 0], rows[at, 0, text[1:]])
    # perplexity against the reference rows': p_t is within bar_t = 1e-4 * max(row_t) / p_t relative, so the sum of the
    # log2 moves by at most sum(bar_t) / ln 2 and 2^(-sum/count) by at most exp(mean bar_t) - 1 relative (word
    # perplexity: the sum over the words counted); the float sum and result add a few 2^-23
    p_ref = ref[at, text[1:]]
    bar = 1e-4 * ref.max(axis=-1).astype(np.float64) / p_ref
    raw = bytes(bytearray(int(c) for c in text))
    got = net.rnn_perplexity(p, raw)
    want = perplexity(p_ref, text)
    words = 1 + sum(c in b" \n\t" for c in raw[1:])
    assert abs(got[0] - want[0]) <= (np.expm1(bar.mean()) + len(p) * 2. ** -21) * want[0], (got, want)
    if want[1] > float(np.finfo(np.float32).max):         # a flat 256-class text of one word: beyond the float the call returns
        assert got[1] == np.inf
    else:
        assert abs(got[1] - want[1]) <= (np.expm1(bar.sum() / words) + len(p) * 2. ** -21) * want[1], (got, want)
    if strict:
        assert np.array_equal(p[:, 0], p_ref)
    net.free()


@pytest.mark.parametrize("case", MINI + ["chargen_rnn"])
def test_scoring_with_eight_time_steps(tmp_path, case):
    g, one = _case(tmp_path, case)
    g, eight = _case(tmp_path, case, T=8)
    text = text_of(g)
    text = text[:(len(text) - 1) // 8 * 8 + 1]
    p1, r1 = one.rnn_score(text, probs=True)
    p8, r8 = eight.rnn_score(text, probs=True)
    assert "input:" in eight.layer_kernel(0)
    _rows_close(r8[:, 0], g["rows"][:len(text) - 1], case + " time_steps 8", False)
    bar = 1e-4 * np.abs(g["rows"][:len(text) - 1]).max(axis=-1)
    assert (np.abs(r8[:, 0] - r1[:, 0]).max(axis=-1) <= bar).all()
    assert (np.abs(p8 - p1)[:, 0] <= bar).all()
    with pytest.raises(darknet.Y2Error, match="time_steps=8"):
        eight.rnn_generate(g["seed"], 4, g["uniforms"][:4])
    one.free(); eight.free()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", MINI)
def test_two_calls_continue_and_reset_restarts(tmp_path, case, graph):
    g, whole = _case(tmp_path, case)
    g, parts = _case(tmp_path, case)
    parts.set_graph(graph)
    u, N = g["uniforms"], len(g["uniforms"])
    full = whole.rnn_generate(g["seed"], N, u)
    a, ra = parts.rnn_generate(g["seed"], N // 2, u[:N // 2], probs=True)
    b = parts.rnn_generate(a[-1], N - N // 2, u[N // 2:])
    assert np.array_equal(np.concatenate([a, b]), full)
    again, rb = parts.rnn_generate(g["seed"], N // 2, u[:N // 2], probs=True)
    assert not np.array_equal(ra, rb), "the second run did not go on from the state the first left"
    parts.reset_rnn_state(-1)
    again, rb = parts.rnn_generate(g["seed"], N // 2, u[:N // 2], probs=True)
    assert np.array_equal(again, a) and np.array_equal(ra, rb), "reset_rnn_state did not restart the sequence"
    whole.free(); parts.free()


@pytest.mark.parametrize("case", MINI)
def test_three_sequences_are_three_runs(tmp_path, case):
    g, three = _case(tmp_path, case, strict=True, B=3)
    N = 16
    seed = np.stack([g["seed"] + b for b in range(3)], axis=1)                     # [len][3]
    u = np.stack([darknet.Network.rnn_uniforms(scalar(g["rseed"]) + b, N) for b in range(3)], axis=1)
    tokens, rows = three.rnn_generate(seed, N, u, probs=True)
    for b in range(3):
        g, one = _case(tmp_path, case, strict=True)
        t1, r1 = one.rnn_generate(seed[:, b], N, u[:, b], probs=True)
        assert np.array_equal(t1[:, 0], tokens[:, b]) and np.array_equal(r1[:, 0], rows[:, b]), "sequence %d" % b
        one.free()
    assert len({tuple(tokens[:, b]) for b in range(3)}) == 3
    three.free()


@pytest.mark.parametrize("case", MINI)
def test_predict_goes_on_from_the_loop(tmp_path, case):
    g, a = _case(tmp_path, case)
    g, b = _case(tmp_path, case)
    u = g["uniforms"]
    ta = a.rnn_generate(g["seed"], 8, u[:8])
    tb, rows = b.rnn_generate(g["seed"], 9, u[:9], probs=True)
    assert np.array_equal(ta, tb[:8])
    x = np.zeros(zoo.RECURRENT[CASES[case]][0], np.float32)
    x[ta[-1, 0]] = 1
    assert np.array_equal(a.network_predict(x), rows[8, 0])
    a.free(); b.free()


def test_no_host_round_trip_inside_the_loop(tmp_path):
    g, net = _case(tmp_path, "chargen_gru_mini")
    L = darknet.lib()
    L.y2h_rnn_sample_launches.restype = C_ulong
    L.y2h_d2h_copies.restype = C_ulong
    u = g["uniforms"]
    net.rnn_generate(g["seed"], 2, u[:2])              # the plan is built
    copies = []
    for n in (8, 40):
        s0, c0 = L.y2h_rnn_sample_launches(), L.y2h_d2h_copies()
        net.rnn_generate(g["seed"], n, u[:n])
        assert L.y2h_rnn_sample_launches() - s0 == n, "one sampling launch per character"
        copies.append(L.y2h_d2h_copies() - c0)
    assert copies[0] == copies[1] == 1, copies         # the tokens, once
    c0 = L.y2h_d2h_copies()
    net.rnn_score(text_of(g))
    assert L.y2h_d2h_copies() - c0 == 1
    net.free()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_on_the_gpu(tmp_path, what):
    net, call = refusal(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=REFUSALS[what]):
        call()
    net.free()


def test_modes_work(tmp_path):
    """fusion off, timing on and a recorded graph generate the same text as the plain run; fp16 stays refused"""
    g, plain = _case(tmp_path, "chargen_rnn_mini")
    u = g["uniforms"][:12]
    want = plain.rnn_generate(g["seed"], 12, u)
    for mode in ("fusion", "timing", "graph"):
        g, net = _case(tmp_path, "chargen_rnn_mini")
        {"fusion": lambda: net.set_fusion(False), "timing": lambda: net.set_timing(True), "graph": lambda: net.set_graph(True)}[mode]()
        assert np.array_equal(net.rnn_generate(g["seed"], 12, u), want), mode
        net.free()
    g, net = _case(tmp_path, "chargen_rnn_mini")
    net.set_half(True)
    with pytest.raises(darknet.Y2Error, match="half"):
        net.rnn_generate(g["seed"], 12, u)
    net.free(); plain.free()


from ctypes import c_ulong as C_ulong  # noqa: E402
