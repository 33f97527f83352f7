"""A drop-in C user of the reference's rnn.c entry points (tests/native/char_rnn_gen.c, compiled against include/ with the
reference's header names): test_char_rnn with rseed and a token file prints exactly the text the reference generated
(strict mode), valid_char_rnn prints the reference's perplexity lines, vec_char_rnn layer 0's vector per line."""
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests.chargen_rule import perplexity
from tests.helpers import load_golden
from tests.test_chargen_host import CASES, scalar, text_of
from tests.test_native_callers import build

pytestmark = pytest.mark.gpu


def _files(workdir, case):
    g = load_golden(case)
    name = CASES[case]
    cfg = os.path.join(workdir, case + ".cfg")
    with open(cfg, "w") as f:
        f.write(zoo.recurrent_cfg_text(name, 1, 1))
    wts = os.path.join(workdir, "%s_s%d.weights" % (name, scalar(g["wseed"])))
    if not os.path.exists(wts):
        synth.write_recurrent_weights(wts, name, scalar(g["wseed"]))
    return g, cfg, wts


@pytest.mark.parametrize("case", sorted(CASES))
def test_test_char_rnn_prints_the_reference_text(workdir, case):
    g, cfg, wts = _files(workdir, case)
    words = os.path.join(workdir, case + ".tokens")
    with open(words, "w") as f:
        f.write("".join("w%d\n" % i for i in range(zoo.RECURRENT[CASES[case]][0])))
    exe = build(workdir, "char_rnn_gen", "gcc", "char_rnn_gen.c")
    seed = bytes(bytearray(int(c) for c in g["seed"]))
    r = subprocess.run([exe, "test", cfg, wts, str(len(g["tokens"])), seed, repr(float(scalar(g["temp"]))), str(scalar(g["rseed"])), words],
                       env=dict(os.environ, Y2_STRICT="1"), check=True, timeout=300, capture_output=True)
    assert r.stdout.decode() == "".join("w%d " % c for c in text_of(g)) + "\n"


def test_valid_char_rnn_prints_the_reference_perplexity(workdir):
    g, cfg, wts = _files(workdir, "chargen_gru_mini")
    text = text_of(g)
    exe = build(workdir, "char_rnn_gen", "gcc", "char_rnn_gen.c")
    # test_char_rnn's temperature is not valid_char_rnn's: the cfg's own (1) applies, so the rows are the engine's own
    # strict rows, which test_gpu_rnn.py pins on the reference
    r = subprocess.run([exe, "valid", cfg, wts, ""], input=bytes(bytearray(int(c) for c in text)),
                       env=dict(os.environ, Y2_STRICT="1"), check=True, timeout=300, capture_output=True)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    p = net.rnn_score(text)[:, 0]
    net.free()
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(text) - 1
    for i in (0, len(p) // 2, len(p) - 1):
        a, b = perplexity(p[:i + 1], text[:i + 2])
        assert lines[i] == "%d Perplexity: %4.4f    Word Perplexity: %4.4f" % (i + 1, a, b)


def test_vec_char_rnn_prints_layer_zero(workdir):
    g, cfg, wts = _files(workdir, "chargen_rnn")
    exe = build(workdir, "char_rnn_gen", "gcc", "char_rnn_gen.c")
    r = subprocess.run([exe, "vec", cfg, wts, "ab"], input=b"hello\n  second line \n", env=dict(os.environ, Y2_STRICT="1"),
                       check=True, timeout=300, capture_output=True)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 2
    for line, text in zip(lines, ["hello", "secondline"]):       # strip (utils.c) drops every blank
        net.reset_rnn_state(0)
        net.rnn_score(np.frombuffer(("ab" + text + " \0").encode(), np.uint8).astype(np.int32))
        v = net.pull_layer_output(0)
        assert line == text + "".join(",%g" % x for x in v)
    net.free()


def test_long_runs_go_in_chunks(workdir):
    """more characters than one chunk of the wrappers (256 generated, 1024 scored): the text and the books go on across
    the chunk boundaries exactly as one call of the API does"""
    g, cfg, wts = _files(workdir, "chargen_gru_mini")
    exe = build(workdir, "char_rnn_gen", "gcc", "char_rnn_gen.c")
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_temperature(.5)
    seed = bytes(bytearray(int(c) for c in g["seed"]))
    r = subprocess.run([exe, "test", cfg, wts, "600", seed, "0.5", "3"], check=True, timeout=300, capture_output=True)
    tokens = net.rnn_generate(g["seed"], 600, net.rnn_uniforms(3, 600))[:, 0]
    assert r.stdout == seed + bytes(bytearray(int(c) for c in tokens)) + b"\n"
    text = np.concatenate([g["seed"], tokens[:2500 - 2]]).astype(np.int32)
    text = np.resize(text, 2500)
    r = subprocess.run([exe, "valid", cfg, wts, ""], input=bytes(bytearray(int(c) for c in text)), check=True, timeout=300,
                       capture_output=True)
    net.set_temperature(1.)
    net.reset_rnn_state(-1)
    p = net.rnn_score(text)[:, 0]
    net.free()
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(text) - 1
    for i in (1023, 1024, 2047, 2048, len(p) - 1):
        a, b = perplexity(p[:i + 1], text[:i + 2])
        assert lines[i] == "%d Perplexity: %4.4f    Word Perplexity: %4.4f" % (i + 1, a, b)
