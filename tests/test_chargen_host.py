"""Text generation and scoring without a GPU: the rnn.c entry points are exported and a drop-in caller compiles against
the shim headers; y2_rnn_uniforms is libc's srand / rand stream bit for bit; the numpy statement of the sampling rule
(tests/chargen_rule.py) reproduces what the reference's own sample_array drew in every fixture, and every fixture keeps
its margin claim; read_tokens and the perplexity books; every refusal happens before the device is touched."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet, zoo
from tests.chargen_rule import margin_bar, perplexity, sample_rule
from tests.helpers import load_golden
from tests.test_native_callers import build

CASES = {"chargen_rnn": "rnn", "chargen_gru": "gru", "chargen_rnn_mini": "rnn-mini", "chargen_gru_mini": "gru-mini"}
MINI = ["chargen_gru_mini", "chargen_rnn_mini"]


def scalar(a):
    return np.asarray(a).reshape(-1)[0].item()


def text_of(g):
    """the fixture's characters: the seed, then what the reference generated"""
    return np.concatenate([g["seed"], g["tokens"]]).astype(np.int32)


def test_symbols_and_drop_in_caller(workdir):
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"test_char_rnn", "valid_char_rnn", "vec_char_rnn", "read_tokens", "y2_rnn_uniforms", "y2_rnn_generate",
            "y2_rnn_score", "y2_rnn_perplexity", "y2h_rnn_sample", "y2h_rnn_feed", "y2h_rnn_score"}
    assert want <= have, sorted(want - have)
    build(workdir, "char_rnn_gen", "gcc", "char_rnn_gen.c", ["-Wall", "-Werror"])


@pytest.mark.parametrize("rseed", [0, 1, 8, 12345, 2 ** 31 - 1])
def test_uniforms_are_libc_rand(rseed):
    libc = C.CDLL(None)
    libc.srand.argtypes = [C.c_uint]
    libc.srand(rseed)
    want = np.array([np.float32(libc.rand()) / np.float32(2147483647) for _ in range(64)], np.float32)   # utils.c:610
    got = darknet.Network.rnn_uniforms(rseed, 64)
    assert got.tobytes() == want.tobytes()
    assert (got >= 0).all() and (got <= 1).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_numpy_rule_draws_the_reference_tokens(case):
    g = load_golden(case)
    inputs = zoo.RECURRENT[CASES[case]][0]
    rows = g["rows"][len(g["seed"]) - 1:]
    assert rows.shape == (len(g["tokens"]), g["rows"].shape[1]) and len(g["uniforms"]) == len(g["tokens"])
    assert np.array_equal(g["uniforms"], darknet.Network.rnn_uniforms(scalar(g["rseed"]), len(g["tokens"])))
    for i, (row, u) in enumerate(zip(rows, g["uniforms"])):
        tok, margin = sample_rule(row, u, inputs)
        assert tok == g["tokens"][i], "draw %d" % i
        assert margin == g["margins"][i]


@pytest.mark.parametrize("case", sorted(CASES))
def test_fixture_keeps_its_margin_claim(case):
    g = load_golden(case)
    inputs = zoo.RECURRENT[CASES[case]][0]
    rows = g["rows"][len(g["seed"]) - 1:]
    bars = np.array([margin_bar(r, inputs) for r in rows])
    assert np.array_equal(bars, g["bars"])
    assert scalar(g["claim"]) == int(case in MINI)
    if scalar(g["claim"]):
        assert (g["margins"] >= bars).all(), "smallest margin %.3g, bar %.3g" % (g["margins"].min(), bars.max())
    assert len(g["tokens"]) >= (48 if case in MINI else 32)


def test_read_tokens_round_trip(tmp_path):
    L = darknet.lib()
    L.read_tokens.restype = C.POINTER(C.c_char_p)
    L.read_tokens.argtypes = [C.c_char_p, C.POINTER(C.c_size_t)]
    words = ["the", "a b", "", "x" * 700, "last"]
    p = tmp_path / "tokens.txt"
    p.write_text("\n".join(words) + "\n")
    n = C.c_size_t(0)
    d = L.read_tokens(str(p).encode(), C.byref(n))
    assert n.value == len(words)
    assert [d[i].decode() for i in range(n.value)] == words
    many = tmp_path / "many.txt"                       # more lines than the first allocation (rnn.c:41)
    many.write_text("".join("t%d\n" % i for i in range(1300)))
    d = L.read_tokens(str(many).encode(), C.byref(n))
    assert n.value == 1300 and d[1299] == b"t1299" and d[512] == b"t512"
    assert not L.read_tokens(str(tmp_path / "missing.txt").encode(), C.byref(n))
    assert L.y2_failed_and_clear() and "open" in L.y2_last_error().decode()


@pytest.mark.parametrize("case", MINI)
def test_perplexity_books(case):
    """y2_rnn_perplexity against rnn.c:402-416 evaluated in numpy on the reference's rows.  Both sides round the running
    sum to float per character; were a log to differ by a double ulp between the two, a float rounding of the sum could
    flip: at most one float ulp of the sum per character, so |d sum| <= n * 2^-23 * |sum| and the perplexity
    2^(-sum/n) differs by at most ln 2 * 2^-23 * |sum| relative."""
    g = load_golden(case)
    text = text_of(g)
    p = g["rows"][np.arange(len(text) - 1), text[1:]]
    assert sum(int(c) in (9, 10, 32) for c in text[1:]) > 0, "the text has no word boundary"
    want = perplexity(p, text)
    got = darknet.Network.rnn_perplexity(p, bytes(bytearray(int(c) for c in text)))
    total = abs(sum(math.log2(float(v)) for v in p))
    for a, b in zip(got, want):
        assert abs(a - b) <= (math.log(2) * 2. ** -23 * total + 2. ** -23) * b, (got, want)
    with pytest.raises(darknet.Y2Error):
        darknet.Network.rnn_perplexity(np.zeros(0, np.float32), b"a")


def _parse(tmp, text, name="n.cfg"):
    cfg = os.path.join(str(tmp), name)
    with open(cfg, "w") as f:
        f.write(text)
    return darknet.Network.parse_network_cfg(cfg)


# what is asked -> a word of the message; all of it is refused on the arguments alone
REFUSALS = {
    "no recurrent layer": "recurrent layer",
    "generate with time_steps 8": "time_steps=8",
    "outputs < inputs": "outputs < inputs",
    "seed token >= inputs": "token 30",
    "negative seed token": "token -3",
    "text token >= inputs": "token 31",
    "characters not a multiple of time_steps": "multiple of time_steps",
}


def refusal(tmp, what):
    u = np.zeros(4, np.float32)
    if what == "no recurrent layer":
        net = _parse(tmp, "[net]\nbatch=1\ninputs=8\n\n[connected]\noutput=8\nactivation=linear\n\n[softmax]\n")
        return net, lambda: net.rnn_generate([1], 4, u)
    if what == "generate with time_steps 8":
        net = _parse(tmp, zoo.recurrent_cfg_text("gru-mini", 1, 8))
        return net, lambda: net.rnn_generate([1], 4, u)
    if what == "outputs < inputs":
        net = _parse(tmp, "[net]\nbatch=1\ninputs=8\n\n[gru]\noutput=6\n\n[connected]\noutput=4\nactivation=linear\n\n[softmax]\n")
        return net, lambda: net.rnn_score([1, 2, 3])
    net = _parse(tmp, zoo.recurrent_cfg_text("rnn-mini", 1, 2 if "multiple" in what else 1))
    if what == "seed token >= inputs":
        return net, lambda: net.rnn_generate([7, 30], 4, u)
    if what == "negative seed token":
        return net, lambda: net.rnn_generate([-3], 4, u)
    if what == "text token >= inputs":
        return net, lambda: net.rnn_score([1, 2, 31, 4])
    return net, lambda: net.rnn_score([1, 2, 3, 4])


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_reason(tmp_path, what):
    net, call = refusal(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=REFUSALS[what]):
        call()
    net.free()
