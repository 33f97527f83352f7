"""The numpy statement of the recurrent layers (tests/rec_rule.py) against what the reference's own compiled CPU path wrote:
for every recurrent fixture of tests/golden/ the [connected] layer's dump -- every row, so every step of every recurrent
layer feeds it -- bit for bit, and each recurrent layer's own dump (step 0).  If this fails the rule is wrong."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import rec_rule
from tests.helpers import GOLDEN, load_golden
from tests.test_native_callers import build

NETS = {"rnn_ref": "rnn", "gru_ref": "gru", "rnn_mini": "rnn-mini", "gru_mini": "gru-mini"}
FIXTURES = sorted(os.path.basename(p)[:-4] for k in NETS for p in glob.glob(os.path.join(GOLDEN, k + "_b*_t*.npz")))


def test_every_row_count_has_a_fixture():
    have = {(NETS[f[:f.index("_b")]], int(load_golden(f)["bt"][0])) for f in FIXTURES}
    assert len(FIXTURES) == 10, FIXTURES
    assert {("rnn-mini", 4), ("gru-mini", 5), ("rnn-mini", 8), ("gru-mini", 9), ("gru", 8), ("rnn", 5)} <= have


@pytest.mark.parametrize("case", FIXTURES)
def test_rule_is_the_reference_bit_for_bit(tmp_path, case):
    g = load_golden(case)
    name = NETS[case[:case.index("_b")]]
    B, T = (int(v) for v in g["bt"])
    wts = str(tmp_path / "net.weights")
    synth.write_recurrent_weights(wts, name, int(g["seeds"][0]))
    records = rec_rule.read_records(wts, zoo.recurrent_records(name))
    layers = zoo.RECURRENT[name][1]
    out, per_layer = rec_rule.network_forward(name, records, g["x"], B, T)
    at = [e[0] for e in layers].index("connected")
    ref = g["layer_%02d" % at].reshape(B * T, -1)
    assert out.shape == ref.shape
    assert np.array_equal(out, ref), "%s [connected]: %d of %d values differ, max %.3g" % (
        case, int((out != ref).sum()), ref.size, float(np.abs(out - ref).max()))
    for i, got in enumerate(per_layer):                         # the reference dumps step 0 of a recurrent layer
        ref = g["layer_%02d" % i].reshape(B, -1)
        assert np.array_equal(got[:B], ref), "%s layer %d (%s), step 0" % (case, i, layers[i][0])


def test_kernel_rule_divide_is_the_header_contract():
    """epilogue with rinv handed in is a product, with var a division: equal where rinv is a power of two"""
    v = np.array([[3., -7., 11.]], np.float32)
    rec = {"bias": np.zeros(3, np.float32), "scale": np.array([1, -2, 3], np.float32), "mean": np.array([1, 2, -3], np.float32),
           "var": np.array([4, 16, .25], np.float32)}
    rinv = 1. / (np.sqrt(rec["var"].astype(np.float64)) + np.float64(np.float32(.000001)))
    a = rec_rule.epilogue(v, rec, "linear")
    b = rec_rule.epilogue(v, rec, "linear", rinv)
    assert rec_rule.ulps(a, b).max() <= 1
    exact = rec_rule.epilogue(v, rec, "linear", np.array([.5, .25, 2.]))
    assert np.array_equal(exact, np.array([[1., 4.5, 84.]], np.float32))


def test_ctypes_mirror_of_rec_args_is_the_c_struct(workdir):
    exe = build(workdir, "rec_args_layout", "gcc", "rec_args_layout.c", ["-Wall", "-Werror"])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    want = dict(l.split(" ", 1) for l in lines if l)
    assert int(want.pop("sizeof")) == C.sizeof(darknet.RecArgs)
    assert want.pop("enums").split() == [str(v) for v in (
        darknet.REC_DENSE, darknet.REC_RNN, darknet.REC_GRU_ZR, darknet.REC_GRU_H, darknet.REC_REF, darknet.REC_SKINNY,
        darknet.REC_SKINNY_MAX_ROWS)]
    assert [n for n, _ in darknet.RecArgs._fields_] == list(want)           # the same fields in the same order
    for name, off in want.items():
        assert getattr(darknet.RecArgs, name).offset == int(off), name
    assert (rec_rule.DENSE, rec_rule.RNN, rec_rule.GRU_ZR, rec_rule.GRU_H) == (
        darknet.REC_DENSE, darknet.REC_RNN, darknet.REC_GRU_ZR, darknet.REC_GRU_H)
