"""The [rnn] / [gru] layers of the reference (rnn_layer.c:83-122, gru_layer.c:118-192 over connected_layer.c:122-155) in
numpy fp32, in the reference's own operation order, every product and sum rounded on its own.  tests/test_rec_rule_host.py
pins it bit for bit on every recurrent fixture the reference's compiled CPU path wrote (tests/golden/gen_rnn_golden.py);
the GPU tests apply it to shapes and row counts no fixture has.  Plain numpy: nothing of the engine is imported.

Two statements of the batch-norm divide live here.  The networks' (`epilogue` with var) is the reference's: a division by
sqrt(var) + .000001f in double.  The step kernel's contract (include/y2_hip.h, y2h_rec_args.rinv) is a product with a
reciprocal handed in (`epilogue` with rinv); the two can differ by an fp32 ulp."""
from __future__ import annotations

import math
import struct

import numpy as np

F = np.float32
DENSE, RNN, GRU_ZR, GRU_H = 0, 1, 2, 3            # include/y2_hip.h Y2H_REC_*
ACT = {"linear": 0, "leaky": 1, "logistic": 2, "relu": 3, "tanh": 6, "loggy": 9}      # include/y2_hip.h Y2H_ACT_*
TRANSCENDENTAL = ("logistic", "tanh", "loggy")


def _exp(v):
    """libm's exp on every value of a float64 array (math.exp is the C library's, as the reference binary calls it)"""
    def one(t):
        try:
            return math.exp(t)
        except OverflowError:
            return math.inf
    flat = np.asarray(v, np.float64).reshape(-1)
    return np.array([one(t) for t in flat.tolist()], np.float64).reshape(np.shape(v))


def dense(x, w):
    """gemm_nt (gemm.c:90-106) with C = 0: out[r][j] = 0 + sum_q x[r][q] * w[j][q], fp32 products summed ascending in q"""
    x = np.asarray(x, F)
    w = np.asarray(w, F)
    x = x.reshape(-1, w.shape[1])
    out = np.empty((x.shape[0], w.shape[0]), F)
    for r in range(x.shape[0]):
        out[r] = np.cumsum(w * x[r], axis=1, dtype=F)[:, -1]
    return (F(0) + out).astype(F)


def activate(v, act):
    """activations.h:34-42 on fp32 values: the double expressions of the reference, rounded to float once"""
    v = np.asarray(v, F)
    d = v.astype(np.float64)
    with np.errstate(all="ignore"):
        if act == "linear":
            return v.copy()
        if act == "leaky":
            return np.where(v > 0, v, (.1 * d).astype(F)).astype(F)
        if act == "relu":
            return (v * (v > 0).astype(F)).astype(F)
        if act == "logistic":
            return (1. / (1. + _exp(-d))).astype(F)
        if act == "loggy":
            return (2. / (1. + _exp(-d)) - 1).astype(F)
        if act == "tanh":
            e = _exp((F(2) * v).astype(F).astype(np.float64))         # exp(2*x): the product in float
            return ((e - 1) / (e + 1)).astype(F)
    raise ValueError(act)


def sigma(v):
    return activate(v, "logistic")


def epilogue(v, rec, act, rinv=None):
    """forward_connected_layer after the gemm: batch-norm on the rolling statistics (normalize_cpu blas.c:122, scale_bias),
    bias, activation.  rec: dict with "bias" and, with batch-norm, "scale", "mean" and "var".  With `rinv` (float64, one
    per column) the divide is the step kernel's contract instead: v = (float)((double)(v - mean) * rinv)"""
    v = np.asarray(v, F)
    if rec.get("scale") is not None:
        d = (v - rec["mean"]).astype(F).astype(np.float64)
        if rinv is None:
            v = (d / (np.sqrt(rec["var"].astype(np.float64)) + np.float64(F(.000001)))).astype(F)
        else:
            v = (d * np.asarray(rinv, np.float64)).astype(F)
        v = (v * rec["scale"]).astype(F)
    v = (v + rec["bias"]).astype(F)
    return activate(v, act)


def connected(x, rec, act):
    return epilogue(dense(x, rec["w"]), rec, act)


def rnn_combine(v, proj, state, shortcut):
    """rnn_layer.c:104-112: fill / copy, axpy(input), axpy(self)"""
    base = np.asarray(state, F) if shortcut else np.zeros_like(v)
    return ((base + np.asarray(proj, F)).astype(F) + v).astype(F)


def gru_combine(z, state, hh):
    """weighted_sum_cpu (blas.c:49-55): z*state + (1-z)*h"""
    z = np.asarray(z, F)
    return ((z * state).astype(F) + ((F(1) - z).astype(F) * hh).astype(F)).astype(F)


def rnn_forward(recs, x, B, T, act, logistic, shortcut, state=None):
    """one [rnn] layer over step-major rows x[T*B][inputs]; recs = (input, self, output).  Returns (out[T*B][outputs],
    the state after the last step)"""
    rin, rself, rout = recs
    self_act = "loggy" if logistic == 2 else ("logistic" if logistic == 1 else act)
    state = np.zeros((B, rself["w"].shape[0]), F) if state is None else state
    proj = connected(x, rin, act)                               # every step's input product: rows do not interact
    out = []
    for t in range(T):
        state = rnn_combine(connected(state, rself, self_act), proj[t * B:(t + 1) * B], state, shortcut)
        out.append(connected(state, rout, act))
    return np.concatenate(out), state


def gru_forward(recs, x, B, T, state=None):
    """one [gru] layer; recs = (input z, r, h, state z, r, h), all linear.  Returns (out[T*B][outputs], the last state)"""
    iz, ir, ih, sz, sr, sh = recs
    state = np.zeros((B, sz["w"].shape[0]), F) if state is None else state
    pz, pr, ph = (connected(x, r, "linear") for r in (iz, ir, ih))
    out = []
    for t in range(T):
        rows = slice(t * B, (t + 1) * B)
        z = sigma((pz[rows] + connected(state, sz, "linear")).astype(F))
        r = sigma((pr[rows] + connected(state, sr, "linear")).astype(F))
        f = (state * r).astype(F)
        hh = sigma((ph[rows] + connected(f, sh, "linear")).astype(F))
        state = gru_combine(z, state, hh)
        out.append(state)
    return np.concatenate(out), state


def read_records(path, shapes):
    """the [connected] records of a synth.write_recurrent_weights file; shapes = zoo.recurrent_records(name)"""
    with open(path, "rb") as f:
        raw = f.read()
    assert struct.unpack_from("<iii", raw, 0) == (0, 1, 0)
    at = 16                                                     # major, minor, revision, seen (parser.c:1022-1029)
    recs = []

    def take(n):
        nonlocal at
        a = np.frombuffer(raw, "<f4", n, at).astype(F)
        at += 4 * n
        return a

    for n, k, bn in shapes:
        rec = {"bias": take(n), "w": take(n * k).reshape(n, k), "scale": None}
        if bn:
            rec["scale"], rec["mean"], rec["var"] = take(n), take(n), take(n)
        recs.append(rec)
    assert at == len(raw), "the file holds %d bytes beyond its records" % (len(raw) - at)
    return recs


def network_forward(name, records, x, B, T):
    """the zoo.RECURRENT network `name` (the table of layer shapes only: no engine code) up to and including its
    [connected] layer.  Returns (the [connected] layer's output [T*B][n], each recurrent layer's output [T*B][outputs])"""
    from sr_object_detection_amd import zoo
    layers = zoo.RECURRENT[name][1]
    x = np.asarray(x, F).reshape(B * T, -1)
    at = 0
    per_layer = []
    for e in layers:
        if e[0] == "rnn":
            x, _ = rnn_forward(records[at:at + 3], x, B, T, e[3], e[5], e[6])
            at += 3
            per_layer.append(x)
        elif e[0] == "gru":
            x, _ = gru_forward(records[at:at + 6], x, B, T)
            at += 6
            per_layer.append(x)
        elif e[0] == "connected":
            return connected(x, records[at], e[2]), per_layer
    raise ValueError("no [connected] layer")


# ---- one y2h_rec_step launch (include/y2_hip.h): the dense product, the epilogue with rinv handed in, the mode's combine

def step_value(a):
    """the value v a launch combines: `pre` as it is, else the epilogue of the dense product"""
    if a.get("pre") is not None:
        return np.asarray(a["pre"], F)
    return epilogue(dense(a["x"], a["w"]), a, a["act"], a.get("rinv"))


def step_dense(a):
    return step_value(a)


def step_rnn(a):
    return rnn_combine(step_value(a), a["proj"], a["state"], a["shortcut"])


def step_gru_zr(a):
    """(z [rows][h], f = state * r [rows][h]); proj is [rows][3h] = z | r | h"""
    h = a["h"]
    v = step_value(a)
    z = sigma((a["proj"][:, :h] + v[:, :h]).astype(F))
    r = sigma((a["proj"][:, h:2 * h] + v[:, h:]).astype(F))
    return z, (a["state"] * r).astype(F)


def step_gru_h(a):
    h = a["h"]
    hh = sigma((a["proj"][:, 2 * h:] + step_value(a)).astype(F))
    return gru_combine(a["z"], a["state"], hh)


def ulps(a, b):
    """distance in fp32 units in the last place between two finite arrays of one sign pattern"""
    ia = np.asarray(a, F).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
