"""What [normalization] and [activation] compute, restated in numpy (normalization_layer.c:65-94, activations.h:21-54).

lrn_sequential walks the channels in the reference's order with its float32 steps and is bit-equal to the compiled
reference; lrn_closed is the closed form the one-pass device kernel evaluates.  Both take [..., c] arrays (channels last)
or, with axis=, any layout.  exp and pow go through libm one value at a time (math.exp / math.pow): numpy's vector exp
need not round like the C library the reference links."""
from __future__ import annotations

import math

import numpy as np

F = np.float32

ACTIVATIONS = ["linear", "leaky", "logistic", "relu", "relie", "ramp", "tanh", "plse", "elu", "loggy", "stair", "hardtan", "lhtan"]
# include/y2_hip.h Y2H_ACT_*: the device code of each name
ACT_CODE = {n: i for i, n in enumerate(ACTIVATIONS)}


def _pow_f32(norms: np.ndarray, beta: float) -> np.ndarray:
    """(float)pow((double)norm, -(double)(float)beta), NaN where libm says so"""
    e = -float(F(beta))
    out = np.empty(norms.shape, F)
    flat, o = norms.reshape(-1), out.reshape(-1)
    for i, v in enumerate(flat.tolist()):
        try:
            o[i] = F(math.pow(v, e))
        except (ValueError, ZeroDivisionError, OverflowError):
            o[i] = F(np.nan) if v < 0 else F(np.inf)
    return out


def lrn_sequential(x: np.ndarray, size: int, alpha: float, beta: float, kappa: float, axis: int = -1) -> np.ndarray:
    x = np.moveaxis(np.asarray(x, F), axis, 0)
    c = x.shape[0]
    a = F(alpha)
    sq = x * x
    norms = np.empty_like(x)
    n = np.full(x.shape[1:], F(kappa), F)
    for k in range(size // 2):
        n = n + a * sq[k]
    norms[0] = n
    for k in range(1, c):
        prev, nxt = k - (size - 1) // 2 - 1, k + size // 2
        if prev >= 0:
            n = n + (-a) * sq[prev]
        if nxt < c:
            n = n + a * sq[nxt]
        norms[k] = n
    with np.errstate(invalid="ignore", over="ignore"):
        out = _pow_f32(norms, beta) * x
    return np.moveaxis(out, 0, axis)


def lrn_norms_closed(x: np.ndarray, size: int, alpha: float, kappa: float) -> np.ndarray:
    """kappa + alpha * (sum over the window, ascending, - sq[size/2]) in float32 steps; channels first"""
    c = x.shape[0]
    sq = x * x
    zero = np.zeros(x.shape[1:], F)
    gone = sq[size // 2] if size // 2 < c else zero
    norms = np.empty_like(x)
    for k in range(c):
        s = zero
        for j in range(max(0, k - (size - 1) // 2), min(c - 1, k + size // 2) + 1):
            s = s + sq[j]
        norms[k] = F(kappa) + F(alpha) * (s - gone)
    return norms


def lrn_closed(x: np.ndarray, size: int, alpha: float, beta: float, kappa: float, axis: int = -1) -> np.ndarray:
    x = np.moveaxis(np.asarray(x, F), axis, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        out = _pow_f32(lrn_norms_closed(x, size, alpha, kappa), beta) * x
    return np.moveaxis(out, 0, axis)


def _exp(xd: np.ndarray) -> np.ndarray:
    out = np.empty(xd.shape, np.float64)
    o = out.reshape(-1)
    for i, v in enumerate(xd.reshape(-1).tolist()):
        try:
            o[i] = math.exp(v)
        except OverflowError:
            o[i] = np.inf
    return out


def activate(x: np.ndarray, name: str) -> np.ndarray:
    """activations.h:21-54 with C's promotions: float x, double constants, the result rounded to float"""
    x = np.asarray(x, F)
    xd = x.astype(np.float64)
    pos = (x > 0).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        if name == "linear":
            return x.copy()
        if name == "leaky":
            return np.where(x > 0, x, (.1 * xd).astype(F))
        if name == "logistic":
            return (1. / (1. + _exp(-xd))).astype(F)
        if name == "relu":
            return x * pos
        if name == "relie":
            return np.where(x > 0, x, (.01 * xd).astype(F))
        if name == "ramp":
            return ((x * pos).astype(np.float64) + .1 * xd).astype(F)
        if name == "tanh":
            e = _exp((F(2) * x).astype(np.float64))
            return ((e - 1) / (e + 1)).astype(F)
        if name == "plse":
            lo = (.01 * (x + F(4)).astype(np.float64)).astype(F)
            hi = (.01 * (x - F(4)).astype(np.float64) + 1).astype(F)
            return np.where(x < -4, lo, np.where(x > 4, hi, (.125 * xd + .5).astype(F)))
        if name == "elu":
            return (((x >= 0).astype(F) * x).astype(np.float64) + (x < 0).astype(np.float64) * (_exp(xd) - 1)).astype(F)
        if name == "loggy":
            return (2. / (1. + _exp(-xd)) - 1).astype(F)
        if name == "stair":
            n = np.floor(xd)
            even = np.floor(xd / 2.).astype(F)
            odd = ((x - n.astype(F)).astype(np.float64) + np.floor(xd / 2.)).astype(F)
            return np.where(np.mod(n, 2) == 0, even, odd)
        if name == "hardtan":
            return np.where(x < -1, F(-1), np.where(x > 1, F(1), x))
        if name == "lhtan":
            return np.where(x < 0, (.001 * xd).astype(F), np.where(x > 1, (.001 * (x - F(1)).astype(np.float64) + 1).astype(F), x))
    raise ValueError(name)
