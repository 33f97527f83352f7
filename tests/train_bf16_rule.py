"""The rounding of the trainer's bf16 precision modes, restated in numpy: y2_bf16_rn and y2_split3 of
include/y2_split_rule.h on bit patterns, and a Bf16Trainer that is tests/train_rule.py's Trainer with the operands of the
three convolution products rounded to bf16 -- nothing else: batch norm, pooling, the heads, the cost and the update run in
the Trainer's own dtype, as the device keeps them in fp32.

Bf16Trainer is the yardstick of bf16 mode (tests/test_gpu_train_bf16.py), run in float64 and in float32: the operands are
results of earlier roundings, so a value near a bf16 tie may round the other way on the device; the two dtypes are two
realisations of where those ties fall."""
import numpy as np

from tests import train_det_rule as D
from tests import train_rule as T

F = np.float32


def bf16_rn(a):
    """y2_bf16_rn: float32 -> bf16 bits (uint16), nearest even; NaNs stay NaNs (quiet bit set), a finite value never
    becomes an infinity"""
    u = np.ascontiguousarray(a, dtype=F).view(np.uint32).astype(np.uint64)
    mag = u & 0x7fffffff
    out = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    out = np.where(mag >= 0x7f7f8000, ((u >> 16) & 0x8000) | 0x7f7f, out)
    out = np.where(mag == 0x7f800000, u >> 16, out)
    out = np.where(mag > 0x7f800000, (u >> 16) | 0x0040, out)
    return out.astype(np.uint16)


def bf16_f32(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(F)


def split3(a):
    """y2_split3: float32 -> (h, m, l) bf16 bits with h + m + l == a; a non-finite a gives h = a, m = l = 0"""
    a = np.ascontiguousarray(a, dtype=F)
    fin = (a.view(np.uint32) & 0x7fffffff) < 0x7f800000
    h = bf16_rn(a)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(fin, a - bf16_f32(h), F(0)).astype(F)
        m = bf16_rn(r)
        r = (r - bf16_f32(m)).astype(F)
    l = bf16_rn(r)
    return h, np.where(fin, m, 0).astype(np.uint16), np.where(fin, l, 0).astype(np.uint16)


def bf16_round(a):
    """the values after y2_bf16_rn, in a's dtype (the value goes through float32 first, as it does on the device)"""
    a = np.asarray(a)
    return bf16_f32(bf16_rn(a.astype(F))).astype(a.dtype)


class _Bf16Products:
    """_conv_forward / _conv_backward with bf16 operands for the three products: the layer's input, its weights and the
    delta the products read are rounded for the products only; what is stored, reduced or handed on is not"""

    def _conv_forward(self, l, d, x):
        full = d["weights"]
        d["weights"] = bf16_round(full)
        try:
            return super()._conv_forward(l, d, bf16_round(x))          # d["xp"], kept for the weight gradient, is rounded too
        finally:
            d["weights"] = full

    def _conv_backward(self, l, d, prev):
        # the base class computes delta (activation gradient, bias / scale sums, batch-norm backward) and the two products
        # from it in one go: run it for the unrounded delta and every reduction, then redo the two products with rounded
        # operands (d["xp"] already holds the rounded input)
        full_w, wu0 = d["weights"], d["weight_updates"]
        super()._conv_backward(l, d, prev)
        delta = d["delta"]
        _, n, k, padflag, bn, act = l
        p = k // 2 if padflag else 0
        dr, wr, xp = bf16_round(delta), bf16_round(full_w), d["xp"]
        B, _, oh, ow = delta.shape
        dw = np.zeros_like(full_w)
        dxp = np.zeros_like(xp)
        for ky in range(k):
            for kx in range(k):
                dw[:, :, ky, kx] = np.einsum("bnhw,bchw->nc", dr, xp[:, :, ky:ky + oh, kx:kx + ow], optimize=True)
                if prev is not None:
                    dxp[:, :, ky:ky + oh, kx:kx + ow] += np.einsum("bnhw,nc->bchw", dr, wr[:, :, ky, kx], optimize=True)
        d["weight_updates"] = wu0 + dw
        if prev is not None:
            H, W = xp.shape[2] - 2 * p, xp.shape[3] - 2 * p
            prev["delta"] = dxp[:, :, p:p + H, p:p + W].copy()


class Bf16Trainer(_Bf16Products, T.Trainer):
    pass


class Bf16DetTrainer(_Bf16Products, D.DetTrainer):
    pass
