"""The three products of a trainable [connected] layer (y2h_train_dense_forward / _dweight / _dinput), exactly.

Integer-valued operands, small enough that every fp32 partial sum is an integer below 2^24: such sums are exact in any
order, so each product must EQUAL numpy's whatever the range count.  Rows 1, 3, 33, 64, 65 (one pass, a partial pass, more
than one pass); inputs 1, 31, 216 (a 6x6x6 image: the host's CHW weights and NCHW activations go through
y2_train_pack_dense_weights and NHWC, and come back through the unpack) and 1000 (no multiple of a staging step, and with
odd outputs no 16-byte aligned rows); outputs 1, 5, 117, 130; range counts forced to 1, 3 and the plan's maximum (every
step its own range).  The weight gradient lands in a pre-filled buffer (+=) and in a zeroed one; the input gradient
stores over a poisoned buffer and adds to a pre-filled one."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests.test_gpu_kernels import Dev, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 33, 64, 65]
INPUTS = [1, 31, 216, 1000]
OUTPUTS = [1, 5, 117, 130]
IMAGE = {216: (6, 6, 6)}          # inputs -> (c, h, w) of the layer in front


@pytest.fixture()
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


def ints(rng, shape, lo, hi):
    return rng.randint(lo, hi + 1, size=shape).astype(np.float32)


def pack(L, w, outputs, chw):
    out = np.zeros_like(w)
    L.y2_train_pack_dense_weights(w.ctypes.data, out.ctypes.data, outputs, *chw)
    return out


def unpack(L, w, outputs, chw):
    out = np.zeros_like(w)
    L.y2_train_unpack_dense_weights(np.ascontiguousarray(w).ctypes.data, out.ctypes.data, outputs, *chw)
    return out


def to_device_rows(x, chw):
    """the reference's [batch][c*h*w] rows as the trainer holds them: dense NHWC"""
    return x if chw[1] * chw[2] == 1 else to_nhwc(x.reshape((x.shape[0],) + chw)).reshape(x.shape[0], -1)


def from_device_rows(x, chw):
    c, h, w = chw
    return x if h * w == 1 else to_nchw(x.reshape(x.shape[0], h, w, c)).reshape(x.shape[0], -1)


@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("rows", ROWS)
def test_three_products_exactly(dev, rows, inputs):
    L = dev.L
    chw = IMAGE.get(inputs, (inputs, 1, 1))
    rng = np.random.RandomState(1000 * rows + inputs)
    x = ints(rng, (rows, inputs), -3, 3)
    d_x = dev.put(to_device_rows(x, chw))
    for outputs in OUTPUTS:
        g = darknet.TrainDense(rows, inputs, outputs)
        w = ints(rng, (outputs, inputs), -2, 2)
        d = ints(rng, (rows, outputs), -2, 2)
        dw0 = ints(rng, (outputs, inputs), -5, 5)
        dx0 = ints(rng, (rows, inputs), -5, 5)
        x64, w64, d64 = x.astype(np.float64), w.astype(np.float64), d.astype(np.float64)
        y_ref, dw_ref, dx_ref = x64 @ w64.T, d64.T @ x64, d64 @ w64
        assert max(np.abs(y_ref).max(), np.abs(dw_ref).max() + 5, np.abs(dx_ref).max() + 5) < 2 ** 24
        d_w, d_d = dev.put(pack(L, w, outputs, chw)), dev.put(d)
        # the weight gradient: += into a pre-filled buffer, and into zeros
        for first in (dw0, np.zeros_like(dw0)):
            d_dw = dev.put(pack(L, first, outputs, chw))
            assert L.y2h_train_dense_dweight(C.byref(g), d_x, d_d, d_dw, None) == 0
            got = unpack(L, dev.get(d_dw, (outputs, inputs)), outputs, chw)
            assert np.array_equal(got, (first + dw_ref).astype(np.float32)), ("dweight", rows, inputs, outputs)
        for product, total in ((darknet.DENSE_FORWARD, inputs), (darknet.DENSE_DINPUT, outputs)):
            most = darknet.train_dense_plan(rows, inputs, outputs, product, 1 << 20)[0]      # clamped to every step
            for forced in sorted({1, 3, most}):
                n, ws_bytes, bounds = darknet.train_dense_plan(rows, inputs, outputs, product, forced)
                assert n == min(forced, most) and bounds[0] == 0 and bounds[-1] == total
                d_ws = dev.empty(ws_bytes) if ws_bytes else None
                what = (rows, inputs, outputs, forced)
                if product == darknet.DENSE_FORWARD:
                    d_y = dev.put(np.full((rows, outputs), np.nan, np.float32))
                    assert L.y2h_train_dense_forward(C.byref(g), d_x, d_w, d_y, d_ws, forced, None) == 0
                    assert np.array_equal(dev.get(d_y, (rows, outputs)), y_ref.astype(np.float32)), ("forward",) + what
                    continue
                d_dx = dev.put(np.full((rows, inputs), np.nan, np.float32))                   # store mode
                assert L.y2h_train_dense_dinput(C.byref(g), d_d, d_w, d_dx, 0, d_ws, forced, None) == 0
                got = from_device_rows(dev.get(d_dx, (rows, inputs)), chw)
                assert np.array_equal(got, dx_ref.astype(np.float32)), ("dinput store",) + what
                d_dx = dev.put(to_device_rows(dx0, chw))                                      # add mode
                assert L.y2h_train_dense_dinput(C.byref(g), d_d, d_w, d_dx, 1, d_ws, forced, None) == 0
                got = from_device_rows(dev.get(d_dx, (rows, inputs)), chw)
                assert np.array_equal(got, (dx0 + dx_ref).astype(np.float32)), ("dinput add",) + what


def test_the_env_switch_forces_the_plan(dev, monkeypatch):
    """Y2_TRAIN_DENSE_KSPLIT is what a step reads: the plan follows it, clamped, and the forward product stays exact"""
    L = dev.L
    rows, inputs, outputs = 3, 1000, 5
    monkeypatch.delenv("Y2_TRAIN_DENSE_KSPLIT", raising=False)
    assert darknet.train_dense_plan(rows, inputs, outputs)[0] == darknet.train_dense_plan(32, inputs, outputs)[0]
    monkeypatch.setenv("Y2_TRAIN_DENSE_KSPLIT", "7")
    n, ws_bytes, _ = darknet.train_dense_plan(rows, inputs, outputs)
    assert n == 7 and ws_bytes == 7 * rows * outputs * 4
    rng = np.random.RandomState(5)
    x, w = ints(rng, (rows, inputs), -3, 3), ints(rng, (outputs, inputs), -2, 2)
    g = darknet.TrainDense(rows, inputs, outputs)
    d_y = dev.empty(rows * outputs * 4)
    assert L.y2h_train_dense_forward(C.byref(g), dev.put(x), dev.put(w), d_y, dev.empty(ws_bytes), 0, None) == 0
    assert np.array_equal(dev.get(d_y, (rows, outputs)), (x.astype(np.float64) @ w.T).astype(np.float32))


def test_products_refuse_bad_arguments(dev):
    L = dev.L
    buf = dev.empty(4096)
    for bad in (darknet.TrainDense(0, 4, 4), darknet.TrainDense(4, 0, 4), darknet.TrainDense(4, 4, 0)):
        assert L.y2h_train_dense_forward(C.byref(bad), buf, buf, buf, buf, 0, None) != 0
        assert L.y2h_train_dense_dinput(C.byref(bad), buf, buf, buf, 0, buf, 0, None) != 0
        assert L.y2h_train_dense_dweight(C.byref(bad), buf, buf, buf, None) != 0
    g = darknet.TrainDense(4, 256, 8)
    assert L.y2h_train_dense_forward(C.byref(g), buf, buf, buf, None, 2, None) != 0      # two ranges need a workspace
    assert L.y2h_train_dense_forward(C.byref(g), None, buf, buf, buf, 0, None) != 0
