"""GPU unit tests of y2h_lrn / y2h_lrn_f16 / y2h_activate_copy(_f16), driven through the C-ABI against the numpy rules of
tests/lrn_rule.py.

The one-pass kernel evaluates the closed form with the rule's own float32 steps (same order, no contraction), so its
norms are the rule's bit for bit and only norm^-beta differs: v_exp_f32(-beta * v_log_f32(norm)) against pow in double.
The tests hold it to 0.75e-4 x max|ref| -- the project's 1e-4 bar less the quarter tests/test_lrn_host.py spends on the
closed form itself -- and print the figure.  Strict mode is the sequential rule, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth
from tests import lrn_rule as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
GUARD = 8                                   # sentinel values in front of and behind every buffer
SIZES = (1, 2, 4, 5, 9)
PIXELS = (1, 15, 67)                        # no multiple of any tile (a tile is 256 / ceil(c/4) pixels)
PIX_MAX = max(PIXELS)
ALPHA, BETA, KAPPA = .05, .75, 1.0
EINVAL = -2


class Dev:
    def __init__(self):
        self.L = darknet.lib()
        self.L.y2h_set_device(0)
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.L.y2h_malloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.L.y2h_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
        self.bufs.append(p)
        return p

    def get(self, p, shape, dtype=np.float32):
        out = np.zeros(shape, dtype=dtype)
        assert self.L.y2h_device_sync() == 0
        assert self.L.y2h_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, None) == 0
        assert self.L.y2h_device_sync() == 0
        return out

    def close(self):
        for p in self.bufs:
            self.L.y2h_free(p)


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.close()


def _strided(x, ld, shift, dtype):
    """[GUARD + shift sentinels][pixels][ld] (channels 0..c-1 of a row = x, the rest sentinels)[GUARD sentinels]"""
    pixels, c = x.shape
    body = np.full((pixels, ld), SENTINEL, dtype)
    body[:, :c] = x
    return np.concatenate([np.full(GUARD + shift, SENTINEL, dtype), body.reshape(-1), np.full(GUARD, SENTINEL, dtype)])


def _run(dev, call, x, ldx, ldy, shift, dtype=np.float32):
    """one launch of `call(px, ldx, py, ldy, pixels, c)` on x [pixels][c] stored with row strides ldx / ldy, both buffers
    `shift` elements off their 16-byte aligned start -> y [pixels][c]; everything around y must keep its sentinel"""
    pixels, c = x.shape
    item = np.dtype(dtype).itemsize
    d_x = dev.put(_strided(x, ldx, shift, dtype))
    host_y = _strided(np.full((pixels, c), SENTINEL, dtype), ldy, shift, dtype)
    d_y = dev.put(host_y)
    off = (GUARD + shift) * item
    rc = call(C.c_void_p(d_x.value + off), ldx, C.c_void_p(d_y.value + off), ldy, pixels, c)
    assert rc == 0, (rc, dev.L.y2h_last_error())
    got = dev.get(d_y, host_y.shape, dtype)
    body = got[GUARD + shift:GUARD + shift + pixels * ldy].reshape(pixels, ldy)
    assert (got[:GUARD + shift] == SENTINEL).all() and (got[GUARD + shift + pixels * ldy:] == SENTINEL).all(), "wrote outside y"
    assert (body[:, c:] == SENTINEL).all(), "wrote behind a row's last channel"
    return body[:, :c].copy()


def _layouts(c, quantum):
    """(ldx, ldy, shift): dense rows; rows 3 wider (no vector access unless c + 3 allows it); dense rows one element off"""
    return ((c, c, 0), (c + 3, c + 3, 0), (c, c, 1), (c + quantum, c + 2 * quantum, 0))


def _lrn(dev, size, strict, alpha=ALPHA, beta=BETA, kappa=KAPPA):
    return lambda px, ldx, py, ldy, pixels, c: dev.L.y2h_lrn(px, ldx, py, ldy, pixels, c, size, alpha, beta, kappa, strict, None)


def _check_fast(got, want, what):
    bar = 0.75e-4 * float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    assert err <= bar, "%s: max error %.3g > %.3g" % (what, err, bar)
    return err / max(float(np.abs(want).max()), 1e-30)


@pytest.mark.parametrize("c", [1, 3, 5, 12, 64, 260])
def test_lrn_equals_the_rules(dev, c):
    """c = 1, size 2: c == size/2; c = 3, size 4 / 5 and c = 5, size 9: c == size/2 + 1; c < size in many; c = 260 takes 65
    four-channel groups per pixel, past one wave's 64; c = 12, 64, 260 with dense rows load 16 bytes per lane, everything
    else (c = 1, 3, 5, rows of c + 3, the shifted pointer) the scalar path; the last layout has ldx != ldy"""
    x = synth.uniform(900 + c, PIX_MAX * c, -2, 2).reshape(PIX_MAX, c)
    worst = 0.
    for size in SIZES:
        if size // 2 > c:
            continue
        args = (size, ALPHA, BETA, KAPPA)
        closed, seq = R.lrn_closed(x, *args), R.lrn_sequential(x, *args)       # once per (c, size), shared below
        assert np.isfinite(seq).all()
        for pixels in PIXELS:
            for ldx, ldy, shift in _layouts(c, 4):
                what = "c %d size %d pixels %d ld %d/%d shift %d" % (c, size, pixels, ldx, ldy, shift)
                got = _run(dev, _lrn(dev, size, 0), x[:pixels], ldx, ldy, shift)
                worst = max(worst, _check_fast(got, closed[:pixels], what))
                got = _run(dev, _lrn(dev, size, 1), x[:pixels], ldx, ldy, shift)
                assert np.array_equal(got, seq[:pixels]), what + ": strict differs from the sequential rule"
    print("c %d: worst one-pass error %.3g of max|ref|" % (c, worst))


@pytest.mark.parametrize("c,fast", [(1024, 1), (1028, 0)])
def test_lrn_wide_rows(dev, c, fast):
    """the threshold between the two kernels: c = 1024 is 256 four-channel groups, one per lane of the workgroup and a tile
    of one pixel; c = 1028 is one more, the row does not fit the tile and the reference-order kernel runs in default mode
    too (bit-equal to the sequential rule)"""
    x = synth.uniform(950 + c, 3 * c, -2, 2).reshape(3, c)
    for size in (4, 5):
        assert dev.L.y2h_lrn_fast_ok(c, size) == fast
        args = (size, .01, BETA, KAPPA)
        closed, seq = R.lrn_closed(x, *args), R.lrn_sequential(x, *args)
        for pixels in (1, 3):
            for ldx, ldy, shift in ((c, c, 0), (c + 3, c + 3, 0), (c, c, 1)):
                what = "c %d size %d pixels %d ld %d shift %d" % (c, size, pixels, ldx, shift)
                got = _run(dev, _lrn(dev, size, 0, alpha=.01), x[:pixels], ldx, ldy, shift)
                if fast:
                    _check_fast(got, closed[:pixels], what)
                else:
                    assert np.array_equal(got, seq[:pixels]), what
                assert np.array_equal(_run(dev, _lrn(dev, size, 1, alpha=.01), x[:pixels], ldx, ldy, shift), seq[:pixels]), what


@pytest.mark.parametrize("strict", [0, 1])
def test_lrn_non_finite_where_the_rule_is(dev, strict):
    """size=4 alpha=1 kappa=.1, a large value in channel 2: the norm of channels 4 and 5 is negative"""
    x = np.full((15, 6), .25, np.float32)
    x[:, 2] = 3
    x[7, 2] = .25                                  # one pixel whose norms stay positive
    want = (R.lrn_sequential if strict else R.lrn_closed)(x, 4, 1.0, .75, .1)
    assert np.isnan(want).sum() == 14 * 2
    got = _run(dev, _lrn(dev, 4, strict, alpha=1.0, kappa=.1), x, 6, 6, 0)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    if strict:
        assert np.array_equal(got[ok], want[ok])
    else:
        assert np.abs(got[ok] - want[ok]).max() <= 0.75e-4 * np.abs(want[ok]).max()


def test_lrn_refuses_bad_arguments(dev):
    p = dev.put(np.zeros(64, np.float32))
    assert dev.L.y2h_lrn(p, 3, p, 3, 1, 3, 8, ALPHA, BETA, KAPPA, 0, None) == EINVAL      # size/2 > c
    assert dev.L.y2h_lrn(p, 3, p, 3, 1, 3, 0, ALPHA, BETA, KAPPA, 0, None) == EINVAL      # size < 1
    assert dev.L.y2h_lrn(p, 2, p, 3, 1, 3, 3, ALPHA, BETA, KAPPA, 0, None) == EINVAL      # ldx < c
    assert dev.L.y2h_lrn_f16(p, 1028, p, 1028, 1, 1028, 5, ALPHA, BETA, KAPPA, None) == EINVAL


@pytest.mark.parametrize("c", [1, 3, 5, 12, 64, 260])
def test_lrn_f16_twin(dev, c):
    """half in, half out, fp32 arithmetic: inputs exact in half; within 2^-10 x max|ref| of the rule rounded to half"""
    x = synth.uniform(970 + c, PIX_MAX * c, -2, 2).reshape(PIX_MAX, c).astype(np.float16)
    x32 = x.astype(np.float32)
    for size in SIZES:
        if size // 2 > c:
            continue
        want = R.lrn_closed(x32, size, ALPHA, BETA, KAPPA).astype(np.float16).astype(np.float32)
        bar = 2.0 ** -10 * float(np.abs(want).max())
        call = lambda px, ldx, py, ldy, pixels, cc: dev.L.y2h_lrn_f16(px, ldx, py, ldy, pixels, cc, size, ALPHA, BETA, KAPPA, None)
        for pixels in PIXELS:
            for ldx, ldy, shift in _layouts(c, 4):
                got = _run(dev, call, x[:pixels], ldx, ldy, shift, np.float16).astype(np.float32)
                err = float(np.abs(got - want[:pixels]).max())
                assert err <= bar, "c %d size %d pixels %d ld %d/%d shift %d: %.3g > %.3g" % (c, size, pixels, ldx, ldy, shift, err, bar)


@pytest.mark.parametrize("name", R.ACTIVATIONS)
def test_activation_out_of_place(dev, name):
    """y[row][k] = act(x[row][k]) with ldx != ldy: exact against the in-place kernel (the strict rule of every mode), within
    1e-6 relative of the numpy formulas"""
    rows, c, ldx, ldy = 37, 13, 15, 18
    x = synth.uniform(990, rows * c, -6, 6).reshape(rows, c)
    x[0, :5] = (0, 1, -1, 4, -4)                   # the corners of hardtan, lhtan, plse
    code = R.ACT_CODE[name]
    got = _run(dev, lambda px, a, py, b, n, cc: dev.L.y2h_activate_copy(px, a, py, b, n, cc, code, None), x, ldx, ldy, 1)
    d_in = dev.put(x)
    assert dev.L.y2h_activate_array(d_in, c, rows, c, code, None) == 0
    assert np.array_equal(got, dev.get(d_in, x.shape)), "differs from y2h_activate_array"
    want = R.activate(x, name)
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), float(np.abs(got - want).max())


def test_activation_f16_twin(dev):
    rows, c, ldx, ldy = 37, 13, 15, 18
    x = synth.uniform(991, rows * c, -6, 6).reshape(rows, c).astype(np.float16)
    for name in R.ACTIVATIONS:
        code = R.ACT_CODE[name]
        call = lambda px, a, py, b, n, cc: dev.L.y2h_activate_copy_f16(px, a, py, b, n, cc, code, None)
        if code > 3:                               # only the activations the half convolutions apply
            p = dev.put(np.zeros(64, np.float16))
            assert call(p, c, p, c, 1, c) == EINVAL
            continue
        got = _run(dev, call, x, ldx, ldy, 1, np.float16).astype(np.float32)
        want = R.activate(x.astype(np.float32), name).astype(np.float16).astype(np.float32)
        assert np.abs(got - want).max() <= 2.0 ** -10 * np.abs(want).max(), name
