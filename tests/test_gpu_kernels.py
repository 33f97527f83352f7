"""GPU unit tests of the individual HIP kernels against the oracle's primitives:
bit-exact for copies / comparisons / the region, decode and NMS arithmetic, and
for the convolution on integer-valued data (where fp32 sums are exact in any
order); edge cases follow SURVEY.md 8a/8c (2x2 stride-1 maxpool reading past the
edge, the reorg quirk, NMS ties, large-magnitude softmax, empty inputs)."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import layer_rule
from tests.helpers import materialize

pytestmark = pytest.mark.gpu


class Dev:
    """Tiny device-buffer helper over the C-ABI (y2h_malloc / memcpy)."""

    def __init__(self):
        self.L = darknet.lib()
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.L.y2h_malloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.L.y2h_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
        self.bufs.append(p)
        return p

    def empty(self, nbytes):
        p = C.c_void_p()
        assert self.L.y2h_malloc(C.byref(p), max(nbytes, 16)) == 0
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
    d.L.y2h_set_device(0)
    yield d
    d.close()


def to_nhwc(x):   # [n,c,h,w] -> [n,h,w,c]
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


def to_nchw(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


def _both_storages(ident, *case):
    """One case for the fp32 entry under `ident` and for the half-storage entry (y2h_*_f16) under `ident`-f16.  Half data
    is chosen exactly representable in half, where max, copy and permutation are exact: both legs compare bit for bit."""
    return [pytest.param(np.float32, *case, id=ident), pytest.param(np.float16, *case, id=ident + "-f16")]


def _offset(p, elements, dtype):
    return C.c_void_p(p.value + elements * np.dtype(dtype).itemsize)


@pytest.mark.parametrize("n,c,h,w", [(1, 3, 5, 7), (2, 32, 19, 19), (3, 425, 13, 13), (1, 1, 1, 1), (2, 70, 33, 65)])
def test_layout_round_trip(dev, n, c, h, w):
    L = dev.L
    x = synth.uniform(1, n * c * h * w, -1, 1).reshape(n, c, h, w)
    dx = dev.put(x)
    dy = dev.empty(x.nbytes)
    dz = dev.empty(x.nbytes)
    L.y2h_nchw_to_nhwc.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.y2h_nhwc_to_nchw.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    assert L.y2h_nchw_to_nhwc(dx, dy, n, c, h, w, c, None) == 0
    assert np.array_equal(dev.get(dy, (n, h, w, c)), to_nhwc(x))
    assert L.y2h_nhwc_to_nchw(dy, c, dz, n, c, h, w, None) == 0
    assert np.array_equal(dev.get(dz, (n, c, h, w)), x)
    # half storage on the device, fp32 NCHW for the host: the conversion to fp32 is exact
    L.y2h_nhwc_f16_to_nchw.argtypes = L.y2h_nhwc_to_nchw.argtypes
    dh = dev.put(to_nhwc(x).astype(np.float16))
    assert L.y2h_nhwc_f16_to_nchw(dh, c, dz, n, c, h, w, None) == 0
    assert np.array_equal(dev.get(dz, (n, c, h, w)), x.astype(np.float16).astype(np.float32))


# (h, w, c, size, stride, pad, ld, off): ld = leading dimension of x and y (0: c), off = elements by which x is moved into
# its buffer.  c = 8 at ld 12 is a 16-byte layout for fp32 and not for half; off = 1 takes the pointer off 16 bytes.
MAXPOOL_CASES = sum((_both_storages("%d-%d-%d-%d-%d-%d" % k, *k, 0, 0) for k in [
    (8, 8, 16, 2, 2, 0), (13, 13, 512, 2, 1, 0), (7, 9, 3, 2, 2, 0), (9, 9, 8, 3, 2, 1), (5, 5, 4, 3, 1, 1), (6, 6, 5, 2, 1, 0),
    (4, 4, 8, 3, 2, 1)]), []) + _both_storages("5-5-8-2-2-0-ld12", 5, 5, 8, 2, 2, 0, 12, 0) + \
    _both_storages("5-5-8-2-2-0-off1", 5, 5, 8, 2, 2, 0, 0, 1)


@pytest.mark.parametrize("dtype,h,w,c,size,stride,pad,ld,off", MAXPOOL_CASES)
def test_maxpool_matches_oracle_bitwise(dev, oracle, dtype, h, w, c, size, stride, pad, ld, off):
    L = dev.L
    n = 2
    ld = ld or c
    half = dtype == np.float16
    x = synth.uniform(3, n * c * h * w, -2, 2).reshape(n, c, h, w)
    if half:          # multiples of 1/64, and the lowest finite half below
        x = (np.round(x * 64) / 64).astype(np.float32)
    x[0, 0, 0, 0] = np.float32(-65504 if half else -3.0e38)
    oh, ow = (h + 2 * pad) // stride, (w + 2 * pad) // stride
    want = oracle.maxpool(x, n, h, w, c, size, stride, pad).reshape(n, c, oh, ow)
    if half:
        # a window with no tap inside the image (5-5-4-3-1-1: the last row and column) keeps the starting value, which
        # is -FLT_MAX in fp32 and the lowest finite half, -65504, in half: no input is below it
        want = np.maximum(want, np.float32(-65504)).astype(np.float16)
    rows = np.zeros((n, h, w, ld), dtype)
    rows[..., :c] = to_nhwc(x)
    dx = dev.put(np.concatenate([np.zeros(off, dtype), rows.reshape(-1)]))
    sentinel = dtype(-7)
    dy = dev.put(np.full(n * oh * ow * ld, sentinel, dtype))
    fn = L.y2h_maxpool_f16 if half else L.y2h_maxpool
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p]
    assert fn(_offset(dx, off, dtype), ld, dy, ld, n, h, w, c, size, stride, pad, oh, ow, None) == 0
    got = dev.get(dy, (n, oh, ow, ld), dtype)
    assert np.array_equal(to_nchw(got[..., :c]), want)
    assert np.all(got[..., c:] == sentinel)           # the padding columns of y are not written


@pytest.mark.parametrize("dtype,w,h,c,s", sum((_both_storages("%d-%d-%d-%d" % k, *k) for k in [
    (2, 2, 4, 2), (2, 2, 8, 2), (4, 2, 4, 2), (38, 38, 64, 2), (6, 6, 9, 3)]), []))
@pytest.mark.parametrize("reverse", [0, 1])
def test_reorg_quirk_matches_oracle_bitwise(dev, oracle, dtype, w, h, c, s, reverse):
    L = dev.L
    n = 2
    if reverse:
        h, w = max(h // s, 1), max(w // s, 1)
    x = np.arange(n * c * h * w, dtype=np.float32).reshape(n, c, h, w)
    if dtype == np.float16:
        x = x % 2039          # integers below 2048 are exact in half; a prime period, so a wrong permutation still shows
    want = oracle.reorg(x, w, h, c, n, s, forward=reverse).astype(dtype)
    oc, oh, ow = (c // (s * s), h * s, w * s) if reverse else (c * s * s, h // s, w // s)
    dx = dev.put(to_nhwc(x).astype(dtype))
    dy = dev.empty(x.nbytes)
    fn = L.y2h_reorg_f16 if dtype == np.float16 else L.y2h_reorg
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
    assert fn(dx, c, dy, oc, n, h, w, c, s, reverse, None) == 0
    got = to_nchw(dev.get(dy, (n, oh, ow, oc), dtype)).reshape(-1)
    assert np.array_equal(got, want.reshape(-1))
    if (w, h, c, s, reverse) == (2, 2, 4, 2, 0):      # SURVEY.md appendix C known answer (batch item 0)
        assert got[:16].tolist() == [0, 2, 8, 10, 1, 3, 9, 11, 4, 6, 12, 14, 5, 7, 13, 15]


@pytest.mark.parametrize("c", [8, 12, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_copy_channels_both_storages(dev, dtype, c):
    """The [route] fallback copy: c = 8 is one 16-byte access in half and two in fp32, 12 is 16-byte in fp32 only, 5 in
    neither; a source row of c + 3 elements, or a destination that starts 3 channels into its row, breaks the 16-byte
    layout and takes the element form.  Only the c copied columns of the destination change."""
    L = dev.L
    npix, ld_dst = 7, 24
    fn = L.y2h_copy_channels_f16 if dtype == np.float16 else L.y2h_copy_channels
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p]
    sentinel = dtype(-7)
    for ld_src in (c + 3, c):
        src = (np.arange(npix * ld_src) % 2039).astype(dtype).reshape(npix, ld_src)       # exact in half
        dsrc = dev.put(src)
        for at in (0, 3):
            ddst = dev.put(np.full((npix, ld_dst), sentinel, dtype))
            assert fn(dsrc, ld_src, _offset(ddst, at, dtype), ld_dst, c, npix, None) == 0
            got = dev.get(ddst, (npix, ld_dst), dtype)
            assert np.array_equal(got[:, at:at + c], src[:, :c]), (ld_src, at)
            assert np.all(got[:, :at] == sentinel) and np.all(got[:, at + c:] == sentinel), (ld_src, at)


@pytest.mark.parametrize("hw,c", [(49, 8), (3, 8), (49, 5), (1, 16)])
@pytest.mark.parametrize("entry", ["y2h_avgpool", "y2h_avgpool_f16"])
def test_avgpool_scalar_and_vector_agree(dev, monkeypatch, entry, hw, c):
    """avgpool_layer.c:40-54 on small integers, where every sum is exact in any order: the fp32 entry, and the half
    entry in its 16-byte form (c % 8 == 0 and at least four pixels) and, with Y2_AVGPOOL_SCALAR set or where that form
    does not apply, in the scalar form, all give sum / hw rounded to fp32 once."""
    L = dev.L
    n = 2
    half = entry.endswith("_f16")
    x = np.round(synth.uniform(5, n * hw * c, -8, 8)).astype(np.float32).reshape(n, hw, c)
    want = (x.astype(np.float64).sum(axis=1) / hw).astype(np.float32)
    dx = dev.put(x.astype(np.float16 if half else np.float32))
    fn = getattr(L, entry)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    for scalar in ((False, True) if half else (False,)):
        if scalar:
            monkeypatch.setenv("Y2_AVGPOOL_SCALAR", "1")
        else:
            monkeypatch.delenv("Y2_AVGPOOL_SCALAR", raising=False)
        dy = dev.put(np.full((n, c), -7, np.float32))
        assert fn(dx, c, dy, n, 1, hw, c, None) == 0
        assert np.array_equal(dev.get(dy, (n, c)), want), scalar


def _maxpool_run(dev, oracle, dtype, n, h, w, c, size, stride, pad, ldx, ldy, seed=3):
    """-> (got [n][oh][ow][ldy], want [n][c][oh][ow]); y pre-filled with -7 and followed by 64 more of them"""
    half = dtype == np.float16
    x = synth.uniform(seed, n * c * h * w, -2, 2).reshape(n, c, h, w)
    if half:
        x = (np.round(x * 64) / 64).astype(np.float32)
    oh, ow = (h + 2 * pad) // stride, (w + 2 * pad) // stride
    want = oracle.maxpool(x, n, h, w, c, size, stride, pad).reshape(n, c, oh, ow)
    if half:
        want = np.maximum(want, np.float32(-65504)).astype(np.float16)
    rows = np.zeros((n, h, w, ldx), dtype)
    rows[..., :c] = to_nhwc(x)
    dy = dev.put(np.full(n * oh * ow * ldy + 64, -7, dtype))
    fn = dev.L.y2h_maxpool_f16 if half else dev.L.y2h_maxpool
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p]
    assert fn(dev.put(rows), ldx, dy, ldy, n, h, w, c, size, stride, pad, oh, ow, None) == 0
    got = dev.get(dy, (n * oh * ow * ldy + 64,), dtype)
    assert np.all(got[-64:] == dtype(-7))
    return got[:-64].reshape(n, oh, ow, ldy), want


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("h,w,c,size,stride,pad,ldx,ldy", layer_rule.MAXPOOL_LD)
def test_maxpool_with_two_leading_dimensions(dev, oracle, dtype, h, w, c, size, stride, pad, ldx, ldy):
    """ldx != ldy, as between a placed route and a layer of its own: 16-byte forms (c = 8 at 12 / 16 in fp32, at 8 / 24 in
    half) and element forms"""
    got, want = _maxpool_run(dev, oracle, dtype, 2, h, w, c, size, stride, pad, ldx, ldy)
    assert np.array_equal(to_nchw(got[..., :c]), want)
    assert np.all(got[..., c:] == dtype(-7))


@pytest.mark.parametrize("key", sorted(layer_rule.MAXPOOL_BIG))
def test_maxpool_second_grid_stride_trip(dev, oracle, key):
    """more than 2^21 work items: the grid is capped at 8192 workgroups, so some threads walk their loop twice"""
    n, h, w, c, size, stride, pad = layer_rule.MAXPOOL_BIG[key]
    dtype = np.float16 if key == "f16" else np.float32
    assert n * ((h + 2 * pad) // stride) * ((w + 2 * pad) // stride) * (c // (8 if key == "f16" else 4)) > 2 ** 21
    got, want = _maxpool_run(dev, oracle, dtype, n, h, w, c, size, stride, pad, c, c)
    assert np.array_equal(to_nchw(got), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("w,h,c,s", [(4, 2, 4, 2), (6, 6, 9, 3), (10, 6, 8, 2)])
def test_reorg_with_leading_dimensions_and_a_guarded_output(dev, oracle, dtype, w, h, c, s, reverse):
    """ldx = c + 2, ldy = oc + 3; the padding columns of y and what lies behind it keep their -7"""
    n = 2
    x = (np.arange(n * c * h * w, dtype=np.float32) % 2039).reshape(n, c, h, w)
    want = oracle.reorg(x, w, h, c, n, s, forward=reverse).astype(dtype)
    oc, oh, ow = (c // (s * s), h * s, w * s) if reverse else (c * s * s, h // s, w // s)
    ldx, ldy = c + 2, oc + 3
    rows = np.full((n, h, w, ldx), 60000, dtype)
    rows[..., :c] = to_nhwc(x)
    dy = dev.put(np.full(n * oh * ow * ldy + 64, -7, dtype))
    fn = dev.L.y2h_reorg_f16 if dtype == np.float16 else dev.L.y2h_reorg
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
    assert fn(dev.put(rows), ldx, dy, ldy, n, h, w, c, s, reverse, None) == 0
    got = dev.get(dy, (n * oh * ow * ldy + 64,), dtype)
    body = got[:-64].reshape(n, oh, ow, ldy)
    assert np.array_equal(to_nchw(body[..., :oc]).reshape(-1), want.reshape(-1))
    assert np.all(body[..., oc:] == dtype(-7)) and np.all(got[-64:] == dtype(-7))


def test_copy_channels_second_grid_stride_trip(dev):
    """2^20 + 300 elements of the element form (c = 5): the grid is capped at 4096 workgroups"""
    c, ld_src, ld_dst = 5, 6, 8
    npix = (layer_rule.PAST + c - 1) // c
    src = (np.arange(npix * ld_src) % 8191).astype(np.float32).reshape(npix, ld_src)
    ddst = dev.put(np.full(npix * ld_dst + 64, -7, np.float32))
    dev.L.y2h_copy_channels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p]
    assert dev.L.y2h_copy_channels(dev.put(src), ld_src, ddst, ld_dst, c, npix, None) == 0
    got = dev.get(ddst, (npix * ld_dst + 64,))
    body = got[:-64].reshape(npix, ld_dst)
    assert np.array_equal(body[:, :c], src[:, :c]) and np.all(body[:, c:] == -7) and np.all(got[-64:] == -7)


def _avgpool_f16(dev, x, ldx):
    """y2h_avgpool_f16 on x [n][hw][c] (half values) stored with row stride ldx -> [n][c]"""
    n, hw, c = x.shape
    rows = np.full((n, hw, ldx), 60000, np.float16)
    rows[..., :c] = x
    dy = dev.put(np.full(n * c + 64, -7, np.float32))
    fn = dev.L.y2h_avgpool_f16
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    assert fn(dev.put(rows), ldx, dy, n, 1, hw, c, None) == 0
    got = dev.get(dy, (n * c + 64,))
    assert np.all(got[-64:] == -7)
    return got[:-64].reshape(n, c)


@pytest.mark.parametrize("hw", layer_rule.AVGPOOL_HW + (3,))
@pytest.mark.parametrize("c,ldx", [(8, 8), (8, 16), (16, 24), (8, 12), (layer_rule.AVGPOOL_WIDE_C, layer_rule.AVGPOOL_WIDE_C)])
def test_avgpool_f16_quarters_and_leading_dimensions(dev, monkeypatch, hw, c, ldx):
    """hw = 4..7: the quarter boundaries p0 = q * hw / 4 of the 16-byte form just above its hw >= 4 limit (hw = 3, and
    ldx = 12: the scalar form); c = 1000: 125 lane groups in two workgroups, the second partly idle; ldx > c.  Integer data:
    exact in either form.  Real-valued half data: the 16-byte form, which adds four partial sums, within
    hw * 2^-24 * sum |x| / hw of the float64 mean (hw - 1 additions and a divide, each within 2^-24 relative of a partial
    result no larger than sum |x|); the scalar form equals the sequential fp32 rule of avgpool_layer.c:40-54."""
    n = 2
    vector = layer_rule.avgpool_form(True, c, ldx, hw) == "avgpool_f16_v8_kernel"
    monkeypatch.delenv("Y2_AVGPOOL_SCALAR", raising=False)
    xi = np.round(synth.uniform(50 + hw, n * hw * c, -8, 8)).astype(np.float16).reshape(n, hw, c)
    assert np.array_equal(_avgpool_f16(dev, xi, ldx), (xi.astype(np.float64).sum(axis=1) / hw).astype(np.float32))
    xr = synth.uniform(60 + hw, n * hw * c, -2, 2).astype(np.float16).reshape(n, hw, c)
    got = _avgpool_f16(dev, xr, ldx)
    seq = layer_rule.avgpool_seq(xr.astype(np.float32))
    if vector:
        x64 = xr.astype(np.float64)
        frac = np.abs(got - x64.mean(axis=1)) / (hw * 2.0 ** -24 * np.abs(x64).sum(axis=1) / hw)
        print("avgpool_f16_v8 hw %d c %d: at most %.3f of the bound" % (hw, c, float(frac.max())))
        assert frac.max() <= 1
        monkeypatch.setenv("Y2_AVGPOOL_SCALAR", "1")
        got = _avgpool_f16(dev, xr, ldx)
    assert np.array_equal(got, seq)


def test_softmax_rows_matches_oracle(dev, oracle):
    L = dev.L
    rows = np.stack([np.array([1, 2, 3, 4], np.float32), np.array([1e4, -1e4, 0, 1e4], np.float32),
                     np.array([-50, -50.5, -49, -80], np.float32), np.zeros(4, np.float32)])
    dx = dev.put(rows)
    dy = dev.empty(rows.nbytes)
    L.y2h_softmax_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_void_p]
    for temp in (1.0, 2.5):
        assert L.y2h_softmax_rows(dx, dy, 4, 4, temp, None) == 0
        got = dev.get(dy, (4, 4))
        want = np.stack([oracle.softmax(r, temp) for r in rows])
        assert np.abs(got - want).max() <= 1.2e-7     # exp() differs from glibc's by at most an ulp
    assert L.y2h_softmax_rows(dx, dy, 4, 4, 1.0, None) == 0
    assert np.allclose(dev.get(dy, (4, 4))[0], [0.0320586041, 0.0871443227, 0.236882836, 0.643914282], atol=1e-9)


def _nms_case(total, classes, seed, ties=False):
    b = synth.uniform(seed, total * 4, 0.05, 0.95).reshape(total, 4)
    b[:, 2:] = b[:, 2:] * 0.5 + 0.05
    p = synth.uniform(seed + 1, total * classes, 0, 1).reshape(total, classes)
    p[p < 0.6] = 0
    if ties:
        p[p > 0] = np.round(p[p > 0] * 8) / 8        # many exactly equal scores
        b[1] = b[0]                                   # identical boxes: IoU exactly 1
    return b.astype(np.float32), p.astype(np.float32)


@pytest.mark.parametrize("total,classes,seed,ties", [(845, 20, 1, False), (1805, 80, 2, False), (64, 3, 3, True),
                                                    (300, 7, 4, True), (1, 1, 5, False), (5, 2, 6, False)])
def test_do_nms_sort_matches_oracle_bitwise(oracle, total, classes, seed, ties):
    boxes, probs = _nms_case(total, classes, seed, ties)
    for thresh in (0.1, 0.4):
        got = darknet.do_nms_sort(boxes, probs, thresh)
        want = oracle.do_nms_sort(boxes, probs, thresh)
        # also with tied scores: the kernel reproduces the order the reference's repeated stable sort gives
        assert np.array_equal(got, want)
    allzero = darknet.do_nms_sort(boxes, np.zeros_like(probs), 0.4)
    assert not allzero.any()


@pytest.mark.parametrize("total,classes,seed", [(200, 5, 11), (845, 20, 12)])
def test_do_nms_matches_oracle_bitwise(oracle, total, classes, seed):
    boxes, probs = _nms_case(total, classes, seed)
    got = darknet.do_nms(boxes, probs, 0.4)
    assert np.array_equal(got, oracle.do_nms(boxes, probs, 0.4))


def test_box_iou_known_answer(oracle):
    assert darknet.box_iou((.5, .5, .4, .4), (.6, .6, .4, .4)) == oracle.box_iou((.5, .5, .4, .4), (.6, .6, .4, .4))
    assert abs(darknet.box_iou((.5, .5, .4, .4), (.6, .6, .4, .4)) - 0.391304165) < 1e-8


def test_resize_image_matches_oracle_bitwise(oracle):
    x = synth.image_batch(1, 3, 53, 71)[0]
    for (w, h) in [(416, 416), (32, 17), (71, 53), (1 + 70, 2)]:
        assert np.array_equal(darknet.resize_image(x, w, h), oracle.resize_image(x, w, h))


def _small_int_conv_case(workdir, spec, size, batch, seed, neg_scale=False, height=None, channels=3):
    """cfg + integer-valued weights/inputs so that every fp32 partial sum is exact in any order.
    neg_scale: batch-norm scales alternate +1, -1.5 (a negative scale turns the epilogue into a DEcreasing function).
    size is the input width; height (default: square) and channels (default 3) describe the rest of the network input."""
    import os
    import struct
    height = height or size
    layers = zoo.resolve(spec, size, height, channels)
    cfg = os.path.join(workdir, "intconv_%d.cfg" % seed)
    text = zoo.cfg_text("x", size, height, batch, spec=spec)
    if channels != 3:
        text = text.replace("\nchannels=3\n", "\nchannels=%d\n" % channels, 1)
    open(cfg, "w").write(text)
    wts = os.path.join(workdir, "intconv_%d.weights" % seed)
    with open(wts, "wb") as f:
        f.write(struct.pack("<iiii", 0, 1, 0, 0))
        s = seed
        for l in layers:
            if l["type"] != "convolutional":
                continue
            n, K = l["filters"], l["c"] * l["size"] ** 2
            s += 1
            f.write(np.round(synth.uniform(s, n, -2, 2)).astype(np.float32).tobytes())          # biases
            if l["batch_normalize"]:
                sc = np.full(n, 1, np.float32)
                if neg_scale:
                    sc[1::2] = -1.5
                f.write(sc.tobytes())                                                             # scales
                f.write(np.round(synth.uniform(s + 100, n, -2, 2)).astype(np.float32).tobytes())  # mean
                f.write(np.full(n, 1, np.float32).tobytes())                                      # variance
            f.write(np.round(synth.uniform(s + 200, n * K, -1.49, 1.49)).astype(np.float32).tobytes())
    x = np.round(synth.uniform(seed + 999, batch * channels * height * size, -2, 2)).astype(np.float32)
    x = x.reshape(batch, channels, height, size)
    return cfg, wts, x


@pytest.mark.parametrize("filters,ksize,size,batch", [(128, 3, 19, 2), (64, 3, 24, 1), (32, 1, 16, 3), (160, 3, 13, 1),
                                                     (425, 1, 13, 2), (96, 3, 38, 1)])
def test_mfma_conv_is_exact_on_integer_data(oracle, workdir, filters, ksize, size, batch):
    """conv(3->32, direct) -> conv(32->filters, MFMA, linear, no BN): integer data makes the GEMM exact, so the
    implicit-GEMM indexing (taps, padding, tile edges, channel offsets) is checked bit for bit."""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", filters, ksize, 0, "linear")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 1000 + filters + ksize + size)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    out = net.network_predict(x)
    assert net.layer_kernel(1).startswith("conv_mfma_f32"), net.layer_kernel(1)
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    assert np.abs(ref).max() < 2 ** 22            # stays in the exactly-representable integer range
    assert np.array_equal(out, ref)
    net.free()
    on.close()


@pytest.mark.parametrize("cin,filters,ksize,size,batch,force", [(64, 192, 3, 13, 1, 0), (64, 1024, 3, 13, 2, 0),
                                                                (64, 128, 3, 19, 1, 3), (64, 425, 1, 13, 1, 2),
                                                                (48, 160, 3, 26, 1, 5)])
def test_split_k_conv_is_exact_on_integer_data(oracle, workdir, monkeypatch, cin, filters, ksize, size, batch, force):
    """Small grids are cut along K (partial sums through an fp32 workspace + reduce kernel).  With integer data
    every partial sum is exact, so the split must reproduce the oracle bit for bit; `force` pins the number of
    K ranges (Y2_CONV_KSPLIT) to also cover uneven splits, 0 lets the cost model choose."""
    if force:
        monkeypatch.setenv("Y2_CONV_KSPLIT", str(force))
    spec = [("conv", cin, 3, 0, "linear"), ("conv", filters, ksize, 0, "linear")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 7000 + cin + filters + ksize + size + force)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    out = net.network_predict(x)
    assert net.layer_kernel(1).startswith("conv_mfma_f32"), net.layer_kernel(1)
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    assert np.abs(ref).max() < 2 ** 22
    assert np.array_equal(out, ref)
    net.free()
    on.close()


def test_region_kernel_matches_oracle(oracle, workdir):
    """the region head inside a network; every kernel form of it by itself: tests/test_gpu_head_kernels.py"""
    cfg, wts, x = materialize(workdir, "mini", 32, 2, 3)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    out = net.network_predict(x)
    on = oracle.OracleNet(cfg, wts)
    assert np.array_equal(out, on.predict(x))
    net.free()
    on.close()
