"""GPU tests of the layers between the convolutions kernel by kernel, by direct calls of the C-ABI: y2h_shortcut
(shortcut_same_kernel<LEAKY / LINEAR / -1>, shortcut_kernel), y2h_crop, y2h_crop_f16, y2h_batchnorm, y2h_binarize, y2h_local
(local_kernel<float, 1|4|8, vector|scalar>, local_ref_kernel), y2h_local_f16 (local_kernel<half, ...>), y2h_connected_ref,
the layout kernels (y2h_nchw_to_nhwc, y2h_nhwc_to_nchw, y2h_nhwc_f16_to_nchw, y2h_nchw_to_nhwc_halo,
y2h_nchw_to_nhwc4_halo_f16), the conversions y2h_f32_to_f16 / y2h_f16_to_f32 and y2h_softmax_rows in both forms -- against
the rule of tests/layer_rule.py (pinned to the compiled reference by tests/test_layer_rule_host.py), whose cases these are;
which kernel form a case reaches is stated and checked there.

Every output lies in a guarded buffer: the tail, the columns c..ld-1 of every row, the elements in front of a moved pointer
and the border of a haloed image are pre-filled with -7 and must come back untouched.

What counts as equal.  Copies, permutations, binarize, conversions and pure fp32 / double arithmetic on named intermediates
(the files are built with -ffp-contract=off): array_equal with the rule.  Two device forms of one computation (vector
against scalar fallback, shortcut_same against shortcut_kernel): array_equal with each other.  Behind a double exp
(logistic): SOFTMAX_BAR.  The fast [local] kernel is an fma chain in lane-strided order followed by a butterfly: on integer
data array_equal; on real-valued data with a 1-Lipschitz activation within (K + 2) * 2^-24 * (|bias| + sum |w x|) of the
rule evaluated in float64 -- the any-order summation bound plus the epilogue's roundings, derived, not measured; the worst
fraction of that bound is printed.  The half [local] on integer data: the fp32 rule rounded once to half.  y2h_softmax_rows:
two fp32 spacings of the rule's value (the sum is walked in the rule's order; the device's exp and the C library's are each
within an ulp of double) and SOFTMAX_BAR; each row sums to 1 within n * 2^-24."""
import ctypes as C

import numpy as np
import pytest

from tests import layer_rule as R
from tests.test_gpu_head_kernels import EINVAL, FILL, Out, ulps
from tests.test_gpu_hier import SOFTMAX_BAR
from tests.test_gpu_kernels import Dev

pytestmark = pytest.mark.gpu

F, H = np.float32, np.float16


def bind(L):
    vp, i, f, ln = C.c_void_p, C.c_int, C.c_float, C.c_long
    L.y2h_shortcut.argtypes = [vp, i, vp, i, vp, i] + [i] * 8 + [vp]
    L.y2h_crop.argtypes = [vp, i, vp, i] + [i] * 8 + [vp]
    L.y2h_crop_f16.argtypes = [vp, i, vp, i, vp] + [i] * 7 + [vp]
    L.y2h_batchnorm.argtypes = [vp, i, vp, i, ln, i, vp, vp, vp, vp]
    L.y2h_binarize.argtypes = [vp, i, vp, ln, i, vp]
    L.y2h_local.argtypes = [vp, i, vp, vp, vp, i] + [i] * 12 + [vp]
    L.y2h_local_f16.argtypes = [vp, i, vp, vp, vp, i] + [i] * 11 + [vp]
    L.y2h_connected_ref.argtypes = [vp, ln, i, i, i, vp, vp, i, i, i, i, vp, vp, vp, vp, vp]
    L.y2h_nchw_to_nhwc.argtypes = [vp, vp] + [i] * 5 + [vp]
    L.y2h_nhwc_to_nchw.argtypes = [vp, i, vp] + [i] * 4 + [vp]
    L.y2h_nhwc_f16_to_nchw.argtypes = L.y2h_nhwc_to_nchw.argtypes
    L.y2h_nchw_to_nhwc_halo.argtypes = [vp, vp] + [i] * 6 + [vp]
    L.y2h_nchw_to_nhwc4_halo_f16.argtypes = [vp, vp] + [i] * 4 + [vp]
    L.y2h_f32_to_f16.argtypes = [vp, vp, ln, vp]
    L.y2h_f16_to_f32.argtypes = [vp, vp, ln, vp]
    L.y2h_softmax_rows.argtypes = [vp, vp, ln, i, f, vp]
    return L


@pytest.fixture()
def dev():
    d = Dev()
    bind(d.L)
    d.L.y2h_set_device(0)
    yield d
    d.close()


def put2d(dev, a, ld=0, off=0, dtype=F):
    """a [rows][c] on the device with row stride ld (the columns c..ld-1 hold a value never to be read), `off` elements behind
    a 16-byte aligned start -> the pointer to a[0][0]"""
    a = np.asarray(a)
    n, c = a.shape
    poison = dtype(6e4 if dtype == H else 1e30)
    body = np.full((n, ld or c), poison, dtype)
    body[:, :c] = a
    p = dev.put(np.concatenate([np.full(off, poison, dtype), body.reshape(-1)]))
    return C.c_void_p(p.value + off * np.dtype(dtype).itemsize)


def put_image(dev, x_nchw, ld=0, off=0, dtype=F):
    b, c, h, w = x_nchw.shape
    return put2d(dev, R.to_nhwc(x_nchw).reshape(b * h * w, c), ld, off, dtype)


class Rows:
    """a guarded output of `pixels` rows of `ld` elements, `off` elements behind an aligned start, of which a kernel is to write
    columns at..at+c-1: everything pre-filled with FILL"""

    def __init__(self, dev, pixels, c, ld=0, off=0, at=0, dtype=F):
        self.pixels, self.c, self.ld, self.off, self.at = pixels, c, ld or c, off, at
        assert at + c <= self.ld
        self.out = Out(dev, (off + pixels * self.ld,), dtype)
        self.p = self.out.at(off + at)

    def full(self):
        """[pixels][ld], everything the buffer holds behind `off`"""
        a = self.out.pull()
        assert (a[:self.off] == FILL).all(), "written in front of the output"
        return a[self.off:].reshape(self.pixels, self.ld)

    def pull(self):
        """[pixels][c]; the other columns must hold FILL"""
        a = self.full()
        assert (a[:, :self.at] == FILL).all() and (a[:, self.at + self.c:] == FILL).all(), "columns outside the output written"
        return a[:, self.at:self.at + self.c].copy()

    def untouched(self):
        return bool((self.full() == FILL).all())


def image(a, b, h, w):
    """[b*h*w][c] -> [b][c][h][w]"""
    return R.to_nchw(a.reshape(b, h, w, -1))


def same(got, want, act, what):
    """array_equal, or SOFTMAX_BAR behind a logistic; -> the distance"""
    if act == R.LOGISTIC:
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("%s: logistic within %.3g of the rule" % (what, err))
        assert err <= SOFTMAX_BAR, what
        return err
    assert got.shape == want.shape and np.array_equal(got, want), what
    return 0.0


# =====================================================================================================================
# A. y2h_shortcut
# =====================================================================================================================
def run_shortcut(dev, c, inp, add):
    (w1, h1, c1), (w2, h2, c2) = c.g1, c.g2
    ld_in, ld_add, ld_out = c.lds
    din, dadd = put_image(dev, inp, ld_in, c.off), put_image(dev, add, ld_add, c.off)
    y = Rows(dev, c.batch * h2 * w2, c2, ld_out, c.off, c.out_at)
    rc = dev.L.y2h_shortcut(din, ld_in, dadd, ld_add, y.p, ld_out, c.batch, w1, h1, c1, w2, h2, c2, c.act, None)
    assert rc == c.rc, (c.ident, rc)
    if rc:
        assert y.untouched(), c.ident
        return None
    return image(y.pull(), c.batch, h2, w2)


@pytest.mark.parametrize("act", sorted(R.SHORTCUT_SAME))
def test_shortcut_same_shape_forms(dev, act):
    """shortcut_same_kernel<LEAKY>, <LINEAR>, <-1> (relu, logistic), and the same inputs through shortcut_kernel"""
    base, same_shape, c6 = R.SHORTCUT_SAME[act]
    inp, add = R.shortcut_data(base)
    vec = run_shortcut(dev, base, inp, add)
    same(vec, R.shortcut(inp, add, base.act), base.act, base.ident)
    if base.act != R.LOGISTIC:
        assert vec[0, 0, 0, 0] == 0                              # .5 + -.5
    for c in same_shape:
        assert np.array_equal(run_shortcut(dev, c, inp, add), vec), c.ident
    inp, add = R.shortcut_data(c6)
    same(run_shortcut(dev, c6, inp, add), R.shortcut(inp, add, c6.act), c6.act, c6.ident)


@pytest.mark.parametrize("c", R.SHORTCUT_GENERAL + R.SHORTCUT_BIG, ids=lambda c: c.ident)
def test_shortcut_geometries(dev, c):
    inp, add = R.shortcut_data(c)
    got = run_shortcut(dev, c, inp, add)
    want = R.shortcut(inp, add, c.act)
    same(got, want, c.act, c.ident)
    assert not np.array_equal(want, R.activate(inp, c.act))          # something was added


@pytest.mark.parametrize("c", R.SHORTCUT_REFUSED, ids=lambda c: c.ident)
def test_shortcut_refusals(dev, c):
    inp, add = R.shortcut_data(c)
    assert run_shortcut(dev, c, inp, add) is None


# =====================================================================================================================
# B. y2h_crop, y2h_crop_f16
# =====================================================================================================================
@pytest.mark.parametrize("c", R.CROP + [R.CROP_BIG], ids=lambda c: c.ident)
def test_crop(dev, c):
    x = R.crop_data(c)
    ldx, ldy = c.ldx or c.c, c.ldy or c.c
    hh, ww = c.oh + 2 * c.halo, c.ow + 2 * c.halo
    y = Rows(dev, c.batch * hh * ww, c.c, ldy)
    assert dev.L.y2h_crop(put_image(dev, x, ldx), ldx, y.p, ldy, c.batch, c.h, c.w, c.c, c.oh, c.ow, c.noadjust, c.halo, None) == 0
    want = np.full((c.batch, hh, ww, ldy), FILL, F)                 # the border and the padding columns keep their prefill
    rule = R.crop(x, c.oh, c.ow, c.noadjust)
    want[:, c.halo:c.halo + c.oh, c.halo:c.halo + c.ow, :c.c] = R.to_nhwc(rule)
    assert np.array_equal(y.full().reshape(want.shape), want)
    assert c.noadjust or (rule.min() == -1 and rule.max() == 1 and (rule == 0).any())


@pytest.mark.parametrize("c", R.CROP_F16 + [R.CROP_F16_BIG], ids=lambda c: c.ident)
def test_crop_f16(dev, c):
    x = R.crop_data(c)
    ldx, ldy = c.ldx or c.c, c.ldy or c.c
    y = Rows(dev, c.batch * c.oh * c.ow, c.c, ldy, dtype=H)
    y4 = Out(dev, (c.batch, c.oh + 2, c.ow + 2, 4), H)
    p4 = {"": None, "y4": y4.p, "off2": y4.at(1)}[c.y4]
    rc = dev.L.y2h_crop_f16(put_image(dev, x, ldx), ldx, y.p, ldy, p4, c.batch, c.h, c.w, c.c, c.oh, c.ow, c.noadjust, None)
    assert rc == c.rc
    want = R.half_once(R.to_nhwc(R.crop(x, c.oh, c.ow, c.noadjust)))
    want4 = np.full(y4.shape, FILL, H)
    if rc == 0 and c.y4:
        want4[:, 1:-1, 1:-1, :] = 0                                  # the channels the layer does not have
        want4[:, 1:-1, 1:-1, :c.c] = want
    assert np.array_equal(y4.pull(), want4)
    if rc:
        assert y.untouched()
    else:
        assert np.array_equal(y.pull().reshape(want.shape), want)


# =====================================================================================================================
# C. y2h_batchnorm
# =====================================================================================================================
@pytest.mark.parametrize("c", R.BATCHNORM, ids=lambda c: c.ident)
def test_batchnorm(dev, c):
    x, mean, var, scale = R.batchnorm_data(c)
    rinv = R.bn_rinv(var)                                            # in double, as the arena prepares it
    ldx, ldy = c.ldx or c.c, c.ldy or c.c
    y = Rows(dev, c.pixels, c.c, ldy)
    assert dev.L.y2h_batchnorm(put2d(dev, x, ldx), ldx, y.p, ldy, c.pixels, c.c, dev.put(mean), dev.put(rinv), dev.put(scale), None) == 0
    assert np.array_equal(y.pull(), R.batchnorm_dev(x, mean, rinv, scale))


# =====================================================================================================================
# D. y2h_binarize
# =====================================================================================================================
@pytest.mark.parametrize("c", R.BINARIZE, ids=lambda c: c.ident)
def test_binarize(dev, c):
    x = R.binarize_data(c)
    ldx = c.ldx or c.c
    y = Out(dev, (c.rows, c.c))
    assert dev.L.y2h_binarize(put2d(dev, x, ldx), ldx, y.p, c.rows, c.c, None) == 0
    got = y.pull()
    # +1 exactly where x > 0 in IEEE terms: the smallest subnormal gives +1; NaN, both zeros and -FLT_MIN give -1
    assert got.reshape(-1)[:R.BIN_SPECIAL.size].tolist() == R.BIN_SPECIAL_WANT.tolist()
    assert np.array_equal(got, R.binarize(x))


# =====================================================================================================================
# E. y2h_local, y2h_local_f16
# =====================================================================================================================
def run_local(dev, c, x, w, bias, mode, act=None, out=None, expect=0):
    """mode: "fast", "strict" (y2h_local) or "half" (y2h_local_f16) -> [b][n][oh][ow]"""
    dt = H if mode == "half" else F
    wp, bp = R.local_pack(w, bias)
    ldx, ldy = c.ldx or c.c, c.ldy or c.n
    oh, ow = out or c.out
    y = Rows(dev, c.batch * oh * ow, c.n, ldy, dtype=dt)
    args = (put_image(dev, x.astype(dt), ldx, c.xoff, dt), ldx, dev.put(wp.astype(dt)), dev.put(bp.astype(F)), y.p, ldy, c.batch, c.h, c.w,
            c.c, c.n, c.size, c.stride, c.pad, oh, ow, c.act if act is None else act)
    rc = dev.L.y2h_local_f16(*args, None) if mode == "half" else dev.L.y2h_local(*args, int(mode == "strict"), None)
    assert rc == expect, (c.ident, mode, rc)
    if rc:
        assert y.untouched(), (c.ident, mode)
        return None
    return image(y.pull(), c.batch, oh, ow)


@pytest.mark.parametrize("c", R.LOCAL, ids=lambda c: c.ident)
def test_local(dev, c):
    x, w, bias = R.local_data(c)
    rule = R.local(x, w, bias, c.size, c.stride, c.pad, c.act)
    twin = R.LOCAL_BY_IDENT.get(R.LOCAL_TWINS.get(c.ident))
    same(run_local(dev, c, x, w, bias, "strict"), rule, c.act, c.ident + " strict")             # also on real-valued data
    if R.local_runs_fast(c):
        got = run_local(dev, c, x, w, bias, "fast")
        if c.data == "int":
            same(got, rule, c.act, c.ident + " fast")
        else:
            pre, mag = R.local64(x, w, bias, c.size, c.stride, c.pad)
            frac = np.abs(got.astype(np.float64) - R.activate64(pre, c.act)) / R.local_bar(c, mag)
            print("%s fast: at most %.3f of the bound (K + 2) 2^-24 (|bias| + sum |w x|), K = %d" % (c.ident, float(frac.max()), c.K))
            assert frac.max() <= 1
        if twin:
            assert np.array_equal(got, run_local(dev, twin, x, w, bias, "fast")), "scalar fallback against the vector form"
    if R.local_runs_half(c):
        got = run_local(dev, c, x, w, bias, "half")
        assert np.array_equal(got, R.half_once(rule)), c.ident + " half"
        if twin:
            assert np.array_equal(got, run_local(dev, twin, x, w, bias, "half"))


def test_local_refusals(dev):
    c = R.LOCAL_BY_IDENT["b3-c8-n5-3x3s1p1"]
    x, w, bias = R.local_data(c)
    for mode in ("fast", "strict", "half"):
        for act in (4, 12, -1):                                  # only LINEAR .. RELU are evaluated inside the kernel
            run_local(dev, c, x, w, bias, mode, act=act, expect=EINVAL)
    # (out_h - 1) * stride + size - pad > h + pad: the last window would leave the padded image
    for mode in ("fast", "strict", "half"):
        run_local(dev, c._replace(pad=0), x, w, bias, mode, out=c.out, expect=EINVAL)


# =====================================================================================================================
# F. y2h_connected_ref
# =====================================================================================================================
@pytest.mark.parametrize("c", R.CONNECTED, ids=lambda c: c.ident)
def test_connected_ref(dev, c):
    x, w, bias, bn = R.connected_data(c)
    scale, mean, var = bn
    y = Out(dev, (c.batch, c.outputs))
    stats = (dev.put(mean), dev.put(R.bn_rinv(var)), dev.put(scale)) if c.bn else (None, None, None)
    dx, dw, db = dev.put(x), dev.put(w), dev.put(bias)
    assert dev.L.y2h_connected_ref(dx, c.hw * c.ld, c.ld, c.hw, c.c, dw, y.p, c.outputs, c.batch, c.bn, c.act, *stats, db, None) == 0
    want = R.connected(R.flatten_nhwc(x, c.batch, c.hw, c.c), w, bias, c.act, bn if c.bn else None, dev=True)
    same(y.pull(), want, c.act, c.ident)
    if c.bn:                                                      # batch_normalize = 1 without its statistics
        z = Out(dev, (c.batch, c.outputs))
        assert dev.L.y2h_connected_ref(dx, c.hw * c.ld, c.ld, c.hw, c.c, dw, z.p, c.outputs, c.batch, 1, c.act, None, stats[1], stats[2], db, None) == EINVAL
        assert (z.pull() == FILL).all()


# =====================================================================================================================
# G. layouts and conversions
# =====================================================================================================================
HW_SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13)}


@pytest.mark.parametrize("c", R.LAYOUT_C)
def test_layouts_with_a_leading_dimension(dev, c):
    """ld = c + 3 and a destination (source) that starts 2 channels into its row, as every placed route has it"""
    L, n, ld, at = dev.L, 2, c + 3, 2
    for hw in R.LAYOUT_HW:
        h, w = HW_SHAPES[hw]
        x = ((np.arange(n * c * hw) * 7) % 2039).astype(F).reshape(n, c, h, w)          # exact in half too
        nhwc = R.to_nhwc(x).reshape(n * hw, c)
        y = Rows(dev, n * hw, c, ld, at=at)
        assert L.y2h_nchw_to_nhwc(dev.put(x), y.p, n, c, h, w, ld, None) == 0
        assert np.array_equal(y.pull(), nhwc), (c, hw)
        for fn, dt in ((L.y2h_nhwc_to_nchw, F), (L.y2h_nhwc_f16_to_nchw, H)):
            wide = np.full((n * hw, ld), 6e4, dt)
            wide[:, at:at + c] = nhwc
            src = dev.put(wide)
            z = Out(dev, x.shape)
            assert fn(C.c_void_p(src.value + at * np.dtype(dt).itemsize), ld, z.p, n, c, h, w, None) == 0
            assert np.array_equal(z.pull(), x), (c, hw, dt)


def test_layout_refusals(dev):
    L = dev.L
    x = dev.put(np.zeros(64, F))
    y = Out(dev, (64,))
    assert L.y2h_nchw_to_nhwc(None, y.p, 1, 2, 2, 2, 2, None) == EINVAL and L.y2h_nchw_to_nhwc(x, None, 1, 2, 2, 2, 2, None) == EINVAL
    assert L.y2h_nchw_to_nhwc(x, y.p, 1, 2, 2, 2, 1, None) == EINVAL
    assert L.y2h_nchw_to_nhwc_halo(None, y.p, 1, 2, 2, 2, 2, 1, None) == EINVAL and L.y2h_nchw_to_nhwc_halo(x, None, 1, 2, 2, 2, 2, 1, None) == EINVAL
    assert L.y2h_nchw_to_nhwc_halo(x, y.p, 1, 2, 2, 2, 2, -1, None) == EINVAL
    assert (y.pull() == FILL).all()


def _halo_case(dev, n, c, h, w, ld, halo):
    x = R.real(9000 + c + halo, (n, c, h, w), -2, 2)
    hh, ww = h + 2 * halo, w + 2 * halo
    y = Rows(dev, n * hh * ww, c, ld)
    assert dev.L.y2h_nchw_to_nhwc_halo(dev.put(x), y.p, n, c, h, w, y.ld, halo, None) == 0
    want = np.full((n, hh, ww, y.ld), FILL, F)
    want[:, halo:halo + h, halo:halo + w, :c] = R.to_nhwc(x)
    assert np.array_equal(y.full().reshape(want.shape), want), (c, halo, ld)


def test_nchw_to_nhwc_halo(dev):
    for c, halo, ld in R.HALO:
        _halo_case(dev, 2, c, 5, 7, ld, halo)


def test_nchw_to_nhwc_halo_second_trip(dev):
    c, n, h, w = R.HALO_BIG
    _halo_case(dev, n, c, h, w, 0, 1)


def test_nchw_to_nhwc4_halo_f16(dev):
    L, n, h, w = dev.L, 2, 5, 7
    for c in (1, 3, 4):
        x = R.real(9100 + c, (n, c, h, w), -2, 2)
        y = Out(dev, (n, h + 2, w + 2, 4), H)
        assert L.y2h_nchw_to_nhwc4_halo_f16(dev.put(x), y.p, n, c, h, w, None) == 0
        want = np.full(y.shape, FILL, H)
        want[:, 1:-1, 1:-1, :] = 0                                  # missing channels: exactly 0
        want[:, 1:-1, 1:-1, :c] = R.half_once(R.to_nhwc(x))
        assert np.array_equal(y.pull(), want), c
    x = dev.put(R.real(9105, (n, 5, h, w), -2, 2))
    y = Out(dev, (n, h + 2, w + 2, 4), H)
    assert L.y2h_nchw_to_nhwc4_halo_f16(x, y.p, n, 5, h, w, None) == EINVAL            # more than four channels
    assert L.y2h_nchw_to_nhwc4_halo_f16(x, y.at(1), n, 3, h, w, None) == EINVAL        # destination 2 bytes off 8
    assert (y.pull() == FILL).all()


def _bits_equal(got, want):
    """NaNs by isnan, everything else bit for bit"""
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan])


def test_f16_to_f32_every_half(dev):
    halves = R.all_halves()
    y = Out(dev, (65536,))
    assert dev.L.y2h_f16_to_f32(dev.put(halves), y.p, 65536, None) == 0
    assert _bits_equal(y.pull(), halves.astype(F))


def test_f32_to_f16_rounds_to_nearest_even(dev):
    v = R.f32_to_f16_values()
    y = Out(dev, (v.size,), H)
    assert dev.L.y2h_f32_to_f16(dev.put(v), y.p, v.size, None) == 0
    with np.errstate(over="ignore"):
        want = v.astype(H)
    got = y.pull()
    assert _bits_equal(got, want), v[(got.view(np.uint16) != want.view(np.uint16)) & ~np.isnan(want)][:8]
    edge = dict(zip([65504., 65519.996, 65520., 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10)], [65504., 65504., np.inf, 2.0 ** -24, 0., 2.0 ** -24]))
    for k, r in edge.items():
        assert (got[v == F(k)] == H(r)).all() and (v == F(k)).any(), k


def test_conversions_second_trip(dev):
    v = R.real(9200, (R.PAST,), -70000, 70000)
    y = Out(dev, (v.size,), H)
    assert dev.L.y2h_f32_to_f16(dev.put(v), y.p, v.size, None) == 0
    with np.errstate(over="ignore"):
        want = v.astype(H)
    assert _bits_equal(y.pull(), want) and np.isinf(want).any()
    z = Out(dev, (v.size,))
    assert dev.L.y2h_f16_to_f32(dev.put(want), z.p, v.size, None) == 0
    assert _bits_equal(z.pull(), want.astype(F))


# =====================================================================================================================
# H. y2h_softmax_rows
# =====================================================================================================================
@pytest.mark.parametrize("n", R.SOFTMAX_N)
def test_softmax_rows(dev, n):
    """the LDS form up to 12288 classes in one and several trips of the 256-thread loops, softmax_rows_kernel<false> from 12289"""
    rows = R.softmax_rows_data(n)
    dx = dev.put(rows)
    for temp in R.SOFTMAX_TEMPS:
        y = Out(dev, rows.shape)
        assert dev.L.y2h_softmax_rows(dx, y.p, rows.shape[0], n, temp, None) == 0
        got, want = y.pull(), R.softmax_rule(rows, temp)
        u, err = ulps(got, want), float(np.abs(got - want).max())
        sums = np.abs(got.astype(np.float64).sum(axis=1) - 1).max()
        print("softmax n = %d temp %g: %.2f fp32 spacings and %.3g from the rule, row sums within %.3g of 1" % (n, temp, u, err, sums))
        assert u <= 2 and err <= SOFTMAX_BAR and sums <= n * 2.0 ** -24
        hot = rows[3] == F(1e4)                                  # the +-1e4 row: exact zeros and exactly 1 / count
        assert (got[3][~hot] == 0).all() and (got[3][hot] == F(1) / F(hot.sum())).all()


def test_softmax_rows_refusals(dev):
    L = dev.L
    dx = dev.put(np.ones(16, F))
    y = Out(dev, (16,))
    for args in ((None, y.p, 4, 4, 1.0), (dx, None, 4, 4, 1.0), (dx, y.p, 4, 4, 0.0), (dx, y.p, 0, 4, 1.0), (dx, y.p, 4, 0, 1.0)):
        assert L.y2h_softmax_rows(*args, None) == EINVAL
    assert (y.pull() == FILL).all()
