"""The y2h_train_rnn_* entry points driven directly (sr_object_detection_amd/csrc/y2_train_rnn.hip) against numpy
restatements of what include/y2_hip.h says they compute.  Tensors are [T][B][C], a group is one time step's B rows.

Operands are small integers (or dyadic fractions) so that every product and every sum is exact in fp32 in ANY order of
summation: the kernel's result must then EQUAL the restatement, whatever its reduction order.  Where that cannot be arranged
it is said and bounded:
  * a group mean is sum * (float)(1 / B): exact for a power-of-two B with column sums that are multiples of B (B = 2, 32) and
    for columns that sum to zero (every other B); both kinds are dealt;
  * a leaky gradient multiplies by .1f, so sums over leaky columns are not exact: compared within B * 2^-24 of the sum of
    magnitudes, the a-priori bound of a sum of B rounded terms;
  * variance_delta goes through pow() in double, which is not correctly rounded on either side: it, and the normalised delta
    that carries it, are held to 2^-22 relative to the tensor's largest value.
Every output buffer has a guard row of SENTINEL in front and behind.  A real-valued case is held against float64 under the
summation bound.  The one-hot kernel is driven with offsets that wrap, through get_rnn_data's restatement.
"""
import ctypes as C

import numpy as np
import pytest

from tests import train_rnn_rule as R
from tests.test_gpu_kernels import Dev

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
SENTINEL = F(-7654321.)
ACT = {"linear": 0, "leaky": 1, "logistic": 2, "relu": 3}        # include/y2_hip.h Y2H_ACT_*

# (T, B, C): every B of {2, 3, 31, 32, 33, 40} (16 is the row chunk: below it, a multiple, off it), C on and off the 32 columns of
# a workgroup, T = 1 included
SHAPES = [(1, 2, 1), (2, 3, 24), (4, 31, 40), (1, 32, 32), (2, 33, 96), (4, 40, 24), (2, 2, 96), (1, 40, 33), (4, 3, 1)]


@pytest.fixture()
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


def guarded(dev, a, rows_shape):
    """a [rows][C] tensor with one SENTINEL row in front and behind -> (base pointer, pointer to the tensor)"""
    width = rows_shape[-1]
    full = np.full((int(np.prod(rows_shape[:-1])) + 2, width), SENTINEL, F)
    full[1:-1] = np.asarray(a, F).reshape(-1, width)
    p = dev.put(full)
    return p, C.c_void_p(p.value + width * 4)


def read_guarded(dev, p, rows_shape):
    width = rows_shape[-1]
    full = dev.get(p, (int(np.prod(rows_shape[:-1])) + 2, width))
    assert (full[0] == SENTINEL).all() and (full[-1] == SENTINEL).all(), "a guard row was written"
    return full[1:-1].reshape(rows_shape)


def exact_groups(rng, T, B, Cn):
    """integers whose group means are exact: multiples of B per column where B is a power of two, zero sums otherwise"""
    x = rng.integers(-6, 7, size=(T, B, Cn)).astype(D)
    s = x.sum(axis=1)
    if B & (B - 1) == 0:
        x[:, 0, :] += (-s) % B                      # the column sum becomes a multiple of B
    else:
        x[:, 0, :] -= s
    return x.astype(F)


def stats_rule(x, rm, rv, keep, take):
    T, B, Cn = x.shape
    mean = (x.astype(D).sum(axis=1)).astype(F) * F(1. / B)
    d = (x - mean[:, None, :]).astype(F)
    var = ((d * d).astype(F).astype(D).sum(axis=1)).astype(F) * F(1. / (B - 1))
    rm, rv = rm.copy(), rv.copy()
    for t in range(T):
        rm = (rm * F(keep)).astype(F) + (F(take) * mean[t]).astype(F)
        rv = (rv * F(keep)).astype(F) + (F(take) * var[t]).astype(F)
    return mean, var, rm.astype(F), rv.astype(F)


@pytest.mark.parametrize("T,B,Cn", SHAPES)
def test_group_statistics_equal_the_rule(dev, T, B, Cn):
    rng = np.random.default_rng(1000 * T + 10 * B + Cn)
    x = exact_groups(rng, T, B, Cn)
    rm0, rv0 = rng.integers(-8, 9, size=Cn).astype(F), rng.integers(1, 9, size=Cn).astype(F)
    d_x = dev.put(x)
    pm, m = guarded(dev, np.zeros((T, Cn)), (T, Cn))
    pv, v = guarded(dev, np.zeros((T, Cn)), (T, Cn))
    prm, rm = guarded(dev, rm0, (1, Cn))
    prv, rv = guarded(dev, rv0, (1, Cn))
    assert dev.L.y2h_train_rnn_bn_stats(d_x, T, B, Cn, m, v, rm, rv, .95, .05, None) == 0
    want = stats_rule(x, rm0, rv0, .95, .05)
    got = (read_guarded(dev, pm, (T, Cn)), read_guarded(dev, pv, (T, Cn)), read_guarded(dev, prm, (Cn,)), read_guarded(dev, prv, (Cn,)))
    for name, g, w in zip(("mean", "variance", "rolling_mean", "rolling_variance"), got, want):
        assert np.array_equal(g, w), name
    assert np.abs(want[0]).max() > 0 or B & (B - 1)              # the power-of-two cases have means that are not all zero


def test_group_statistics_real_valued_under_the_summation_bound(dev):
    T, B, Cn = 3, 37, 50
    rng = np.random.default_rng(5)
    x = rng.standard_normal((T, B, Cn)).astype(F)
    d_x, d_m, d_v = dev.put(x), dev.empty(T * Cn * 4), dev.empty(T * Cn * 4)
    d_rm, d_rv = dev.put(np.zeros(Cn, F)), dev.put(np.ones(Cn, F))
    assert dev.L.y2h_train_rnn_bn_stats(d_x, T, B, Cn, d_m, d_v, d_rm, d_rv, .95, .05, None) == 0
    x64 = x.astype(D)
    mean, var = x64.mean(axis=1), x64.var(axis=1, ddof=1)
    u = 2. ** -24
    # a sum of B rounded additions, one more rounding for the scale: (B + 1) u times the sum of magnitudes
    bm = (B + 1) * u * np.abs(x64).sum(axis=1) / B
    assert (np.abs(dev.get(d_m, (T, Cn)) - mean) <= bm).all()
    # each term (x - m)^2 carries the mean's error twice and three roundings; then the sum's B and the scale's one
    dev2 = (x64 - mean[:, None, :]) ** 2
    bv = ((B + 5) * u * dev2.sum(axis=1) + 2 * np.sqrt(dev2).sum(axis=1) * bm) / (B - 1)
    assert (np.abs(dev.get(d_v, (T, Cn)) - var) <= bv).all()


def activate(v, act):
    v = v.astype(F)
    if act == "leaky":
        return np.where(v > 0, v, (D(.1) * v.astype(D)).astype(F))
    if act == "relu":
        return (v * (v > 0)).astype(F)
    if act == "logistic":
        return (1. / (1. + np.exp(-v.astype(D)))).astype(F)
    return v


@pytest.mark.parametrize("act", sorted(ACT))
@pytest.mark.parametrize("T,B,Cn", [(1, 3, 24), (4, 33, 40), (2, 40, 96)])
def test_group_apply_equals_the_rule(dev, act, T, B, Cn):
    rng = np.random.default_rng(B + Cn)
    y = rng.integers(-9, 10, size=(T, B, Cn)).astype(F)
    mean = rng.integers(-3, 4, size=(T, Cn)).astype(F)
    var = (rng.integers(1, 5, size=(T, Cn)).astype(F)) ** 2                # sqrt is exact
    scales, biases = rng.integers(-2, 3, size=Cn).astype(F), rng.integers(-2, 3, size=Cn).astype(F)
    py, yy = guarded(dev, y, (T, B, Cn))
    px, xx = guarded(dev, np.zeros_like(y), (T, B, Cn))
    pn, nn = guarded(dev, np.zeros_like(y), (T, B, Cn))
    code = ACT[act]
    assert dev.L.y2h_train_rnn_bn_apply(yy, xx, nn, dev.put(mean), dev.put(var), dev.put(scales), dev.put(biases), code, T, B, Cn, None) == 0
    xn = ((y - mean[:, None, :]).astype(F).astype(D) / (np.sqrt(var.astype(D)) + D(F(.000001)))[:, None, :]).astype(F)
    want = activate((xn * scales).astype(F) + biases, act)
    assert np.array_equal(read_guarded(dev, px, (T, B, Cn)), y)
    assert np.array_equal(read_guarded(dev, pn, (T, B, Cn)), xn)
    got = read_guarded(dev, py, (T, B, Cn))
    if act == "logistic":                       # exp in double is not correctly rounded on either side: one unit of fp32
        assert np.abs(got - want).max() <= 2. ** -23
    else:
        assert np.array_equal(got, want)


def gradient(y, act):
    if act == "leaky":
        return np.where(y > 0, F(1), F(.1)).astype(F)
    if act == "relu":
        return (y > 0).astype(F)
    if act == "logistic":
        return ((1 - y) * y).astype(F)
    return np.ones_like(y)


def leaky_bn(dev, d, x, xn, scales, mean, var, B, got_d, got_s, got_md, got_vd):
    """The leaky batch-norm path (rnn.train.cfg's own).  d = delta * gradient is one rounded product per value, so the three
    sums over a group are sums of B rounded terms added with B - 1 rounded additions: each is within (B + 1) u sum|term| of
    the exact sum of the exact terms of the same d (u = 2^-24, first order; the factor 2 below covers the higher orders).
    mean_delta and variance_delta multiply a sum by a factor computed in double and round once (2 u more); the normalised
    delta is three terms computed in double and rounded once, and carries the two sums' errors through its coefficients."""
    u = 2. ** -24
    d64, sc, xc = d.astype(D), scales.astype(D), (x - mean).astype(D)
    ds = (d * scales).astype(F).astype(D)                           # scale_bias: one more rounded product
    t1, t2, t3 = d64 * xn.astype(D), ds, ds * xc
    b1, b2, b3 = (2 * (B + 1) * u * np.abs(t).sum(axis=1) for t in (t1, t2, t3))
    assert (np.abs(got_s - t1.sum(axis=1)) <= b1).all()
    veps = (var + F(.00001)).astype(F).astype(D)
    f_md, f_vd = -1. / np.sqrt(veps), -.5 * np.power(veps, -1.5)
    md, vd = t2.sum(axis=1) * f_md, t3.sum(axis=1) * f_vd
    e_md = b2 * np.abs(f_md) + 4 * u * np.abs(md)
    e_vd = b3 * np.abs(f_vd) + 4 * u * np.abs(vd)
    assert (np.abs(got_md - md[0]) <= e_md[0]).all() and (np.abs(got_vd - vd[0]) <= e_vd[0]).all()
    want = ds / (np.sqrt(var.astype(D)) + D(F(.00001))) + vd[:, None, :] * 2. * xc / B + (md / B)[:, None, :]
    bound = 4 * u * (np.abs(ds / np.sqrt(var.astype(D))) + np.abs(vd[:, None, :] * 2. * xc / B) + np.abs(md / B)[:, None, :]) + \
        e_vd[:, None, :] * np.abs(2. * xc / B) + (e_md / B)[:, None, :]
    assert (np.abs(got_d - want) <= bound).all()
    assert np.abs(want).max() > 100 * bound.max()                  # the bound decides something


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("act", sorted(ACT))
@pytest.mark.parametrize("T,B,Cn", [(1, 2, 1), (2, 3, 24), (4, 31, 40), (1, 32, 32), (2, 33, 96), (4, 40, 24)])
def test_delta_groups_equal_the_rule(dev, bn, act, T, B, Cn):
    rng = np.random.default_rng(100 * B + Cn + bn)
    delta = rng.integers(-4, 5, size=(T, B, Cn)).astype(F)
    # outputs whose gradient is exact: logistic at .25 / .5 / .75, the others by sign
    out = (rng.integers(1, 4, size=(T, B, Cn)) / 4.).astype(F) if act == "logistic" else rng.integers(-3, 4, size=(T, B, Cn)).astype(F)
    x = rng.integers(-5, 6, size=(T, B, Cn)).astype(F)
    xn = (rng.integers(-8, 9, size=(T, B, Cn)) / 4.).astype(F)
    scales = rng.integers(1, 4, size=Cn).astype(F) * np.where(np.arange(Cn) % 3 == 1, F(-1), F(1))
    mean, var = rng.integers(-2, 3, size=Cn).astype(F), (rng.integers(1, 4, size=Cn).astype(F)) ** 2
    pd, dd = guarded(dev, delta, (T, B, Cn))
    pb, bb = guarded(dev, np.zeros((T, Cn)), (T, Cn))
    ps, ss = guarded(dev, np.zeros((T, Cn)), (T, Cn))
    pm, mm = guarded(dev, np.zeros(Cn), (1, Cn))
    pv, vv = guarded(dev, np.zeros(Cn), (1, Cn))
    none = C.c_void_p(None)
    code = ACT[act]
    rc = dev.L.y2h_train_rnn_delta(dev.put(out), dd, dev.put(x) if bn else none, dev.put(xn) if bn else none, dev.put(scales) if bn else none,
                                   dev.put(mean) if bn else none, dev.put(var) if bn else none, code, T, B, Cn, bb, ss, mm, vv, None)
    assert rc == 0
    d = (delta * gradient(out, act)).astype(F)                      # one fp32 product per value
    leaky_sum_bound = B * 2. ** -24 * np.abs(d.astype(D)).sum(axis=1)
    got_b = read_guarded(dev, pb, (T, Cn))
    if act == "leaky":
        assert (np.abs(got_b - d.astype(D).sum(axis=1)) <= leaky_sum_bound).all()
    else:
        assert np.array_equal(got_b, d.astype(D).sum(axis=1).astype(F))
    got_d = read_guarded(dev, pd, (T, B, Cn))
    if not bn:
        assert np.array_equal(got_d, d)
        assert (read_guarded(dev, ps, (T, Cn)) == 0).all() and (read_guarded(dev, pm, (Cn,)) == 0).all()      # untouched
        return
    if act == "leaky":
        leaky_bn(dev, d, x, xn, scales, mean, var, B, got_d, read_guarded(dev, ps, (T, Cn)), read_guarded(dev, pm, (Cn,)),
                 read_guarded(dev, pv, (Cn,)))
        return
    ds = (d * scales).astype(F)
    assert np.array_equal(read_guarded(dev, ps, (T, Cn)), (d.astype(D) * xn).sum(axis=1).astype(F))
    s2 = ds.astype(D).sum(axis=1).astype(F)
    s3 = (ds.astype(D) * (x - mean).astype(D)).sum(axis=1).astype(F)
    veps = (var + F(.00001)).astype(F).astype(D)
    md = (s2.astype(D) * (-1. / np.sqrt(veps))).astype(F)
    vd = (s3.astype(D) * (-.5 * np.power(veps, D(F(-1.5))))).astype(F)
    assert np.array_equal(read_guarded(dev, pm, (Cn,)), md[0])      # group 0's: what the reference's arrays hold after its loop
    got_vd = read_guarded(dev, pv, (Cn,))
    assert np.abs(got_vd - vd[0]).max() <= 2. ** -22 * max(np.abs(vd[0]).max(), 1e-30)
    want = (ds.astype(D) * 1. / (np.sqrt(var.astype(D)) + D(F(.00001))) + vd.astype(D)[:, None, :] * 2. * (x - mean).astype(D) / B +
            (md / F(B)).astype(D)[:, None, :]).astype(F)
    assert np.abs(got_d - want).max() <= 2. ** -22 * np.abs(want).max()


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("act", sorted(ACT))
@pytest.mark.parametrize("B,Cn", [(2, 1), (3, 24), (31, 40), (32, 32), (33, 96), (40, 24)])
def test_step_finish_equals_statistics_apply_and_combine(dev, bn, act, B, Cn):
    """one launch for a step of the self sub-layer: what bn_stats (T = 1), bn_apply and combine give one after the other"""
    rng = np.random.default_rng(7 * B + Cn + bn)
    y = exact_groups(rng, 1, B, Cn)
    proj = rng.integers(-5, 6, size=(B, Cn)).astype(F)
    rm0, rv0 = rng.integers(-8, 9, size=Cn).astype(F), rng.integers(1, 9, size=Cn).astype(F)
    scales, biases = rng.integers(-2, 3, size=Cn).astype(F), rng.integers(-2, 3, size=Cn).astype(F)
    py, yy = guarded(dev, y, (B, Cn))
    px, xx = guarded(dev, np.zeros((B, Cn)), (B, Cn))
    pn, nn = guarded(dev, np.zeros((B, Cn)), (B, Cn))
    pnext, nx = guarded(dev, np.zeros((B, Cn)), (B, Cn))
    pm, m = guarded(dev, np.zeros(Cn), (1, Cn))
    pv, v = guarded(dev, np.zeros(Cn), (1, Cn))
    prm, rm = guarded(dev, rm0, (1, Cn))
    prv, rv = guarded(dev, rv0, (1, Cn))
    none = C.c_void_p(None)
    assert dev.L.y2h_train_rnn_step_finish(yy, xx if bn else none, nn if bn else none, m if bn else none, v if bn else none, rm, rv,
                                           .95, .05, dev.put(scales), dev.put(biases), ACT[act], B, Cn, dev.put(proj), nx, None) == 0
    if bn:
        mean, var, wrm, wrv = stats_rule(y, rm0, rv0, .95, .05)
        assert np.array_equal(read_guarded(dev, pm, (Cn,)), mean[0]) and np.array_equal(read_guarded(dev, pv, (Cn,)), var[0])
        assert np.array_equal(read_guarded(dev, prm, (Cn,)), wrm) and np.array_equal(read_guarded(dev, prv, (Cn,)), wrv)
        xn = ((y[0] - mean[0]).astype(F).astype(D) / (np.sqrt(var[0].astype(D)) + D(F(.000001)))).astype(F)
        assert np.array_equal(read_guarded(dev, px, (B, Cn)), y[0])
        assert np.array_equal(read_guarded(dev, pn, (B, Cn)), xn)     # a column of equal values: 0 / 1e-6 on both sides
        want = activate((xn * scales).astype(F) + biases, act)
    else:
        want = activate(y[0] + biases, act)
        assert (read_guarded(dev, pm, (Cn,)) == 0).all() and np.array_equal(read_guarded(dev, prm, (Cn,)), rm0)     # untouched
    got, nxt = read_guarded(dev, py, (B, Cn)), read_guarded(dev, pnext, (B, Cn))
    assert np.array_equal(nxt, ((F(0) + proj) + got).astype(F))     # the combine, on the values the launch stored
    if act == "logistic":                           # exp in double is not correctly rounded on either side: one unit of fp32
        assert np.abs(got - want).max() <= 2. ** -23
    else:
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 255, 256 * 256 + 17, (1 << 20) + 3])
def test_chunked_cost_equals_the_rule(dev, n):
    """integer-valued differences: every square and every sum is exact in any order, so the chunks' sums must EQUAL the total"""
    rng = np.random.default_rng(n)
    pred, truth = rng.integers(-3, 4, size=n).astype(F), rng.integers(-3, 4, size=n).astype(F)
    bufs = [guarded(dev, np.zeros(n), (n, 1)) for _ in range(3)]
    pc, cost = guarded(dev, np.zeros(1), (1, 1))
    assert dev.L.y2h_train_cost_sse_chunked(dev.put(pred), dev.put(truth), bufs[0][1], bufs[1][1], bufs[2][1], .5, n, cost,
                                            dev.empty(256 * 4), None) == 0
    d = truth - pred
    assert np.array_equal(read_guarded(dev, bufs[0][0], (n, 1))[:, 0], d * d)
    assert np.array_equal(read_guarded(dev, bufs[1][0], (n, 1))[:, 0], d)
    assert np.array_equal(read_guarded(dev, bufs[2][0], (n, 1))[:, 0], F(.5) * d)
    assert read_guarded(dev, pc, (1,))[0] == (d.astype(D) ** 2).sum() < 2 ** 24


@pytest.mark.parametrize("T,Cn", [(1, 1), (4, 40), (7, 96)])
def test_sum_steps_adds_the_last_step_first(dev, T, Cn):
    rng = np.random.default_rng(T)
    steps = rng.standard_normal((T, Cn)).astype(F)                  # real values: the ORDER is the statement
    base = rng.standard_normal(Cn).astype(F)
    p, q = guarded(dev, base, (1, Cn))
    assert dev.L.y2h_train_rnn_sum_steps(dev.put(steps), T, Cn, q, None) == 0
    want = base.copy()
    for t in range(T - 1, -1, -1):
        want = (want + steps[t]).astype(F)
    assert np.array_equal(read_guarded(dev, p, (Cn,)), want)


@pytest.mark.parametrize("O,K", [(1, 1), (24, 20), (32, 64), (33, 31), (96, 40)])
def test_add_transposed(dev, O, K):
    rng = np.random.default_rng(O * 100 + K)
    dst, src = rng.standard_normal((O, K)).astype(F), rng.standard_normal((K, O)).astype(F)
    p, q = guarded(dev, dst, (O, K))
    assert dev.L.y2h_train_rnn_add_transposed(q, dev.put(src), O, K, None) == 0
    assert np.array_equal(read_guarded(dev, p, (O, K)), (dst + src.T).astype(F))      # one addition per value


def test_combine_is_two_additions(dev):
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((3, 24)).astype(F), rng.standard_normal((3, 24)).astype(F)
    p, q = guarded(dev, np.zeros_like(a), a.shape)
    assert dev.L.y2h_train_rnn_combine(dev.put(a), dev.put(b), q, a.size, None) == 0
    assert np.array_equal(read_guarded(dev, p, a.shape), ((F(0) + a) + b).astype(F))


@pytest.mark.parametrize("T,B,Cn", [(1, 1, 8), (4, 3, 8), (5, 2, 33)])
def test_onehot_equals_get_rnn_data(dev, T, B, Cn):
    text = bytes([1, 2, 3, 4, 5, 6, 7, 3, 2, 1, 5])
    offsets = [(9 + 4 * b) % len(text) for b in range(B)]           # streams that wrap at len inside the T steps
    tok = np.array([[text[(o + j) % len(text)] for j in range(T + 1)] for o in offsets], np.uint8)
    want_x, want_y = R.get_rnn_data(text, list(offsets), Cn, B, T)
    px, x = guarded(dev, np.full((T * B, Cn), 9), (T * B, Cn))      # every element is written: no zeroing in front
    py, y = guarded(dev, np.full((T * B, Cn), 9), (T * B, Cn))
    assert dev.L.y2h_train_rnn_onehot(dev.put(tok), T, B, Cn, x, y, None) == 0
    assert np.array_equal(read_guarded(dev, px, (T * B, Cn)), want_x)
    assert np.array_equal(read_guarded(dev, py, (T * B, Cn)), want_y)


def test_bad_arguments_are_refused(dev):
    p = dev.empty(64)
    L = dev.L
    assert L.y2h_train_rnn_bn_stats(p, 1, 1, 4, p, p, p, p, .95, .05, None) != 0          # one row: the variance divides by zero
    assert L.y2h_train_rnn_bn_stats(p, 70000, 2, 4, p, p, p, p, .95, .05, None) != 0      # more steps than a grid dimension
    assert L.y2h_train_rnn_bn_stats(None, 1, 2, 4, p, p, p, p, .95, .05, None) != 0
    assert L.y2h_train_rnn_delta(p, p, None, None, None, p, p, 0, 1, 2, 4, p, p, p, p, None) != 0   # batch norm without x
    assert L.y2h_train_rnn_sum_steps(p, 0, 4, p, None) != 0
    assert L.y2h_train_rnn_combine(p, p, p, 0, None) != 0
    assert L.y2h_train_rnn_onehot(p, 0, 1, 8, p, p, None) != 0


# ---- the fused step kernels ----
# every B of the issue's list, the bound (128) and, refused, the bound + 1; hidden on and off the 32 columns of a workgroup and
# the 32-steps of a K quarter.  fused_forward and fused_backward are not templates: one instantiation each.
FUSED_SHAPES = [(2, 1), (3, 24), (31, 40), (32, 32), (33, 96), (40, 24), (128, 96), (128, 160), (40, 132)]


def test_fused_shapes_cover_the_issues_list():
    assert {b for b, _ in FUSED_SHAPES} >= {2, 3, 31, 32, 33, 40, 128} and {h for _, h in FUSED_SHAPES} >= {1, 24, 32, 40, 96}
    assert any(h % 4 for _, h in FUSED_SHAPES) and any(h > 128 for _, h in FUSED_SHAPES)      # the scalar path; every K quarter busy


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("act", sorted(ACT))
@pytest.mark.parametrize("B,H", FUSED_SHAPES)
def test_fused_forward_equals_product_then_step_finish(dev, bn, act, B, H):
    """Integer state rows that sum to zero and integer weights: the product is exact in any order and every column of it sums to
    zero, so the statistics are exact in any order too, and the fused launch must EQUAL y2h_train_rnn_step_finish (held against
    the rule above) run on the exact product, array by array."""
    rng = np.random.default_rng(13 * B + H + bn)
    state = rng.integers(-3, 4, size=(B, H)).astype(D)
    state[0] -= state.sum(axis=0)
    w = rng.integers(-4, 5, size=(H, H)).astype(D)
    y = (state @ w.T).astype(F)
    assert np.abs(y).max() < 2 ** 20
    proj = rng.integers(-5, 6, size=(B, H)).astype(F)
    rm0, rv0 = rng.integers(-8, 9, size=H).astype(F), rng.integers(1, 9, size=H).astype(F)
    scales, biases = rng.integers(-2, 3, size=H).astype(F), rng.integers(-2, 3, size=H).astype(F)
    none = C.c_void_p(None)
    d_sc, d_bi, d_pr = dev.put(scales), dev.put(biases), dev.put(proj)
    runs = []
    for fused in (0, 1):
        bufs = {k: guarded(dev, y if (k == "y" and not fused) else np.zeros((B, H)), (B, H)) for k in ("y", "x", "xn", "next")}
        vecs = {k: guarded(dev, v, (1, H)) for k, v in (("m", np.zeros(H)), ("v", np.zeros(H)), ("rm", rm0), ("rv", rv0))}
        opt = lambda k, table: table[k][1] if bn else none
        if fused:
            rc = dev.L.y2h_train_rnn_fused_forward(dev.put(state.astype(F)), dev.put(w.astype(F)), bufs["y"][1], opt("x", bufs), opt("xn", bufs),
                                                   opt("m", vecs), opt("v", vecs), vecs["rm"][1], vecs["rv"][1], .95, .05, d_sc, d_bi,
                                                   ACT[act], B, H, d_pr, bufs["next"][1], None)
        else:
            rc = dev.L.y2h_train_rnn_step_finish(bufs["y"][1], opt("x", bufs), opt("xn", bufs), opt("m", vecs), opt("v", vecs),
                                                 vecs["rm"][1], vecs["rv"][1], .95, .05, d_sc, d_bi, ACT[act], B, H, d_pr, bufs["next"][1], None)
        assert rc == 0
        got = {k: read_guarded(dev, p, (B, H)) for k, (p, _) in bufs.items()}
        got.update({k: read_guarded(dev, p, (H,)) for k, (p, _) in vecs.items()})
        runs.append(got)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    if bn:
        assert np.array_equal(runs[1]["x"], y) and (runs[1]["m"] == 0).all() and runs[1]["v"].max() > 0


def test_fused_forward_real_valued_under_the_summation_bound(dev):
    """the matrix-core product against float64: a dot product of H rounded-free fp32 products (exact in the MFMA's fp32
    multiply? no: each product is rounded once) added with H - 1 rounded additions: within (H + 1) u sum|terms|, u = 2^-24"""
    B, H = 40, 132
    rng = np.random.default_rng(11)
    state, w = rng.standard_normal((B, H)).astype(F), (rng.standard_normal((H, H)) / 8).astype(F)
    zeros = np.zeros(H, F)
    py, yy = guarded(dev, np.zeros((B, H)), (B, H))
    pn, nn = guarded(dev, np.zeros((B, H)), (B, H))
    assert dev.L.y2h_train_rnn_fused_forward(dev.put(state), dev.put(w), yy, None, None, None, None, None, None, .95, .05, None,
                                             dev.put(zeros), ACT["linear"], B, H, dev.put(np.zeros((B, H), F)), nn, None) == 0
    exact = state.astype(D) @ w.astype(D).T
    bound = (H + 1) * 2. ** -24 * (np.abs(state.astype(D)) @ np.abs(w.astype(D)).T)
    got = read_guarded(dev, py, (B, H))
    assert (np.abs(got - exact) <= bound).all() and np.abs(exact).max() > 1000 * bound.max()
    assert np.array_equal(read_guarded(dev, pn, (B, H)), got)


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("act", sorted(ACT))
@pytest.mark.parametrize("B,H", FUSED_SHAPES)
def test_fused_backward_equals_the_rule(dev, bn, act, B, H):
    """The delta work against y2h_train_rnn_delta's restatement (equal where the sums are exact, the leaky bounds otherwise);
    the input gradient against float64 on the delta the launch stored: exact operands give EQUAL, real ones the a-priori bound
    of 32 partial dot products of 32 terms added in range order, (H + 32) u sum|terms|."""
    rng = np.random.default_rng(17 * B + H + bn)
    delta = rng.integers(-4, 5, size=(B, H)).astype(F)
    out = (rng.integers(1, 4, size=(B, H)) / 4.).astype(F) if act == "logistic" else rng.integers(-3, 4, size=(B, H)).astype(F)
    x = rng.integers(-5, 6, size=(B, H)).astype(F)
    xn = (rng.integers(-8, 9, size=(B, H)) / 4.).astype(F)
    scales = rng.integers(1, 4, size=H).astype(F) * np.where(np.arange(H) % 3 == 1, F(-1), F(1))
    mean, var = rng.integers(-2, 3, size=H).astype(F), (rng.integers(1, 4, size=H).astype(F)) ** 2
    w = rng.integers(-4, 5, size=(H, H)).astype(F)
    prev0 = rng.integers(-6, 7, size=(B, H)).astype(F)
    pd, dd = guarded(dev, delta, (B, H))
    pp, prev = guarded(dev, prev0, (B, H))
    pb, bb = guarded(dev, np.zeros(H), (1, H))
    ps, ss = guarded(dev, np.zeros(H), (1, H))
    pm, mm = guarded(dev, np.zeros(H), (1, H))
    pv, vv = guarded(dev, np.zeros(H), (1, H))
    none = C.c_void_p(None)
    nbytes = dev.L.y2h_train_rnn_fused_ws_bytes(B, H)
    assert nbytes == -(-H // 32) * B * H * 4
    pw, ws = guarded(dev, np.zeros((nbytes // 4 // H, H)), (nbytes // 4 // H, H))
    rc = dev.L.y2h_train_rnn_fused_backward(dev.put(out), dd, dev.put(x) if bn else none, dev.put(xn) if bn else none,
                                            dev.put(scales) if bn else none, dev.put(mean) if bn else none, dev.put(var) if bn else none,
                                            ACT[act], B, H, dev.put(w), bb, ss, mm, vv, prev, ws, None)
    assert rc == 0
    read_guarded(dev, pw, (nbytes // 4 // H, H))                    # the partials stay inside their bytes
    d = (delta * gradient(out, act)).astype(F)[None]
    got_d, got_b = read_guarded(dev, pd, (1, B, H)), read_guarded(dev, pb, (1, H))
    if act == "leaky":
        assert (np.abs(got_b - d.astype(D).sum(axis=1)) <= B * 2. ** -24 * np.abs(d.astype(D)).sum(axis=1)).all()
    else:
        assert np.array_equal(got_b, d.astype(D).sum(axis=1).astype(F))
    exact_delta = not bn
    if not bn:
        assert np.array_equal(got_d, d)
    elif act == "leaky":
        leaky_bn(dev, d, x[None], xn[None], scales, mean, var, B, got_d, read_guarded(dev, ps, (1, H)), read_guarded(dev, pm, (H,)),
                 read_guarded(dev, pv, (H,)))
    else:
        ds = (d * scales).astype(F)
        assert np.array_equal(read_guarded(dev, ps, (1, H)), (d.astype(D) * xn).sum(axis=1).astype(F))
        s2, s3 = ds.astype(D).sum(axis=1).astype(F), (ds.astype(D) * (x - mean).astype(D)).sum(axis=1).astype(F)
        veps = (var + F(.00001)).astype(F).astype(D)
        md = (s2.astype(D) * (-1. / np.sqrt(veps))).astype(F)
        vd = (s3.astype(D) * (-.5 * np.power(veps, D(F(-1.5))))).astype(F)
        assert np.array_equal(read_guarded(dev, pm, (H,)), md[0])
        assert np.abs(read_guarded(dev, pv, (H,)) - vd[0]).max() <= 2. ** -22 * max(np.abs(vd[0]).max(), 1e-30)
        want = (ds.astype(D) * 1. / (np.sqrt(var.astype(D)) + D(F(.00001))) + vd.astype(D)[:, None, :] * 2. * (x - mean).astype(D) / B +
                (md / F(B)).astype(D)[:, None, :]).astype(F)
        assert np.abs(got_d - want).max() <= 2. ** -22 * np.abs(want).max()
    # dprev += delta x w, on the delta the launch left
    stored = got_d[0].astype(D)
    grad = stored @ w.astype(D)
    got_p = read_guarded(dev, pp, (B, H))
    if exact_delta and act != "leaky":
        assert np.array_equal(got_p, (prev0 + grad).astype(F))
    else:
        bound = (H + 32 + 2) * 2. ** -24 * (np.abs(stored) @ np.abs(w.astype(D)) + np.abs(prev0))
        assert (np.abs(got_p - (prev0 + grad)) <= bound).all()


def test_fused_backward_without_an_input_gradient(dev):
    """step 0: no dprev, no partials, the delta work all the same"""
    B, H = 33, 40
    rng = np.random.default_rng(2)
    delta, out = rng.integers(-4, 5, size=(B, H)).astype(F), rng.integers(-3, 4, size=(B, H)).astype(F)
    pd, dd = guarded(dev, delta, (B, H))
    pb, bb = guarded(dev, np.zeros(H), (1, H))
    none = C.c_void_p(None)
    assert dev.L.y2h_train_rnn_fused_backward(dev.put(out), dd, none, none, none, none, none, ACT["relu"], B, H, none, bb, none, none, none,
                                              none, none, None) == 0
    d = delta * (out > 0)
    assert np.array_equal(read_guarded(dev, pd, (B, H)), d) and np.array_equal(read_guarded(dev, pb, (H,)), d.sum(axis=0))


def test_the_fused_kernels_refuse_what_does_not_fit(dev):
    p = dev.empty(64)
    L = dev.L
    assert L.y2h_train_rnn_fused_fits(128, 1024) == 1 and L.y2h_train_rnn_fused_fits(129, 1024) == 0
    assert L.y2h_train_rnn_fused_forward(p, p, p, None, None, None, None, None, None, .95, .05, None, p, 0, 129, 8, p, p, None) != 0
    assert L.y2h_train_rnn_fused_backward(p, p, None, None, None, None, None, 0, 129, 8, p, p, None, None, None, p, p, None) != 0
    assert L.y2h_train_rnn_fused_forward(p, p, p, None, None, p, None, None, None, .95, .05, None, p, 0, 4, 8, p, p, None) != 0   # batch norm without x
