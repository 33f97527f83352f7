"""The direct split form (include/y2_splitd_rule.h, y2_conv_split.hip: the fp32 3x3 convolution on the bf16 matrix cores, both
operands as three bf16 planes, six MFMAs per product) against the CPU oracle.

Forced on (Y2_SPLITD=1) on layers far too small for the rule to take, the filter tile forced where a case needs a second one
(Y2_SPLITD_TILE), the persistent grid capped at three workgroups (Y2_CONV_GRID=3: every workgroup walks many tiles).  The
integer cases feed the layer integers of up to 13 bits (the network input of _small_int_conv_case times 32): the m plane is
used (asserted on the host: the layer's input reaches 256) and nothing needs more than 16 bits (asserted: below 2^16, so
l == 0 and the six products are the whole product), the sums stay below 2^24 -- the result must EQUAL the oracle's, and
behind batch-norm + leaky the direct kernel's bits."""
import os
import struct

import numpy as np
import pytest

from sr_object_detection_amd import darknet, zoo
from tests.test_gpu_kernels import _small_int_conv_case

pytestmark = pytest.mark.gpu

TILES = [(256, 128), (256, 256)]    # (positions, filters) of y2_conv_split.hip; the K-tile is 16
BK = 16
SCALE = 32.0                        # network input of the integer cases: integers in [-64, 64]


def _env(monkeypatch, splitd, tile=None, grid=3):
    for k, v in (("Y2_SPLITD", splitd), ("Y2_SPLITD_TILE", None if tile is None else "%dx%d" % tile),
                 ("Y2_CONV_GRID", None if grid is None else str(grid))):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _predict(cfg, wts, x, layer=1):
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    out = net.network_predict(x).copy()
    name = net.layer_kernel(layer)
    net.free()
    return out, name


def _oracle(oracle, cfg, wts, x):
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x).copy()
    on.close()
    return ref


def _tile_of(filters, tile):
    return tile or (256, 128 if filters <= 128 else 256)


def _name(filters, tile, pool):
    t = (256, 128) if pool else _tile_of(filters, tile)        # the pooled form has the 128-wide filter tile only
    return "conv_splitd_f32_%dx%dx%d%s" % (t[0], t[1], BK, "+maxpool2" if pool else "")


def _int_case(oracle, workdir, spec, w, batch, seed, layer=1, **kw):
    """_small_int_conv_case with the input scaled, after checking on the host what the split layer is fed: the oracle's
    output of the layers in front of it holds integers that reach 256 and stay below 2^16."""
    cfg, wts, x = _small_int_conv_case(workdir, spec[:layer], w, batch, seed, **kw)      # same seed: the same first layers and input
    x = x * np.float32(SCALE)
    d = _oracle(oracle, cfg, wts, x).astype(np.float64)
    assert np.array_equal(d, np.round(d))
    assert np.abs(d).max() >= 256, np.abs(d).max()
    assert np.abs(d).max() < 2 ** 16, np.abs(d).max()
    cfg, wts, x = _small_int_conv_case(workdir, spec, w, batch, seed, **kw)
    return cfg, wts, x * np.float32(SCALE)


def _run_exact(oracle, workdir, monkeypatch, spec, w, h, batch, seed, filters, tile, pool, layer=1):
    cfg, wts, x = _int_case(oracle, workdir, spec, w, batch, seed, layer=layer, height=h)
    ref = _oracle(oracle, cfg, wts, x)
    assert np.abs(ref).max() < 2 ** 24
    _env(monkeypatch, 1, tile)
    before = darknet.lib().y2h_conv_splitd_launches()
    out, name = _predict(cfg, wts, x, layer)
    assert name == _name(filters, tile, pool), name
    assert darknet.lib().y2h_conv_splitd_launches() > before
    assert np.array_equal(out, ref)


# width, height, batch, cin, filters (None: the forced tile's BN + 40, two filter tiles with the second partial), pool
#   7x5 b2: 2 * 6 * 9 = 108 positions, one partial tile holding both images and their zero rows, odd sizes
#   8x6 b3 n36: a partial filter tile, six K-tiles; pooled: 9 units of which 8 columns are real
#   26x26 b3: 3 * 27 * 28 = 2268 positions = nine tiles, the last partial, tile boundaries in mid-row; bn + 40: a second,
#     partial filter tile; pooled with n 128: 39 units = ten tiles, windows at every tile boundary; pooled with n 168: the
#     same patch staged once per filter tile
#   62x6 and 30x6: W + 2 = 64 and 32, the tap shifts of a row tile land on and off the 512-byte runs; pooled 62: two units
#     per row pair, the second partial
SHAPES = [(7, 5, 2, 32, 64, False), (8, 6, 3, 96, 36, False), (8, 6, 3, 96, 36, True), (26, 26, 3, 96, None, False),
          (26, 26, 3, 96, 128, True), (26, 26, 3, 96, 168, True), (62, 6, 2, 32, 64, False), (62, 6, 2, 32, 64, True), (30, 6, 2, 32, 64, False)]


def _shape_cases():
    for s in SHAPES:
        for tile in (TILES if s[4] is None else [None]):
            yield pytest.param(s, tile, id="%dx%d_b%d_c%d_n%s%s%s" % (s[0], s[1], s[2], s[3], s[4] or "bn+40", "_pool" if s[5] else "",
                                                                     "_%dx%d" % tile if tile else ""))


@pytest.mark.parametrize("shape,tile", _shape_cases())
def test_splitd_is_exact(oracle, workdir, monkeypatch, shape, tile):
    w, h, batch, cin, filters, pool = shape
    filters = filters or tile[1] + 40
    spec = [("conv", cin, 3, 0, "linear"), ("conv", filters, 3, 0, "linear")] + ([("max", 2, 2)] if pool else [])
    seed = 51000 + 7 * w + 11 * h + 13 * batch + cin + filters + 1000 * pool
    _run_exact(oracle, workdir, monkeypatch, spec, w, h, batch, seed, filters, tile, pool)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
def test_splitd_batchnorm_leaky_equals_direct_and_oracle(oracle, workdir, monkeypatch, pool):
    """batch-norm + leaky with negative scales (under the pool: the minimum of the window is what the epilogue sees): the sums
    are exact integers either way, so the shared epilogue gives the direct kernel's bits, which are the oracle's"""
    filters = 128 if pool else 168
    tile = None if pool else (256, 128)
    spec = [("conv", 96, 3, 0, "linear"), ("conv", filters, 3, 1, "leaky")] + ([("max", 2, 2)] if pool else [])
    size = 26 if pool else 19
    cfg, wts, x = _int_case(oracle, workdir, spec, size, 3, 52000 + pool, neg_scale=True)
    _env(monkeypatch, 1, tile)
    out, name = _predict(cfg, wts, x)
    assert name == _name(filters, tile, pool), name
    _env(monkeypatch, 0, None)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_") and "_k3" in dname, dname
    assert np.array_equal(out, direct)
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))
    assert (out < 0).any() and (out > 0).any()


def test_splitd_writes_into_a_route_target(oracle, workdir, monkeypatch):
    """the layer reads its input from, and writes its output into, the buffer of the [route] that concatenates the two
    (ldx = ldy = 96 + 136 = 232 > filters; output channel offset 96), on an odd map: 16-byte stores into a strided view"""
    spec = [("conv", 96, 3, 0, "linear"), ("conv", 136, 3, 1, "leaky"), ("route", [-2, -1])]
    cfg, wts, x = _int_case(oracle, workdir, spec, 13, 2, 53000, neg_scale=True, height=9)
    _env(monkeypatch, 1, None)
    out, name = _predict(cfg, wts, x)
    assert name == _name(136, None, False), name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def test_splitd_dword_stores_into_an_unaligned_stride(oracle, workdir, monkeypatch):
    """ldy = 6 + 36 = 42 floats (the [route] joins a 6-filter layer's output and this one's): rows are not 16-byte aligned, the
    outputs leave dword by dword"""
    spec = [("conv", 6, 3, 0, "linear"), ("conv", 32, 3, 0, "linear"), ("conv", 36, 3, 1, "leaky"), ("route", [0, -1])]
    cfg, wts, x = _int_case(oracle, workdir, spec, 13, 2, 53500, layer=2, neg_scale=True, height=9)
    _env(monkeypatch, 1, None)
    before = darknet.lib().y2h_conv_splitd_launches()
    out, name = _predict(cfg, wts, x, layer=2)
    assert name == _name(36, None, False), name
    assert darknet.lib().y2h_conv_splitd_launches() > before
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def _real_case(workdir, tag, seed):
    spec = [("conv", 128, 3, 1, "leaky"), ("conv", 256, 3, 1, "leaky")]
    layers = zoo.resolve(spec, 14, 14, 3)
    cfg = os.path.join(workdir, "splitd_%s.cfg" % tag)
    open(cfg, "w").write(zoo.cfg_text("x", 14, 14, 2, spec=spec))
    wts = os.path.join(workdir, "splitd_%s.weights" % tag)
    rng = np.random.RandomState(seed)
    with open(wts, "wb") as f:
        f.write(struct.pack("<iiii", 0, 1, 0, 0))
        for l in layers:
            if l["type"] != "convolutional":
                continue
            n, K = l["filters"], l["c"] * l["size"] ** 2
            f.write(rng.normal(0, 0.1, n).astype(np.float32).tobytes())                       # biases
            f.write(rng.uniform(0.8, 1.2, n).astype(np.float32).tobytes())                    # scales
            f.write(rng.normal(0, 0.1, n).astype(np.float32).tobytes())                       # mean
            f.write(rng.uniform(0.8, 1.2, n).astype(np.float32).tobytes())                    # variance
            f.write(rng.normal(0, np.sqrt(2.0 / K), n * K).astype(np.float32).tobytes())      # He-scaled weights
    x = rng.normal(0, 1, (2, 3, 14, 14)).astype(np.float32)
    return cfg, wts, x


def test_splitd_real_valued_layer_is_within_tolerance(oracle, workdir, monkeypatch):
    """c 128 -> 256, 14x14, batch 2, He-scaled weights: within 1e-4 x the layer's largest value of the oracle (the bar of
    test_dense_frames_error_by_layer); the direct kernel's error is printed beside it"""
    cfg, wts, x = _real_case(workdir, "real", 78)
    ref = _oracle(oracle, cfg, wts, x)
    _env(monkeypatch, 1, None, None)
    out, name = _predict(cfg, wts, x)
    assert name.startswith("conv_splitd_f32_"), name
    _env(monkeypatch, 0, None, None)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_"), dname
    tol = 1e-4 * float(np.abs(ref).max())
    err, derr = (float(np.abs(o - ref).max()) for o in (out, direct))
    print("layer max %.3f: |splitd - oracle| %.3g, |direct - oracle| %.3g, bound %.3g" % (np.abs(ref).max(), err, derr, tol))
    assert err <= tol


def test_splitd_non_finite_inputs_stay_where_the_direct_kernel_puts_them(workdir, monkeypatch):
    """One +inf and one NaN in the layer's input (planted through the first layer: linear, no batch-norm, so an infinite or NaN
    network input reaches every channel of its 3x3 neighbourhood): the outputs that are not finite are exactly those the direct
    kernel makes non-finite, and every other output is within the real-valued bar of it.  The split of a non-finite value is
    h = a, m = l = 0; behind it inf * m' and inf * l' of filter planes of either sign may turn the direct kernel's
    infinity into a NaN, so the comparison is of the non-finite SET, and of the NaNs the direct kernel already has."""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 64, 3, 0, "linear")]
    layers = zoo.resolve(spec, 12, 10, 3)
    cfg = os.path.join(workdir, "splitd_nonfinite.cfg")
    open(cfg, "w").write(zoo.cfg_text("x", 12, 10, 2, spec=spec))
    wts = os.path.join(workdir, "splitd_nonfinite.weights")
    rng = np.random.RandomState(79)
    with open(wts, "wb") as f:
        f.write(struct.pack("<iiii", 0, 1, 0, 0))
        for l in layers:
            n, K = l["filters"], l["c"] * l["size"] ** 2
            f.write(rng.normal(0, 0.1, n).astype(np.float32).tobytes())
            f.write(rng.normal(0, np.sqrt(2.0 / K), n * K).astype(np.float32).tobytes())
    x = rng.normal(0, 1, (2, 3, 10, 12)).astype(np.float32)
    x[0, 1, 2, 3] = np.inf
    x[1, 0, 7, 9] = np.nan
    _env(monkeypatch, 1, None)
    out, name = _predict(cfg, wts, x)
    assert name.startswith("conv_splitd_f32_"), name
    _env(monkeypatch, 0, None)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_"), dname
    bad, dbad = ~np.isfinite(out), ~np.isfinite(direct)
    print("non-finite outputs: splitd %d (NaN %d), direct %d (NaN %d) of %d" % (bad.sum(), np.isnan(out).sum(), dbad.sum(),
                                                                              np.isnan(direct).sum(), out.size))
    assert dbad.any() and not dbad.all()
    assert np.array_equal(bad, dbad)
    assert np.isnan(out[np.isnan(direct)]).all()
    ok = ~dbad
    assert np.abs(out[ok] - direct[ok]).max() <= 1e-4 * np.abs(direct[ok]).max()


def test_splitd_is_never_taken_in_strict_mode(oracle, workdir, monkeypatch):
    """strict mode keeps the reference-order direct kernel with the switch on, and equals the oracle"""
    spec = [("conv", 64, 3, 0, "linear"), ("conv", 96, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 19, 2, 54500)
    _env(monkeypatch, 1, None, None)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    out = net.network_predict(x).copy()
    name = net.layer_kernel(1)
    net.free()
    assert name == "conv_direct_f32", name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def test_splitd_switches(workdir, monkeypatch):
    """Y2_SPLITD=1 names the layer conv_splitd_f32_* and moves the launch counter; Y2_SPLITD=0 and no switch at all (a grid this
    small is never taken by the rule) are the direct kernel and leave the counter alone; integer data: the same bits"""
    spec = [("conv", 64, 3, 0, "linear"), ("conv", 96, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 19, 2, 54000)
    count = darknet.lib().y2h_conv_splitd_launches
    _env(monkeypatch, 1, None, None)
    before = count()
    out, name = _predict(cfg, wts, x)
    assert name.startswith("conv_splitd_f32_") and count() == before + 1, name
    _env(monkeypatch, 0, None, None)
    off, off_name = _predict(cfg, wts, x)
    _env(monkeypatch, None, None, None)
    plain, plain_name = _predict(cfg, wts, x)
    assert off_name == plain_name and off_name.startswith("conv_mfma_f32_") and off_name.endswith("_k3"), (off_name, plain_name)
    assert count() == before + 1
    assert np.array_equal(off, plain) and np.array_equal(out, plain)
