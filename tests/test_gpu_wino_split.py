"""The split form of the Winograd path (include/y2_split_rule.h: fp32 operands as three bf16 planes, six bf16 MFMAs per
product; wino_input_split_kernel + y2_wino_split.hip) against the CPU oracle.

Forced on (Y2_WINO=1 Y2_WINO_SPLIT=1) on layers far too small for the rule to take, the split tile forced (Y2_WINO_SPLIT_TILE) and
the persistent grid capped at three workgroups (Y2_CONV_GRID=3: many tiles per workgroup).  The integer cases feed the layer
integers of up to 13 bits (the network input of _small_int_conv_case times 32), so V = B^T d B needs the h AND the m plane
(asserted from a host restatement: |V| reaches 256) while nothing needs more than 16 bits (asserted: l == 0 everywhere, the
six products are the whole product) -- the result must EQUAL the oracle's, and behind batch-norm + leaky the direct kernel's
bits."""
import os
import struct

import numpy as np
import pytest

from sr_object_detection_amd import darknet, zoo
from tests.test_gpu_kernels import _small_int_conv_case

pytestmark = pytest.mark.gpu

SPLIT_TILES = [(256, 256)]          # (BM, BN) of y2_wino_split.hip; the K-tile is 16
BK = 16
SCALE = 32.0                        # network input of the integer cases: integers in [-64, 64]


def _env(monkeypatch, wino, split, tile=None, grid=3):
    for k, v in (("Y2_WINO", wino), ("Y2_WINO_SPLIT", split), ("Y2_WINO_SPLIT_TILE", None if tile is None else "%dx%d" % tile),
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


def _name(tile, pool):
    return "conv_winox_f32_%dx%dx%d%s" % (tile[0], tile[1], BK, "+maxpool2" if pool else "")


def _int_case(oracle, workdir, spec, w, batch, seed, **kw):
    """_small_int_conv_case with the input scaled, after checking on the host what the split layer (layer 1) is fed:
    d = the oracle's layer 0 output, V = B^T d B of every 4x4 patch.  |V| reaches 256 (the m plane is exercised), V and U need
    at most 16 bits (U = G g G^T of filters in {-1, 0, 1}: multiples of 1/4 below 2^3), so exactness is owed."""
    cfg, wts, x = _small_int_conv_case(workdir, spec[:1], w, batch, seed, **kw)          # same seed: the same layer 0 and input
    x = x * np.float32(SCALE)
    h = x.shape[2]
    d = _oracle(oracle, cfg, wts, x).reshape(batch, spec[0][1], h, w).astype(np.float64)
    th, tw = (h + 1) // 2, (w + 1) // 2
    p = np.zeros((batch, d.shape[1], 2 * th + 2, 2 * tw + 2))
    p[:, :, 1:h + 1, 1:w + 1] = d
    bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    patches = np.stack([np.stack([p[:, :, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)]) for i in range(4)])      # [i][j][b][c][ty][tx]
    v = np.einsum("ik,klbcyx,jl->ijbcyx", bt, patches, bt)
    assert np.abs(v).max() >= 256, np.abs(v).max()
    assert np.abs(v).max() < 2 ** 16 and np.array_equal(v, np.round(v))
    cfg, wts, x = _small_int_conv_case(workdir, spec, w, batch, seed, **kw)
    return cfg, wts, x * np.float32(SCALE)


# width, height, batch, cin, filters (None: bn + 40, two filter tiles with the second partial), pool
#   7x5: 24 tiles per component = one row block, almost all padding; 8x6: 36 filters = one partial filter tile; 26x26 b3: 507
#   tiles = two row blocks, the last partial; cin 32 = two K-tiles, 96 = six
SHAPES = [(7, 5, 2, 32, None, False), (8, 6, 3, 96, 36, False), (8, 6, 3, 96, 36, True), (26, 26, 3, 96, None, False), (26, 26, 3, 96, None, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_b%d_c%d_n%s%s" % (s[0], s[1], s[2], s[3], s[4] or "bn+40", "_pool" if s[5] else ""))
@pytest.mark.parametrize("tile", SPLIT_TILES, ids=lambda t: "%dx%d" % t)
def test_split_tile_is_exact(oracle, workdir, monkeypatch, tile, shape):
    w, h, batch, cin, filters, pool = shape
    filters = filters or tile[1] + 40
    spec = [("conv", cin, 3, 0, "linear"), ("conv", filters, 3, 0, "linear")] + ([("max", 2, 2)] if pool else [])
    seed = 41000 + tile[0] + 7 * w + 11 * h + 13 * batch + cin + filters + 1000 * pool
    cfg, wts, x = _int_case(oracle, workdir, spec, w, batch, seed, height=h)
    _env(monkeypatch, 1, 1, tile)
    before = darknet.lib().y2h_wino_split_launches()
    out, name = _predict(cfg, wts, x)
    assert name == _name(tile, pool), name
    assert darknet.lib().y2h_wino_split_launches() > before
    ref = _oracle(oracle, cfg, wts, x)
    assert np.abs(ref).max() < 2 ** 20
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("tile", SPLIT_TILES, ids=lambda t: "%dx%d" % t)
def test_split_batchnorm_leaky_equals_direct_and_oracle(oracle, workdir, monkeypatch, tile, pool):
    """batch-norm + leaky with negative scales (under the pool: the minimum of the window is what the epilogue sees): the sums
    are exact integers either way, so the shared epilogue gives the direct kernel's bits, which are the oracle's"""
    spec = [("conv", 96, 3, 0, "linear"), ("conv", tile[1] + 40, 3, 1, "leaky")] + ([("max", 2, 2)] if pool else [])
    size = 26 if pool else 19
    cfg, wts, x = _int_case(oracle, workdir, spec, size, 3, 42000 + tile[0] + pool, neg_scale=True)
    _env(monkeypatch, 1, 1, tile)
    out, name = _predict(cfg, wts, x)
    assert name == _name(tile, pool), name
    _env(monkeypatch, 0, 0, None)
    monkeypatch.delenv("Y2_CONV_TILE", raising=False)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_") and "_k3" in dname, dname
    assert np.array_equal(out, direct)
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))
    assert (out < 0).any() and (out > 0).any()


@pytest.mark.parametrize("tile", SPLIT_TILES, ids=lambda t: "%dx%d" % t)
def test_split_writes_into_a_route_target(oracle, workdir, monkeypatch, tile):
    """the layer reads its input from, and writes its output into, the buffer of the [route] that concatenates the two
    (ldx = ldy = 96 + 136 = 232 > filters; output channel offset 96), on an odd map"""
    spec = [("conv", 96, 3, 0, "linear"), ("conv", 136, 3, 1, "leaky"), ("route", [-2, -1])]
    cfg, wts, x = _int_case(oracle, workdir, spec, 13, 2, 43000 + tile[0], neg_scale=True, height=9)
    _env(monkeypatch, 1, 1, tile)
    out, name = _predict(cfg, wts, x)
    assert name == _name(tile, False), name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def test_split_real_valued_layer_is_within_tolerance(oracle, workdir, monkeypatch):
    """the C = 256, 14x14, batch 2 case of tests/test_gpu_wino.py (He-scaled weights): within 1e-4 * max(1, |layer max|) of the
    oracle; the fp32 Winograd and the direct errors are printed beside it"""
    spec = [("conv", 256, 3, 1, "leaky"), ("conv", 64, 3, 1, "leaky")]
    layers = zoo.resolve(spec, 14, 14, 3)
    cfg = os.path.join(workdir, "winox_real.cfg")
    open(cfg, "w").write(zoo.cfg_text("x", 14, 14, 2, spec=spec))
    wts = os.path.join(workdir, "winox_real.weights")
    rng = np.random.RandomState(77)
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
    ref = _oracle(oracle, cfg, wts, x)
    _env(monkeypatch, 1, 1, None, None)
    out, name = _predict(cfg, wts, x)
    assert name.startswith("conv_winox_f32_"), name
    _env(monkeypatch, 1, None, None, None)
    wino, wname = _predict(cfg, wts, x)
    assert wname.startswith("conv_wino_f32_"), wname
    _env(monkeypatch, 0, None, None, None)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_"), dname
    tol = 1e-4 * max(1.0, float(np.abs(ref).max()))
    err, werr, derr = (float(np.abs(o - ref).max()) for o in (out, wino, direct))
    print("layer max %.3f: |split - oracle| %.3g, |fp32 winograd - oracle| %.3g, |direct - oracle| %.3g, bound %.3g" % (
        np.abs(ref).max(), err, werr, derr, tol))
    assert err <= tol


def test_split_is_never_taken_in_strict_mode(oracle, workdir, monkeypatch):
    """strict mode keeps the reference-order direct kernel even with both switches on, and equals the oracle"""
    spec = [("conv", 64, 3, 0, "linear"), ("conv", 96, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 19, 2, 44500)
    _env(monkeypatch, 1, 1, None, None)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_strict(True)
    out = net.network_predict(x).copy()
    name = net.layer_kernel(1)
    net.free()
    assert name == "conv_direct_f32", name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def test_split_switches(workdir, monkeypatch):
    """Y2_WINO=1 Y2_WINO_SPLIT=1 names the layer conv_winox_f32_* and moves the launch counter; Y2_WINO=1 alone is the fp32
    Winograd form, Y2_WINO_SPLIT=0 and no switch at all (a grid this small is never taken by the rule) the direct kernel; the
    counter stands still for all three; integer data: the same bits every way"""
    spec = [("conv", 64, 3, 0, "linear"), ("conv", 96, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 19, 2, 44000)
    count = darknet.lib().y2h_wino_split_launches
    _env(monkeypatch, 1, 1, None, None)
    before = count()
    out, name = _predict(cfg, wts, x)
    assert name.startswith("conv_winox_f32_") and count() == before + 1, name
    _env(monkeypatch, 1, None, None, None)
    wino, wname = _predict(cfg, wts, x)
    assert wname.startswith("conv_wino_f32_"), wname
    _env(monkeypatch, None, 0, None, None)
    off, off_name = _predict(cfg, wts, x)
    _env(monkeypatch, None, None, None, None)
    plain, plain_name = _predict(cfg, wts, x)
    assert off_name == plain_name and off_name.startswith("conv_mfma_f32_") and off_name.endswith("_k3"), (off_name, plain_name)
    assert count() == before + 1
    assert np.array_equal(off, plain) and np.array_equal(wino, plain) and np.array_equal(out, plain)
