"""The fused stationary Winograd kernel of the shallow fp32 3x3 convolutions (y2_winos.hip, 32-channel form) against the CPU
oracle.

Forced on (Y2_WINOS=1) on layers far too small for the rule to take, its persistent grid capped at three workgroups
(Y2_CONV_GRID=3: a workgroup walks several patches, and image borders fall inside a patch halo).  B^T and A^T only add and
subtract and G g G^T of a small-integer filter is a multiple of 1/4, so on integer data every value is exact and the result
must EQUAL the oracle's (convolutional_layer.c:435-474, gemm.c:74-88, maxpool_layer.c:79-114 restated in
oracle/y2_oracle.c) -- and, behind batch-norm + leaky, the direct kernel's bits."""
import os
import struct

import numpy as np
import pytest

from sr_object_detection_amd import darknet, zoo
from tests.test_gpu_kernels import _small_int_conv_case

pytestmark = pytest.mark.gpu


def _env(monkeypatch, winos, grid=3, **more):
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        monkeypatch.delenv(k)
    for k, v in dict(more, Y2_WINOS=winos, Y2_CONV_GRID=grid).items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _predict(cfg, wts, x, layer=1, strict=False, half=False):
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    if strict:
        net.set_strict(True)
    if half:
        net.set_half(True)
    out = net.network_predict(x).copy()
    name = net.layer_kernel(layer)
    net.free()
    return out, name


def _oracle(oracle, cfg, wts, x):
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x).copy()
    on.close()
    return ref


def _name(pool):
    return "conv_winos_f32_c32" + ("+maxpool2" if pool else "")


# filters: 64 = two full filter tiles, 48 = the second partial, 20 = one partial tile (the second tile's waves idle);
# width x height: 32 x 32 = 2 x 4 patches per image, 48 x 48 = 3 x 6, 32 x 48 non-square; batch 2-5
SHAPES = [(64, 32, 32, 2), (64, 48, 48, 3), (64, 32, 48, 5), (48, 32, 32, 3), (48, 48, 48, 2), (48, 32, 48, 4),
          (20, 32, 32, 5), (20, 48, 48, 2), (20, 32, 48, 3)]


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_%dx%d_b%d" % s)
def test_winos_is_exact(oracle, workdir, monkeypatch, shape, pool):
    filters, w, h, batch = shape
    spec = [("conv", 32, 3, 0, "linear"), ("conv", filters, 3, 0, "linear")] + ([("max", 2, 2)] if pool else [])
    cfg, wts, x = _small_int_conv_case(workdir, spec, w, batch, 41000 + filters + 7 * w + 11 * h + 13 * batch + 1000 * pool, height=h)
    _env(monkeypatch, 1)
    before = darknet.lib().y2h_winos_launches()
    out, name = _predict(cfg, wts, x)
    assert name == _name(pool), name
    assert darknet.lib().y2h_winos_launches() > before
    ref = _oracle(oracle, cfg, wts, x)
    assert np.abs(ref).max() < 2 ** 20
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
def test_winos_batchnorm_leaky_equals_direct_and_oracle(oracle, workdir, monkeypatch, pool):
    """batch-norm + leaky with negative scales (under the pool: the minimum of the window is what the epilogue sees): the sums
    are exact integers either way, so the shared epilogue gives the direct kernel's bits, which are the oracle's"""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 48, 3, 1, "leaky")] + ([("max", 2, 2)] if pool else [])
    cfg, wts, x = _small_int_conv_case(workdir, spec, 48, 3, 42000 + pool, neg_scale=True, height=32)
    _env(monkeypatch, 1)
    out, name = _predict(cfg, wts, x)
    assert name == _name(pool), name
    _env(monkeypatch, 0)
    direct, dname = _predict(cfg, wts, x)
    assert not dname.startswith("conv_winos"), dname
    assert np.array_equal(out, direct)
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))
    assert (out < 0).any() and (out > 0).any()


def test_winos_writes_into_a_route_target(oracle, workdir, monkeypatch):
    """the layer reads its input from, and writes its output into, the buffer of the [route] that concatenates the two
    (ldx = ldy = 32 + 48 > filters; output channel offset 32)"""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 48, 3, 1, "leaky"), ("route", [-2, -1])]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 32, 2, 43000, neg_scale=True, height=48)
    _env(monkeypatch, 1)
    out, name = _predict(cfg, wts, x)
    assert name == _name(False), name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))


def test_winos_scalar_stores_when_ldy_is_not_a_multiple_of_4(oracle, workdir, monkeypatch):
    """the route's buffer is 6 + 44 channels wide and the layer's output starts at channel 6: neither ldy nor the pointer is
    16-byte aligned, so the outputs leave dword by dword"""
    spec = [("conv", 6, 1, 0, "linear"), ("conv", 32, 3, 0, "linear"), ("conv", 44, 3, 1, "leaky"), ("route", [-3, -1])]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 32, 3, 44000, neg_scale=True)
    _env(monkeypatch, 1)
    before = darknet.lib().y2h_winos_launches()
    out, name = _predict(cfg, wts, x, layer=2)
    assert name == _name(False), name
    assert darknet.lib().y2h_winos_launches() > before
    ref = _oracle(oracle, cfg, wts, x)
    assert out.size == 3 * 50 * 32 * 32 and np.abs(ref).max() < 2 ** 20
    assert np.array_equal(out, ref)


def test_winos_is_never_taken_in_strict_or_half_mode(oracle, workdir, monkeypatch):
    """strict mode keeps the reference-order direct kernel and half mode its fp16 kernel even with Y2_WINOS=1"""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 64, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 32, 2, 45000)
    _env(monkeypatch, 1, None)
    out, name = _predict(cfg, wts, x, strict=True)
    assert name == "conv_direct_f32", name
    assert np.array_equal(out, _oracle(oracle, cfg, wts, x))
    _env(monkeypatch, 0, None)
    _, half_off = _predict(cfg, wts, x, half=True)
    _env(monkeypatch, 1, None)
    _, half_on = _predict(cfg, wts, x, half=True)
    assert half_on == half_off and "f16" in half_on, (half_on, half_off)


def test_winos_switches(workdir, monkeypatch):
    """Y2_WINOS=1 names the layer conv_winos_f32_c32; with no switch a grid this small is never taken by the rule, and
    Y2_C32F_MIN_TILES=1 -- which lowers conv_c32_f32's threshold, not this rule's -- still gives conv_c32_f32_16x16"""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 64, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 32, 2, 46000)
    _env(monkeypatch, 1, None)
    out, name = _predict(cfg, wts, x)
    assert name == _name(False), name
    _env(monkeypatch, 0, None)
    off, off_name = _predict(cfg, wts, x)
    _env(monkeypatch, None, None)
    plain, plain_name = _predict(cfg, wts, x)
    assert off_name == plain_name and off_name.startswith("conv_mfma_f32_"), (off_name, plain_name)
    _env(monkeypatch, None, None, Y2_C32F_MIN_TILES=1)
    c32, c32_name = _predict(cfg, wts, x)
    assert c32_name == "conv_c32_f32_16x16", c32_name
    assert np.array_equal(off, plain) and np.array_equal(c32, plain)
    assert np.array_equal(out, plain)              # integer data: exact either way


def test_one_form_per_layer_split_beats_wino_beats_stationary(workdir, monkeypatch):
    """The layer of test_winos_switches is one all three Winograd rules find eligible (tests/test_conv_form_cpu.py).  With every
    switch on it runs as the split form, without Y2_WINO_SPLIT as fp32 Winograd, with Y2_WINOS alone as the stationary kernel:
    the name says so, exactly that form's launch counter moves, and on integer data every form gives the direct kernel's bits."""
    spec = [("conv", 32, 3, 0, "linear"), ("conv", 64, 3, 1, "leaky")]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 32, 2, 46000)
    lib = darknet.lib()
    counters = (lib.y2h_wino_split_launches, lib.y2h_wino_launches, lib.y2h_winos_launches)
    _env(monkeypatch, None, None)
    direct, direct_name = _predict(cfg, wts, x)
    assert direct_name.startswith("conv_mfma_f32_"), direct_name
    rows = [(dict(Y2_WINO=1, Y2_WINO_SPLIT=1), "conv_winox_f32_"), (dict(Y2_WINO=1), "conv_wino_f32_"), (dict(), "conv_winos_f32_c32")]
    for k, (more, prefix) in enumerate(rows):
        _env(monkeypatch, 1, None, **more)
        before = [c() for c in counters]
        out, name = _predict(cfg, wts, x)
        moved = [c() - b for c, b in zip(counters, before)]
        assert name.startswith(prefix), (more, name)
        assert [m > 0 for m in moved] == [j == k for j in range(3)], (more, name, moved)
        assert np.array_equal(out, direct), (more, name)


def test_winos_real_valued_layer_is_within_tolerance(oracle, workdir, monkeypatch):
    """real-valued data, 3 -> 32 -> 64 channels, 32x32, batch 2: within 1e-4 * max(1, |layer max|) of the oracle (whose own
    distance from the truth is its sequential fp32 k-sum); the direct kernel's error for the same case is printed beside it"""
    spec = [("conv", 32, 3, 1, "leaky"), ("conv", 64, 3, 1, "leaky")]
    layers = zoo.resolve(spec, 32, 32, 3)
    cfg = os.path.join(workdir, "winos_real.cfg")
    open(cfg, "w").write(zoo.cfg_text("x", 32, 32, 2, spec=spec))
    wts = os.path.join(workdir, "winos_real.weights")
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
    x = rng.normal(0, 1, (2, 3, 32, 32)).astype(np.float32)
    ref = _oracle(oracle, cfg, wts, x)
    _env(monkeypatch, 1, None)
    out, name = _predict(cfg, wts, x)
    assert name == _name(False), name
    _env(monkeypatch, 0, None)
    direct, dname = _predict(cfg, wts, x)
    assert dname.startswith("conv_mfma_f32_"), dname
    tol = 1e-4 * max(1.0, float(np.abs(ref).max()))
    err, derr = float(np.abs(out - ref).max()), float(np.abs(direct - ref).max())
    print("layer max %.3f: |winos - oracle| %.3g, |direct - oracle| %.3g, bound %.3g" % (np.abs(ref).max(), err, derr, tol))
    assert err <= tol
