"""The convolution forms tests/test_gpu_tiles.py does not reach, against the CPU oracle, bit for bit.

test_gpu_tiles.py pins the matrix-core tiles for 1x1 and 3x3 filters at stride 1.  What is left of y2_conv.hip is held to
the same standard here, on integer-valued weights and inputs without batch-norm and with linear activation, so that every
fp32 partial sum is exact in any order and the result must EQUAL the oracle's (convolutional_layer.c:435-474, gemm.c:74-88
restated in oracle/y2_oracle.c):

  1. the four 5x5 tiles (conv_mfma_kernel<.., 5>: the generic one-bit-per-tap mask), forced, several tiles per workgroup,
     split-K with range boundaries inside a filter's 25 taps, images smaller than the filter's reach;
  2. a.stride in the fp32 tile kernel (coordinate decode, a_off, the masks against a.W / a.H) on large and small tiles,
     with split-K and stream-K;
  3. conv_stem_kernel<NT> for NT = 1..4, K odd / even / a multiple of 16 (the zero-weight padding taps), 1, 3 and 4
     input channels, and the walk over several tiles per wave (Y2_CONV_GRID caps stem_launch's workgroups);
  4. conv_direct_kernel<XH> outside strict mode: what no fast kernel takes in fp32, and its three storage combinations
     in fp16 mode (fp32 in / half out, half in / half out, half in / fp32 out).

Every case states the kernel it expects by full name, and the oracle-side condition that makes equality meaningful:
fp32 |ref| < 2**22 (integers exact in fp32); half storage: what is stored in half <= 2048 where it is read again
(integers exact in half) and < 60000 where it is only written (no overflow; compared with the oracle rounded once to half).
A case is data (Case), so the conditions can be evaluated from the oracle alone, without a device."""
import zlib
from typing import NamedTuple

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests.test_gpu_kernels import _small_int_conv_case
from tests.test_gpu_tiles import TESTED_F32

pytestmark = pytest.mark.gpu

# every switch a case may set: cleared first, so that a case runs under exactly its own
SWITCHES = ("Y2_CONV_TILE", "Y2_CONV_GRID", "Y2_CONV_KSPLIT", "Y2_SKF", "Y2_SKF_WGS", "Y2_XCD_ORDER", "Y2_NO_C32F",
            "Y2_C32F_MIN_TILES", "Y2_NO_FIRST_NCHW", "Y2_F32_SCALAR_STORES")

STEM = "conv_stem_mfma_f32"
DIRECT32 = "conv_direct_f32"
DIRECT16 = "conv_direct_f16"


class Case(NamedTuple):
    ident: str
    spec: list              # zoo spec; ("conv", filters, size, bn, act, stride, pad flag)
    w: int
    h: int
    batch: int
    names: dict             # layer index -> the kernel name it must report
    env: dict = {}
    half: bool = False
    channels: int = 3
    neg_scale: bool = False
    padding0: int = -1      # >= 0: layer 0 gets `padding=` written out (its spec entry carries pad flag 0)
    pull: int = -1          # >= 0: compare this layer's output instead of the network's (an fp32 layer inside a half network)
    half_layers: tuple = ()  # half mode: layers whose half output is read again by the layer under test

    @property
    def seed(self):
        return 200000 + zlib.crc32(self.ident.encode()) % 100000


def _materialize(workdir, case):
    cfg, wts, x = _small_int_conv_case(workdir, case.spec, case.w, case.batch, case.seed, neg_scale=case.neg_scale,
                                       height=case.h, channels=case.channels)
    if case.padding0 >= 0:
        text = open(cfg).read()
        assert text.count("pad=0\n") >= 1
        open(cfg, "w").write(text.replace("pad=0\n", "pad=0\npadding=%d\n" % case.padding0, 1))
    return cfg, wts, x


def _as_half(a):
    return a.astype(np.float16).astype(np.float32)


def _reference(oracle, cfg, wts, x, case):
    """the oracle's result for the case, and the conditions under which the device must equal it"""
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    if case.pull >= 0:
        ref = on.layer_output(case.pull)
    stored = [np.abs(on.layer_output(i)).max() for i in case.half_layers]
    on.close()
    if case.half:
        assert all(m <= 2048 for m in stored), stored          # read again from half: exact
        if case.pull >= 0:
            assert np.abs(ref).max() < 2 ** 22                 # the fp32 output of a half network
        else:
            assert np.abs(ref).max() < 60000                   # written in half: no overflow
            ref = _as_half(ref)
    else:
        assert np.abs(ref).max() < 2 ** 22
    assert np.abs(ref).max() > 0
    return ref


def _device(monkeypatch, case, cfg, wts, x):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, str(v))
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    if case.half:
        net.set_half(True)
    out = net.network_predict(x)
    names = {i: net.layer_kernel(i) for i in case.names}
    if case.pull >= 0:
        out = net.pull_layer_output(case.pull)
    net.free()
    return out, names


def _check_exact(oracle, workdir, monkeypatch, case):
    cfg, wts, x = _materialize(workdir, case)
    ref = _reference(oracle, cfg, wts, x, case)
    out, names = _device(monkeypatch, case, cfg, wts, x)
    assert names == case.names, names
    assert out.shape == ref.shape
    assert np.array_equal(out, ref), "%d of %d values differ, max |d| = %g" % (
        int((out != ref).sum()), out.size, float(np.abs(out - ref).max()))


def _ids(cases):
    assert len({c.ident for c in cases}) == len(cases)
    return dict(argvalues=cases, ids=[c.ident for c in cases])


# ---------------------------------------------------------------------------
# the fp32 tile kernel: 5x5 filters and strides
# ---------------------------------------------------------------------------
def _tile_case(ident, tile, ks, cin, filters=None, w=26, h=26, batch=2, stride=1, ksplit=1, grid=3, bnorm=0, act="linear",
               pool=False, env=None, fused=False, neg_scale=False):
    bm, bn = tile
    filters = bn + 40 if filters is None else filters          # two filter tiles, the second partial
    spec = [("conv", cin, 3, 0, "linear"), ("conv", filters, ks, bnorm, act, stride)] + ([("max", 2, 2)] if pool else [])
    e = {"Y2_CONV_TILE": "%dx%d" % tile, "Y2_CONV_KSPLIT": ksplit}
    if grid:
        e["Y2_CONV_GRID"] = grid
    e.update(env or {})
    name = "conv_mfma_f32_%dx%dx%d_k%d" % (bm, bn, 32 if cin % 32 == 0 else 16, ks)
    assert name in TESTED_F32
    return Case(ident, spec, w, h, batch, {1: name + ("+maxpool2" if fused else "")}, e, neg_scale=neg_scale)


K5_TILES = [(128, 128, 32), (64, 64, 32), (128, 128, 16), (64, 64, 16)]       # g_variants, y2_conv.hip: (BM, BN, BK)
MASK_EDGES = [(1, 1), (2, 3), (5, 4), (11, 37)]                               # (h, w)

# 26x26 batch 2: 1352 GEMM rows, a partial last row tile, tiles that straddle the two images; three workgroups walk them
K5_CASES = [_tile_case("k5_%dx%dx%d" % t, t[:2], 5, 64 if t[2] == 32 else 48) for t in K5_TILES]
# 75 K-steps (25 taps x 96 / 32) in four ranges of 18 / 19 / 19 / 19: every boundary inside a filter's taps; BN + 37
# filters: no multiple of 4, the scalar partial-sum stores
K5_CASES += [_tile_case("k5_%dx%dx32_ksplit4" % t, t, 5, 96, w=19, h=19, batch=3, ksplit=4) for t in ((128, 128), (64, 64))]
K5_CASES += [_tile_case("k5_64x64x32_ksplit4_scalar_stores", (64, 64), 5, 96, filters=64 + 37, w=19, h=19, batch=3, ksplit=4)]
# images smaller than the filter's reach (a tap row / column outside on BOTH sides), and a non-square one whose masks
# differ if a.W and a.H are swapped (11 x 37: rows 0-1 and 9-10 against columns 0-1 and 35-36)
K5_CASES += [_tile_case("k5_64x64x32_image_%dx%d" % hw, (64, 64), 5, 64, w=hw[1], h=hw[0], batch=3) for hw in MASK_EDGES]
K5_CASES += [_tile_case("k3_64x64x32_image_%dx%d" % hw, (64, 64), 3, 64, w=hw[1], h=hw[0], batch=3) for hw in MASK_EDGES]


@pytest.mark.parametrize("case", **_ids(K5_CASES))
def test_5x5_tile_is_exact(oracle, workdir, monkeypatch, case):
    _check_exact(oracle, workdir, monkeypatch, case)


@pytest.mark.parametrize("tile", [(128, 128), (64, 64)], ids=lambda t: "%dx%d" % t)
def test_5x5_tile_with_batchnorm_leaky_epilogue(oracle, workdir, monkeypatch, tile):
    """batch-norm + leaky with alternating negative scales behind the 5x5 accumulator: the accumulator is exact, the epilogue's
    double reciprocal instead of the double divide may differ by one fp32 ulp -- the bound of
    test_f32_tile_with_batchnorm_leaky_epilogue"""
    case = _tile_case("k5_%dx%d_bn_leaky" % tile, tile, 5, 64, bnorm=1, act="leaky", neg_scale=True)
    cfg, wts, x = _materialize(workdir, case)
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    on.close()
    out, names = _device(monkeypatch, case, cfg, wts, x)
    assert names == case.names, names
    assert (ref < 0).any() and (ref > 0).any()
    assert np.abs(out - ref).max() <= np.abs(ref).max() * 2.0 ** -23
    assert (out != ref).mean() < 1e-3


# Non-square inputs, one extent odd and one even, batch 3.  Stride 2 on 27 x 22 (h x w) -> 14 x 11 outputs, 462 GEMM rows:
# the last row's bottom tap is outside (26 + 1 = H), the last column's right tap inside (20 + 1 < W).  Stride 3 on 26 x 19
# -> 9 x 7, 189 rows, 63 per image (a 64-row tile straddles two images): bottom inside (24 + 1 < H), right outside
# (18 + 1 = W).  Neither 462 nor 189 is a multiple of 64, 128 or 192.
STRIDE_INPUT = {2: (27, 22), 3: (26, 19)}
STRIDE_CASES = []
for _tile, _sizes in (((192, 256), (1, 3)), ((128, 128), (1, 3, 5)), ((64, 64), (1, 3, 5))):
    for _ks in _sizes:
        for _s in (2, 3):
            STRIDE_CASES.append(_tile_case("k%d_s%d_%dx%d" % ((_ks, _s) + _tile), _tile, _ks, 64, w=STRIDE_INPUT[_s][1],
                                           h=STRIDE_INPUT[_s][0], batch=3, stride=_s))
# the same inputs transposed (22 x 27 -> 11 x 14, 19 x 26 -> 7 x 9): the outside tap changes sides, so each stride meets
# a last row and a last column of both kinds
for _ks in (3, 5):
    for _s in (2, 3):
        STRIDE_CASES.append(_tile_case("k%d_s%d_64x64_transposed" % (_ks, _s), (64, 64), _ks, 64, w=STRIDE_INPUT[_s][0],
                                       h=STRIDE_INPUT[_s][1], batch=3, stride=_s))
STRIDE_CASES.append(_tile_case("k3_s2_128x128_bk16", (128, 128), 3, 48, w=22, h=27, batch=3, stride=2))
# 27 K-steps in three ranges of 9: the workspace rows follow the strided output grid
STRIDE_CASES.append(_tile_case("k3_s2_128x128_ksplit3", (128, 128), 3, 96, w=22, h=27, batch=3, stride=2, ksplit=3))


@pytest.mark.parametrize("case", **_ids(STRIDE_CASES))
def test_strided_tile_is_exact(oracle, workdir, monkeypatch, case):
    _check_exact(oracle, workdir, monkeypatch, case)


def test_strided_tile_stream_k_is_exact(oracle, workdir, monkeypatch):
    """3x3 stride 2 with the K loops of all 8 output tiles (4 x 2 of 128x128, 27 K-steps each) in equal shares over 11
    workgroups (a share may not exceed one tile, so at least as many workgroups as tiles; 216 / 11: shares that straddle
    tile boundaries), then sk_reduce_kernel"""
    case = _tile_case("k3_s2_128x128_stream_k", (128, 128), 3, 96, w=22, h=27, batch=3, stride=2, ksplit=0,
                      env={"Y2_SKF_WGS": 11})
    before = darknet.lib().y2h_f32_stream_k_launches()
    _check_exact(oracle, workdir, monkeypatch, case)
    assert darknet.lib().y2h_f32_stream_k_launches() > before


def test_strided_conv_in_front_of_maxpool_is_not_fused(oracle, workdir, monkeypatch):
    """mfma_ok refuses fuse_maxpool2 with stride != 1: a 3x3 stride-2 convolution with even output extents (27 x 24 ->
    14 x 12) in front of a 2x2/2 maxpool runs under the un-fused name, the maxpool as its own layer"""
    case = _tile_case("k3_s2_128x128_then_maxpool", (128, 128), 3, 64, w=24, h=27, batch=3, stride=2, pool=True)
    _check_exact(oracle, workdir, monkeypatch, case)


# ---------------------------------------------------------------------------
# the stem kernel
# ---------------------------------------------------------------------------
# (size, stride, pad flag, explicit padding or -1): K = 147, 363, 75, 27, 48, 12, 3 with 3 channels -- odd, even and a
# multiple of 16, so the K padding (taps k >= K re-read tap K - 1 with a zero weight) runs from 0 to 13 taps deep
GEOMETRY = {"7x7s2p3": (7, 2, 1, -1), "11x11s4p0": (11, 4, 0, -1), "5x5s1p2": (5, 1, 1, -1), "3x3s2p1": (3, 2, 1, -1),
            "4x4s2p1": (4, 2, 0, 1), "2x2s2p0": (2, 2, 0, -1), "1x1s1p0": (1, 1, 0, -1)}


def _stem_case(geo, filters, w, h, batch, channels=3, env=None, name=STEM, tag=""):
    size, stride, flag, padding = GEOMETRY[geo]
    ident = "%s_n%d_%dx%d_b%d_c%d%s" % (geo, filters, w, h, batch, channels, tag)
    return Case(ident, [("conv", filters, size, 0, "linear", stride, flag)], w, h, batch, {0: name}, env or {},
                channels=channels, padding0=padding)


# filters 20 / 64 / 100 / 128 = NT 1 / 2 / 3 / 4 (partial last tile at 20 and 100); every NT meets at least two geometries;
# odd, non-square inputs
STEM_CASES = [
    _stem_case("7x7s2p3", 20, 33, 21, 3), _stem_case("7x7s2p3", 64, 67, 59, 2), _stem_case("7x7s2p3", 100, 33, 21, 2),
    _stem_case("7x7s2p3", 128, 33, 21, 3),
    _stem_case("11x11s4p0", 20, 67, 59, 2), _stem_case("11x11s4p0", 64, 67, 59, 3), _stem_case("11x11s4p0", 96, 67, 59, 2),
    _stem_case("5x5s1p2", 64, 33, 21, 2), _stem_case("5x5s1p2", 128, 33, 21, 2),
    _stem_case("3x3s2p1", 20, 67, 59, 2), _stem_case("3x3s2p1", 100, 33, 21, 3), _stem_case("3x3s2p1", 128, 67, 59, 2),
    _stem_case("4x4s2p1", 64, 33, 21, 3), _stem_case("4x4s2p1", 100, 67, 59, 2),
    _stem_case("2x2s2p0", 20, 33, 21, 3), _stem_case("2x2s2p0", 128, 67, 59, 2),
    _stem_case("1x1s1p0", 64, 33, 21, 2), _stem_case("1x1s1p0", 100, 33, 21, 3),
    # 1 and 4 input channels (K = 49 / 196 / 9 / 36): the plan gives them to the stem kernel as well
    _stem_case("7x7s2p3", 64, 33, 21, 2, channels=1), _stem_case("7x7s2p3", 100, 33, 21, 2, channels=4),
    _stem_case("3x3s2p1", 20, 33, 21, 3, channels=1), _stem_case("3x3s2p1", 128, 33, 21, 2, channels=4),
]
# Several tiles per wave (Y2_CONV_GRID caps the workgroups: 4 or 12 waves).  A narrow output: 7 x 40 per image (27 tiles:
# four to five row wraps per 32-pixel step) and 7 x 3 = 21 pixels per image (14 tiles: an image wrap inside every step);
# a wide one: 75 x 11 (52 tiles: a step stays in one row or wraps once).
for _g in (1, 3):
    STEM_CASES += [_stem_case("3x3s2p1", 64, 13, 79, 3, env={"Y2_CONV_GRID": _g}, tag="_grid%d" % _g),
                   _stem_case("7x7s2p3", 20, 13, 5, 20, env={"Y2_CONV_GRID": _g}, tag="_grid%d" % _g),
                   _stem_case("3x3s2p1", 100, 149, 21, 2, env={"Y2_CONV_GRID": _g}, tag="_grid%d" % _g),
                   _stem_case("5x5s1p2", 128, 75, 11, 2, env={"Y2_CONV_GRID": _g}, tag="_grid%d" % _g)]
# The production launch path, no switch: 6 x 150 x 150 = 135 000 output pixels = 4219 tiles on 4 x 256 x 4 = 4096 waves,
# chunks of two tiles
STEM_CASES.append(_stem_case("3x3s2p1", 20, 300, 300, 6, tag="_natural_two_tile_chunks"))
# 11x11 with more than 96 filters: the tables of NT = 4 exceed the LDS, stem_ok refuses, the direct kernel takes the layer
STEM_CASES.append(_stem_case("11x11s4p0", 100, 67, 59, 2, name=DIRECT32, tag="_lds_refusal"))


@pytest.mark.parametrize("case", **_ids(STEM_CASES))
def test_stem_kernel_is_exact(oracle, workdir, monkeypatch, case):
    _check_exact(oracle, workdir, monkeypatch, case)


# ---------------------------------------------------------------------------
# the direct kernel outside strict mode
# ---------------------------------------------------------------------------
def _direct_case(ident, cin, conv, w, h, batch):
    return Case(ident, [("conv", cin, 3, 0, "linear"), ("conv",) + conv], w, h, batch, {1: DIRECT32})


DIRECT_F32_CASES = [
    _direct_case("k3_c24", 24, (40, 3, 0, "linear"), 21, 17, 2),                  # channels no multiple of 16
    _direct_case("k3_pad0_c32", 32, (40, 3, 0, "linear", 1, 0), 21, 17, 2),       # pad != size / 2
    _direct_case("k7_s2_c32", 32, (24, 7, 0, "linear", 2), 21, 17, 2),            # 7x7 with many channels
    _direct_case("k4_s2_c16", 16, (40, 4, 0, "linear", 2), 21, 17, 2),            # even sizes (pad = size / 2 and pad 0)
    _direct_case("k2_s2_pad0_c16", 16, (40, 2, 0, "linear", 2, 0), 21, 17, 2),
    _direct_case("k3_c24_odd_outputs", 24, (5, 3, 0, "linear"), 9, 7, 3),         # out_w * out_h * Cout = 315
    # 4 x 64 x 64 x 136 = 2 228 224 outputs on the 8192 x 256 threads the launch is capped at: the grid-stride loop
    _direct_case("k3_c24_grid_stride", 24, (136, 3, 0, "linear"), 64, 64, 4),
]


@pytest.mark.parametrize("case", **_ids(DIRECT_F32_CASES))
def test_direct_kernel_f32_is_exact(oracle, workdir, monkeypatch, case):
    _check_exact(oracle, workdir, monkeypatch, case)


_REGION = ("region", {"anchors": [1.0, 1.0, 2.0, 2.0], "classes": 3, "num": 2})        # 2 * (3 + 5) = 16 filters in front
DIRECT_F16_CASES = [
    # fp32 in / half out: a 7x7/2 stem as layer 0 of a half network (stem_ok refuses half output)
    Case("f32_in_half_out_k7_s2_stem", [("conv", 40, 7, 0, "linear", 2)], 33, 21, 2, {0: DIRECT32}, half=True,
         half_layers=(0,)),
    # half in / half out: what mfma_h_ok refuses -- strides, 5x5, channels no multiple of 32
    Case("half_in_half_out_k3_s2_c32", [("conv", 32, 3, 0, "linear"), ("conv", 40, 3, 0, "linear", 2)], 22, 27, 2,
         {1: DIRECT16}, half=True, half_layers=(0,)),
    Case("half_in_half_out_k5_c32", [("conv", 32, 3, 0, "linear"), ("conv", 37, 5, 0, "linear")], 21, 17, 2,
         {1: DIRECT16}, half=True, half_layers=(0,)),
    Case("half_in_half_out_k3_c24", [("conv", 24, 3, 0, "linear"), ("conv", 40, 3, 0, "linear")], 21, 17, 2,
         {1: DIRECT16}, half=True, half_layers=(0,)),
    # half in / fp32 out: the last convolution, in front of the region head
    Case("half_in_f32_out_k3_s2_c32", [("conv", 32, 3, 0, "linear"), ("conv", 16, 3, 0, "linear", 2), _REGION], 22, 27, 2,
         {1: DIRECT16}, half=True, half_layers=(0,), pull=1),
    Case("half_in_f32_out_k1_c24", [("conv", 24, 3, 0, "linear"), ("conv", 16, 1, 0, "linear"), _REGION], 21, 17, 2,
         {1: DIRECT16}, half=True, half_layers=(0,), pull=1),
]


@pytest.mark.parametrize("case", **_ids(DIRECT_F16_CASES))
def test_direct_kernel_half_storage_is_exact(oracle, workdir, monkeypatch, case):
    _check_exact(oracle, workdir, monkeypatch, case)


ALL_CASES = K5_CASES + STRIDE_CASES + STEM_CASES + DIRECT_F32_CASES + DIRECT_F16_CASES
