"""Every tile instantiation of the matrix-core convolutions against the CPU oracle, bit for bit.

The host picks a tile per layer from the grid size (pick_variant, y2_conv.hip; pick_h, y2_conv_f16.hip), so small
test networks only ever reach the small tiles.  Here each instantiated shape is FORCED (Y2_CONV_TILE) on a layer whose
pixel count and filter count are not multiples of the tile (partial edge tiles in both GEMM dimensions, tiles that
straddle two images), with the persistent grid capped (Y2_CONV_GRID) so that every workgroup walks several tiles and
the cross-tile prefetch of the staging side runs, with 1x1 and 3x3 filters, both K-slice depths, with and without the
fused 2x2 maxpool, and K-split for the tiles that use it.  Integer-valued data make every fp32 partial sum exact in
any order, so the result must EQUAL the oracle's (convolutional_layer.c:435-474, gemm.c:74-88 restated in
oracle/y2_oracle.c); the fp16 kernels must equal it rounded once to half.  The four 5x5 tiles, strides above 1, the stem
kernel and the direct kernel are held to the same standard in tests/test_gpu_conv_forms.py; the 5x5 names are listed here.

TESTED_F32 / TESTED_F16 are also what tests/test_gpu_configs.py holds the BASELINE workloads to: a kernel name the
benchmark times must be in these sets."""
import re

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests.test_gpu_kernels import _small_int_conv_case

pytestmark = pytest.mark.gpu

# (BM, BN): every fp32 instantiation of conv_mfma_kernel for 1x1 / 3x3 filters (g_variants, y2_conv.hip)
F32_TILES_BK32 = [(192, 256), (256, 128), (256, 64), (128, 128), (128, 64), (64, 64), (128, 32)]
F32_TILES_BK16 = [(128, 128), (128, 64), (64, 64), (128, 32)]
# fp16: (BM, BN, m16) -- g_variants_h, y2_conv_f16.hip
F16_TILES = [(256, 256, True), (256, 256, False), (256, 128, False), (256, 64, False), (128, 128, False), (128, 64, False),
             (64, 64, False)]

# (BM, BN): the 5x5 instantiations, at both K-slice depths; forced and compared in tests/test_gpu_conv_forms.py
F32_TILES_K5 = [(128, 128), (64, 64)]

TESTED_F32 = {"conv_mfma_f32_%dx%dx%d_k%d" % (bm, bn, bk, ks) for bk, tiles in ((32, F32_TILES_BK32), (16, F32_TILES_BK16))
              for (bm, bn) in tiles for ks in (1, 3)}
TESTED_F32 |= {"conv_mfma_f32_%dx%dx%d_k5" % (bm, bn, bk) for (bm, bn) in F32_TILES_K5 for bk in (32, 16)}
TESTED_F16 = {"conv_mfma_f16_%dx%dx%d_k%d" % (bm, bn, bk, ks) for (bm, bn, _) in F16_TILES for bk in (64, 32) for ks in (1, 3)}


def _as_half(a):
    return a.astype(np.float16).astype(np.float32)


def _run(oracle, workdir, monkeypatch, *, cin, filters, ksize, size, batch, tile, pool, half=False, no_m16=False,
         grid=3, ksplit=1, bn=0, act="linear", seed=0):
    spec = [("conv", cin, 3, 0, "linear"), ("conv", filters, ksize, bn, act)]
    if pool:
        spec.append(("max", 2, 2))
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 20000 + seed)
    monkeypatch.setenv("Y2_CONV_TILE", "%dx%d" % tile)
    if grid is None:
        monkeypatch.delenv("Y2_CONV_GRID", raising=False)
    else:
        monkeypatch.setenv("Y2_CONV_GRID", str(grid))
    monkeypatch.setenv("Y2_CONV_KSPLIT", str(ksplit))
    if no_m16:
        monkeypatch.setenv("Y2_NO_M16", "1")
    else:
        monkeypatch.delenv("Y2_NO_M16", raising=False)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    if half:
        net.set_half(True)
    out = net.network_predict(x)
    name = net.layer_kernel(1)
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    l0 = np.abs(on.layer_output(0)).max()
    net.free()
    on.close()
    return out, ref, name, l0


_seed = [0]


def _next_seed():
    _seed[0] += 1
    return _seed[0]


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("bk,tile", [(32, t) for t in F32_TILES_BK32] + [(16, t) for t in F32_TILES_BK16],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "bk%d" % v)
def test_f32_tile_is_exact(oracle, workdir, monkeypatch, bk, tile, ksize, pool):
    bm, bn = tile
    cin = 64 if bk == 32 else 48
    filters = bn + 40                       # two filter tiles, the second partial
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=cin, filters=filters, ksize=ksize, size=26, batch=2, tile=tile,
                             pool=pool, seed=bm * 7 + bn * 3 + bk + ksize * 100 + pool * 1000)
    assert name == "conv_mfma_f32_%dx%dx%d_k%d%s" % (bm, bn, bk, ksize, "+maxpool2" if pool else ""), name
    assert name.split("+")[0] in TESTED_F32
    assert np.abs(ref).max() < 2 ** 22
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("tile", F32_TILES_BK32, ids=lambda t: "%dx%d" % t)
def test_f32_tile_split_k_is_exact(oracle, workdir, monkeypatch, tile, pool):
    """the K loop of a tile cut into four uneven ranges (27 slices of a 3x3x96 filter -> 6/7/7/7), partial sums through
    the workspace, splitk_reduce_kernel -- which also takes the fused 2x2 maxpool (pool-major GEMM rows: max over the four
    epilogue results of a window)"""
    bm, bn = tile
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=96, filters=bn + 24, ksize=3, size=20 if pool else 19, batch=3,
                             tile=tile, pool=pool, ksplit=4, seed=5000 + bm + bn + pool)
    assert name == "conv_mfma_f32_%dx%dx32_k3%s" % (bm, bn, "+maxpool2" if pool else ""), name
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("wgs", [23, 18, 20, 64, 200])
@pytest.mark.parametrize("tile", [(192, 256), (128, 128)], ids=lambda t: "%dx%d" % t)
def test_f32_stream_k_is_exact(oracle, workdir, monkeypatch, tile, wgs, pool):
    """conv_mfma_kernel<..., SKM> forced (Y2_SKF_WGS): the K loops of ALL output tiles (12 of 192x256, 18 of 128x128; 27 K-steps
    each) dealt in equal contiguous shares to `wgs` workgroups -- shares that straddle tile boundaries (23), whole tiles (18
    on the 128x128 tile), shares of a few K-steps (64, 200: several workgroups per tile) -- raw sums to tile-local piece
    slots, sk_reduce_kernel adds a tile's pieces in K order, pools and applies the epilogue.  Exact against the oracle on
    integer data (convolutional_layer.c:435-474, gemm.c:74-88, maxpool_layer.c:79-114)"""
    bm, bn = tile
    size = 20 if pool else 19
    tiles = -(-3 * size * size // bm) * -(-(bn + 24) // bn)
    if tiles > wgs:
        pytest.skip("a share may not exceed one tile: %d tiles on %d workgroups" % (tiles, wgs))
    monkeypatch.setenv("Y2_SKF_WGS", str(wgs))
    before = darknet.lib().y2h_f32_stream_k_launches()
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=96, filters=bn + 24, ksize=3, size=20 if pool else 19, batch=3,
                             tile=tile, pool=pool, ksplit=0, seed=5200 + bm + bn + pool + wgs)
    assert name == "conv_mfma_f32_%dx%dx32_k3%s" % (bm, bn, "+maxpool2" if pool else ""), name
    assert darknet.lib().y2h_f32_stream_k_launches() > before
    assert np.array_equal(out, ref)


def test_f32_stream_k_with_batchnorm_leaky_equals_split_k(oracle, workdir, monkeypatch):
    """the reduce pass runs the reference's epilogue arithmetic (epilogue_f32 / pool_pick) like splitk_reduce_kernel: on
    integer data, batch-norm + leaky with negative scales, the same bits as the integer split"""
    outs = []
    for mode in ("sk", "split"):
        if mode == "sk":
            monkeypatch.setenv("Y2_SKF_WGS", "23")
        else:
            monkeypatch.delenv("Y2_SKF_WGS", raising=False)
            monkeypatch.setenv("Y2_SKF", "0")
        spec = [("conv", 96, 3, 0, "linear"), ("conv", 152, 3, 1, "leaky"), ("max", 2, 2)]
        cfg, wts, x = _small_int_conv_case(workdir, spec, 20, 3, 5300, neg_scale=True)
        monkeypatch.setenv("Y2_CONV_TILE", "128x128")
        monkeypatch.setenv("Y2_CONV_KSPLIT", "0" if mode == "sk" else "3")
        net = darknet.Network.parse_network_cfg(cfg)
        net.load_weights(wts)
        outs.append(net.network_predict(x).copy())
        net.free()
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0] < 0).any() and (outs[0] > 0).any()


@pytest.mark.parametrize("tile", [(192, 256), (128, 128), (64, 64)], ids=lambda t: "%dx%d" % t)
def test_f32_split_k_scalar_store_fallback_is_exact(oracle, workdir, monkeypatch, tile):
    """a filter count that is no multiple of 4: the partial sums take the scalar store path instead of the 16-byte one"""
    bm, bn = tile
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=96, filters=bn + 37, ksize=3, size=19, batch=3,
                             tile=tile, pool=False, ksplit=3, seed=5500 + bm + bn)
    assert name == "conv_mfma_f32_%dx%dx32_k3" % (bm, bn), name
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("tile", F32_TILES_BK32, ids=lambda t: "%dx%d" % t)
def test_f32_tile_with_batchnorm_leaky_epilogue(oracle, workdir, monkeypatch, tile, pool):
    """the epilogue copy compiled with batch-norm + leaky as constants (every conv of the BASELINE cfgs but the last):
    same exact accumulator, epilogue arithmetic as blas.c:122 / convolutional_layer.c:407-419 / activations.h:41 -- the
    double reciprocal instead of the double divide may differ by one fp32 ulp"""
    bm, bn = tile
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=64, filters=bn + 40, ksize=3, size=26, batch=2, tile=tile,
                             pool=pool, bn=1, act="leaky", seed=9000 + bm + bn + pool)
    assert name.startswith("conv_mfma_f32_%dx%dx32_k3" % (bm, bn)), name
    assert np.abs(out - ref).max() <= np.abs(ref).max() * 2.0 ** -23
    assert (out != ref).mean() < 1e-3


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("bk", [64, 32])
@pytest.mark.parametrize("tile", F16_TILES, ids=lambda t: "%dx%d%s" % (t[0], t[1], "_m16" if t[2] else ""))
def test_f16_tile_is_exact(oracle, workdir, monkeypatch, tile, bk, ksize, pool):
    bm, bn, m16 = tile
    cin = 64 if bk == 64 else 96
    filters = bn + 40                       # a multiple of 8: the 16-byte store path (required by the 16x16x32 variant)
    out, ref, name, l0 = _run(oracle, workdir, monkeypatch, cin=cin, filters=filters, ksize=ksize, size=26, batch=2,
                              tile=(bm, bn), pool=pool, half=True, no_m16=not m16,
                              seed=30000 + bm * 7 + bn * 3 + bk + ksize * 100 + pool * 1000 + m16)
    assert name == "conv_mfma_f16_%dx%dx%d_k%d%s" % (bm, bn, bk, ksize, "+maxpool2" if pool else ""), name
    assert name.split("+")[0] in TESTED_F16
    assert l0 <= 2048 and np.abs(ref).max() < 60000          # layer 0 exact in half, no overflow
    assert np.array_equal(out, _as_half(ref))


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("bk", [64, 32])
def test_f16_register_staged_256x256_m16_is_exact(oracle, workdir, monkeypatch, bk, ksize, pool):
    """the register-staged 16x16x32 form of the 256x256 tile (conv_mfma_f16_kernel<256, 256, ..., M16 = true>): what runs
    when the LDS-DMA kernel is switched off (Y2_F16_NO_P8, the A/B switch of profiles/r02_notes.md) and, at BK = 32, the
    only 16x16x32 form there is"""
    monkeypatch.setenv("Y2_F16_NO_P8", "1")
    out, ref, name, l0 = _run(oracle, workdir, monkeypatch, cin=64 if bk == 64 else 96, filters=296, ksize=ksize, size=26, batch=2,
                              tile=(256, 256), pool=pool, half=True, seed=33000 + bk + ksize * 100 + pool * 1000)
    assert name == "conv_mfma_f16_256x256x%d_k%d%s" % (bk, ksize, "+maxpool2" if pool else ""), name
    assert l0 <= 2048 and np.abs(ref).max() < 60000
    assert np.array_equal(out, _as_half(ref))


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("tile", [t for t in F16_TILES if not t[2]], ids=lambda t: "%dx%d" % (t[0], t[1]))
def test_f16_tile_scalar_store_path_is_exact(oracle, workdir, monkeypatch, tile, pool):
    """a filter count that is not a multiple of 8 takes the 2-byte store epilogue"""
    bm, bn, _ = tile
    out, ref, name, l0 = _run(oracle, workdir, monkeypatch, cin=64, filters=bn + 37, ksize=3, size=26, batch=2,
                              tile=(bm, bn), pool=pool, half=True, seed=40000 + bm + bn + pool)
    assert name.startswith("conv_mfma_f16_%dx%dx64_k3" % (bm, bn)), name
    assert np.array_equal(out, _as_half(ref))


# (tail tiles cut along K, workgroups sharing them, persistent grid): 12 output tiles of 256x256 (6 x 2, partial in both
# dimensions).  5/7/7: one whole tile per workgroup behind its share, shares of 12.9 K-tiles that straddle tile boundaries;
# 3/3/5: shares of exactly one tile (a tile fixed up from a single piece), two workgroups without a share; 12/13/13: no whole
# tile at all; 2/7/7 and 7/7/7: more workgroups than K-tiles in the 1x1 cases (empty shares)
SK_CASES = [(5, 7, 7), (3, 3, 5), (12, 13, 13), (2, 7, 7), (7, 7, 7)]


@pytest.mark.parametrize("grid", [16, 40])
@pytest.mark.parametrize("pblk", [1, 3, 100])
@pytest.mark.parametrize("tile,filters", [((64, 64), 64 * 20 + 40), ((128, 128), 128 * 10 + 24), ((192, 256), 256 * 9 + 40)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "n%d" % v)
def test_f32_xcd_grouped_tile_order_is_exact(oracle, workdir, monkeypatch, tile, filters, pblk, grid):
    """wide 1x1 heads (yolo9000's 28 269-filter layer, cfg/yolo9000.cfg:198-218): tiles are dealt per XCD -- workgroups with
    the same b % 8 own filter tiles x, x + 8, ... and walk them in blocks of `pblk` pixel tiles -- instead of filter-tile
    fastest.  Every tile must still be computed exactly once: equal to the oracle on integer data, with 10 / 11 / 21 filter
    tiles (uneven over the eight XCDs), a partial last pixel block and more than one tile per workgroup."""
    monkeypatch.setenv("Y2_XCD_ORDER", "1")
    monkeypatch.setenv("Y2_XCD_PBLK", str(pblk))
    before = darknet.lib().y2h_xcd_order_launches()
    out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=64, filters=filters, ksize=1, size=26, batch=2, tile=tile,
                             pool=False, grid=grid, seed=80000 + tile[0] + pblk * 7 + grid)
    assert name == "conv_mfma_f32_%dx%dx32_k1" % tile, name
    assert darknet.lib().y2h_xcd_order_launches() > before
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ksize,cin", [(3, 128), (1, 256), (1, 64)], ids=["k3_nk18", "k1_nk4", "k1_nk1"])
@pytest.mark.parametrize("sk", SK_CASES, ids=lambda c: "sk%d_wg%d_grid%d" % c)
def test_f16_stream_k_is_exact(oracle, workdir, monkeypatch, sk, ksize, cin, pool):
    """conv_p8_f16_kernel with stream-K forced (Y2_SK_TILES / Y2_SK_WGS): the tail tiles' K loops are dealt to the
    workgroups in equal contiguous shares, every share leaves one or two pieces of raw fp32 sums in the workspace and
    conv_p8_fixup_kernel adds a tile's pieces in K order and applies the epilogue (also the fused 2x2 maxpool).  Integer
    data: the sums are exact in any order, so the result must EQUAL the oracle's rounded once to half
    (convolutional_layer.c:435-474, gemm.c:74-88)."""
    tiles, wgs, grid = sk
    monkeypatch.setenv("Y2_SK_TILES", str(tiles))
    monkeypatch.setenv("Y2_SK_WGS", str(wgs))
    before = darknet.lib().y2h_stream_k_launches()
    out, ref, name, l0 = _run(oracle, workdir, monkeypatch, cin=cin, filters=256 + 40, ksize=ksize, size=26, batch=2,
                              tile=(256, 256), pool=pool, half=True, grid=grid,
                              seed=70000 + tiles * 31 + wgs * 7 + grid + ksize * 100 + cin + pool * 1000)
    assert name == "conv_mfma_f16_256x256x64_k%d%s" % (ksize, "+maxpool2" if pool else ""), name
    assert darknet.lib().y2h_stream_k_launches() > before          # the split really ran
    assert l0 <= 2048 and np.abs(ref).max() < 60000
    assert np.array_equal(out, _as_half(ref))


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("ntail", [5, 2, 12], ids=lambda n: "tail%d" % n)
@pytest.mark.parametrize("tile", [(256, 128), (256, 64), (128, 128), (128, 64), (64, 64)], ids=lambda t: "%dx%d" % t)
def test_f16_small_tile_tail_is_exact(oracle, workdir, monkeypatch, tile, ntail, ksize, pool):
    """the other way to finish a partial last round of the 256x256 kernel: the tail tiles' GEMM rows go to a second launch
    of a smaller register-staged tile (ConvK.row0).  12 tiles of 256x256 (6 x 2): 5 -> 6 tail tiles (the whole-tile part
    must end on a row boundary: rows 768..1351 x 296 filters), 2 (the last, partial row tile only), 12 (nothing left for
    the 256x256 kernel).  Exact against the oracle on integer data (convolutional_layer.c:435-474, gemm.c:74-88)."""
    monkeypatch.setenv("Y2_TAIL_TILES", str(ntail))
    monkeypatch.setenv("Y2_TAIL_TILE", "%dx%d" % tile)
    L = darknet.lib()
    before = L.y2h_tail_launches()
    out, ref, name, l0 = _run(oracle, workdir, monkeypatch, cin=128, filters=256 + 40, ksize=ksize, size=26, batch=2,
                              tile=(256, 256), pool=pool, half=True, grid=4,
                              seed=72000 + tile[0] * 3 + tile[1] + ntail * 17 + ksize * 100 + pool * 1000)
    assert name == "conv_mfma_f16_256x256x64_k%d%s" % (ksize, "+maxpool2" if pool else ""), name
    assert L.y2h_tail_launches() > before
    assert l0 <= 2048 and np.abs(ref).max() < 60000
    assert np.array_equal(out, _as_half(ref))


def test_f16_stream_k_equals_whole_tiles_with_batchnorm_leaky(oracle, workdir, monkeypatch):
    """the fix-up launch takes the same epilogue code as the kernel's own (p8_epilogue_quadrant): batch-norm + leaky on
    integer data gives the same bits with and without the split"""
    outs = []
    for tiles in (0, 5):
        if tiles:
            monkeypatch.setenv("Y2_SK_TILES", str(tiles))
            monkeypatch.setenv("Y2_SK_WGS", "7")
        else:
            monkeypatch.setenv("Y2_SK", "0")
        out, ref, name, _ = _run(oracle, workdir, monkeypatch, cin=128, filters=296, ksize=3, size=26, batch=2, tile=(256, 256),
                                 pool=True, half=True, grid=7, bn=1, act="leaky", seed=71000)
        monkeypatch.delenv("Y2_SK", raising=False)
        outs.append(out.copy())
    assert np.array_equal(outs[0], outs[1])
    assert np.abs(outs[0] - ref).max() <= np.abs(ref).max() * 2.0 ** -9


@pytest.mark.parametrize("tile", [(192, 256), (128, 128), (64, 64)], ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("ksplit", [1, 3])
def test_pooled_epilogue_with_negative_scales(oracle, workdir, monkeypatch, tile, ksplit):
    """conv + 2x2 maxpool evaluates the epilogue ONCE per window, on the max (scale >= 0) or the min (scale < 0) of the
    four accumulators: the epilogue is monotone, so this equals max over four evaluations exactly
    (maxpool_layer.c:79-114 behind convolutional_layer.c:435-474)"""
    bm, bn = tile
    spec = [("conv", 64, 3, 0, "linear"), ("conv", bn + 40, 3, 1, "leaky"), ("max", 2, 2)]
    cfg, wts, x = _small_int_conv_case(workdir, spec, 26, 2, 61000 + bm + bn + ksplit, neg_scale=True)
    monkeypatch.setenv("Y2_CONV_TILE", "%dx%d" % tile)
    monkeypatch.setenv("Y2_CONV_GRID", "3")
    monkeypatch.setenv("Y2_CONV_KSPLIT", str(ksplit))
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    outs = []
    for fuse in (True, False):
        net = darknet.Network.parse_network_cfg(cfg)
        net.load_weights(wts)
        net.set_fusion(fuse)
        outs.append(net.network_predict(x).copy())
        assert ("+maxpool2" in net.layer_kernel(1)) == fuse
        net.free()
    on.close()
    assert np.array_equal(outs[0], outs[1])                       # fused == conv then maxpool, bit for bit
    assert np.abs(outs[0] - ref).max() <= np.abs(ref).max() * 2.0 ** -23
    assert (ref < 0).any() and (ref > 0).any()


@pytest.mark.parametrize("direct", [True, False], ids=["nchw", "halo"])
def test_first_layer_pooled_epilogue_with_negative_scales(oracle, workdir, monkeypatch, direct):
    """the 3-channel first-layer kernel (conv_first_kernel, pipelined batch-norm + leaky copy and generic copy), reading
    the NCHW network input itself (border taps masked per tile; 38 = a size that is no multiple of the 32-pixel tile) and
    in its older form behind the NHWC + halo transform: the same bits"""
    if direct:
        monkeypatch.delenv("Y2_NO_FIRST_NCHW", raising=False)
    else:
        monkeypatch.setenv("Y2_NO_FIRST_NCHW", "1")
    for act, size in (("leaky", 40), ("linear", 40), ("leaky", 38)):
        spec = [("conv", 32, 3, 1, act), ("max", 2, 2)]
        cfg, wts, x = _small_int_conv_case(workdir, spec, size, 3, 62000 + len(act) + size, neg_scale=True)
        on = oracle.OracleNet(cfg, wts)
        ref = on.predict(x)
        outs = []
        for fuse in (True, False):
            net = darknet.Network.parse_network_cfg(cfg)
            net.load_weights(wts)
            net.set_fusion(fuse)
            outs.append(net.network_predict(x).copy())
            want = "conv_first_mfma_f32_nchw_c3_n32" if direct else "conv_first_mfma_f32_c3_n32"
            assert net.layer_kernel(0) == want + ("+maxpool2" if fuse else ""), net.layer_kernel(0)
            net.free()
        on.close()
        assert np.array_equal(outs[0], outs[1])
        assert np.abs(outs[0] - ref).max() <= np.abs(ref).max() * 2.0 ** -23


def test_first_layer_from_nchw_is_exact_on_integer_data(oracle, workdir, monkeypatch):
    """fp32 first layer without batch-norm on integer data: every border tap masked correctly <=> equal to the oracle"""
    monkeypatch.delenv("Y2_NO_FIRST_NCHW", raising=False)
    for filters, size, batch in ((32, 38, 2), (48, 33, 3), (16, 64, 1)):
        spec = [("conv", filters, 3, 0, "linear")]
        cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 63000 + filters + size)
        net = darknet.Network.parse_network_cfg(cfg)
        net.load_weights(wts)
        out = net.network_predict(x)
        assert net.layer_kernel(0).startswith("conv_first_mfma_f32_nchw_c3_n")
        net.free()
        on = oracle.OracleNet(cfg, wts)
        ref = on.predict(x)
        on.close()
        assert np.array_equal(out, ref)


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("filters,size", [(32, 40), (64, 36), (24, 20), (20, 24), (32, 132)])
def test_f16_first_layer_reads_the_nchw_input(oracle, workdir, monkeypatch, filters, size, pool):
    """fp16 mode, first layer straight from the fp32 NCHW network input (conv_first_nchw_f16_kernel: bands of eight rows
    staged in LDS; 36 and 20 end in a partial band, 132 has two 64-lane passes per staged row and partial tiles at the
    row end, 64 filters = two MFMA column tiles): exact against the oracle on integer data, and bit-identical to the
    two-kernel form (input transform + conv_first_f16_kernel) with batch-norm + leaky"""
    for bn, act in ((0, "linear"), (1, "leaky")):
        spec = [("conv", filters, 3, bn, act)] + ([("max", 2, 2)] if pool else [])
        cfg, wts, x = _small_int_conv_case(workdir, spec, size, 3, 64000 + filters + size + pool + bn, neg_scale=bool(bn))
        outs = []
        for direct in (True, False):
            if direct:
                monkeypatch.delenv("Y2_NO_FIRST_NCHW", raising=False)
            else:
                monkeypatch.setenv("Y2_NO_FIRST_NCHW", "1")
            net = darknet.Network.parse_network_cfg(cfg)
            net.load_weights(wts)
            net.set_half(True)
            outs.append(net.network_predict(x).copy())
            want = "conv_first_mfma_f16_nchw_c3_n%d" % (32 if filters <= 32 else 64) if direct else "conv_first_mfma_f16_c3_n%d" % (32 if filters <= 32 else 64)
            assert net.layer_kernel(0) == want + ("+maxpool2" if pool else ""), net.layer_kernel(0)
            net.free()
        assert np.array_equal(outs[0], outs[1])
        on = oracle.OracleNet(cfg, wts)
        ref = on.predict(x)
        on.close()
        if not bn:
            assert np.abs(ref).max() < 60000
            assert np.array_equal(outs[0], _as_half(ref))
        else:
            assert np.abs(outs[0] - ref).max() <= np.abs(ref).max() * 2.0 ** -10


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("filters,size,batch", [(64, 48, 3), (48, 32, 5), (20, 64, 2)])
def test_f32_c32_weights_stationary_kernel_is_exact(oracle, workdir, monkeypatch, filters, size, batch, pool):
    """conv_c32_f32_kernel (3x3, 32 input channels, <= 64 filters in fp32: weights in registers, 18x18 input patch in LDS,
    2x16 pixel strips in pool-major order, v_mfma_f32_32x32x2_f32 with the k pairing of the generic kernel): exact against the
    oracle on integer data with and without the fused 2x2 maxpool, full / partial / single filter tile, several tiles per
    workgroup, image borders inside the patch halo (convolutional_layer.c:435-474, maxpool_layer.c:79-114).  With batch-norm
    + leaky and negative scales: the same bits as the generic tile kernel (same accumulator on integer data, same
    epilogue_f32 / pool_pick arithmetic)"""
    monkeypatch.setenv("Y2_C32F_MIN_TILES", "1")
    monkeypatch.setenv("Y2_CONV_GRID", "4")
    monkeypatch.delenv("Y2_CONV_TILE", raising=False)
    spec = [("conv", 32, 3, 0, "linear"), ("conv", filters, 3, 0, "linear")] + ([("max", 2, 2)] if pool else [])
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 85000 + filters + size + pool)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    out = net.network_predict(x)
    assert net.layer_kernel(1) == "conv_c32_f32_16x16" + ("+maxpool2" if pool else ""), net.layer_kernel(1)
    net.free()
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    on.close()
    assert np.abs(ref).max() < 2 ** 22
    assert np.array_equal(out, ref)
    spec = [("conv", 32, 3, 0, "linear"), ("conv", filters, 3, 1, "leaky")] + ([("max", 2, 2)] if pool else [])
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, batch, 85500 + filters + size + pool, neg_scale=True)
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("Y2_NO_C32F", "1")
        else:
            monkeypatch.delenv("Y2_NO_C32F", raising=False)
        net = darknet.Network.parse_network_cfg(cfg)
        net.load_weights(wts)
        outs.append(net.network_predict(x).copy())
        assert net.layer_kernel(1).startswith("conv_c32_f32") != off, net.layer_kernel(1)
        net.free()
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0] < 0).any() and (outs[0] > 0).any()


def test_kernel_name_pattern():
    for n in sorted(TESTED_F32 | TESTED_F16):
        assert re.fullmatch(r"conv_mfma_f(32|16)_\d+x\d+x\d+_k[135]", n)
