"""The direct split form (include/y2_splitd_rule.h) without a GPU: the filter packer through a stand-alone C program
(tests/splitd_pack_check.c, built with -fsanitize=address,undefined -- no Python in that process) against an index function
restated here, the shape gate, the switches, and the rule through y2h_conv_splitd_plan against its committed table."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "splitd_plan_table.txt")
SRC = os.path.join(ROOT, "tests", "splitd_pack_check.c")
CFLAGS = ["-ffp-contract=off", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    d = tmp_path_factory.mktemp("splitd")
    san = str(d / "pack_san")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + CFLAGS + [SRC, "-o", san, "-lm"], check=True)
    return san, d


@pytest.fixture(scope="module")
def pd():
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.the_lib = C.CDLL(os.path.join(ROOT, "sr_object_detection_amd", "libsr_yolo2.so"))
    return mod


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        monkeypatch.delenv(k)


def _bf16_rn(a):
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)        # finite values far from overflow only


def _bf16_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _index(c, bn, co, ci, tap, p):
    """where plane p of filter co, channel ci, tap 3 ky + kx lives: one run per (filter tile, K-tile of 16 channels, tap),
    inside it [plane][k-half][filter % bn][8 channels]"""
    run = ((co // bn) * (c // 16) + ci // 16) * 9 + tap
    return run * 48 * bn + ((p * 2 + (ci % 16) // 8) * bn + co % bn) * 8 + ci % 8


@pytest.mark.parametrize("c,n,bn", [(32, 36, 128), (96, 128, 128), (96, 168, 128), (64, 256, 256), (96, 296, 256), (16, 4, 256)])
def test_packer_layout_equals_index_function(packer, c, n, bn):
    """y2_splitd_pack_u == the reference-layout weights [n][c][3][3] themselves, split three ways, each plane's value at
    _index; everything else in the slot (the rows that fill the last filter tile) is zero"""
    path = str(packer[1] / ("u_%d_%d_%d.bin" % (c, n, bn)))
    subprocess.run([packer[0], str(c), str(n), str(bn), path], check=True)
    got = np.fromfile(path, dtype=np.uint16)
    i = np.arange(n * c * 9, dtype=np.uint64)
    w = ((((i * np.uint64(2654435761) + np.uint64(12345)) >> np.uint64(3)) & np.uint64(0xffffff)).astype(np.float64) / 16777216.0 - 0.5)
    w = w.astype(np.float32).reshape(n, c, 9)
    h = _bf16_rn(w)
    r1 = w - _bf16_f32(h)
    m = _bf16_rn(r1)
    r2 = r1 - _bf16_f32(m)
    assert not (r2.view(np.uint32) & 0xffff).any()
    l = (r2.view(np.uint32) >> 16).astype(np.uint16)
    assert m.any() and l.any()
    tiles = (n + bn - 1) // bn
    assert got.size == tiles * (c // 16) * 9 * 48 * bn
    want = np.zeros_like(got)
    co, ci, tap = np.meshgrid(np.arange(n), np.arange(c), np.arange(9), indexing="ij")
    for p, plane in enumerate((h, m, l)):
        idx = _index(c, bn, co, ci, tap, p)
        assert idx.max() < got.size
        want[idx.reshape(-1)] = plane.reshape(-1)
    assert np.array_equal(got, want)
    # a fragment read is contiguous: the 8 channels of a k-half, then the next filter, 16 bytes on
    assert _index(c, bn, 0, 1, 0, 0) == _index(c, bn, 0, 0, 0, 0) + 1 and _index(c, bn, 1, 0, 0, 0) == _index(c, bn, 0, 0, 0, 0) + 8


def test_rule_table_unchanged():
    """tools/plan_dump.py --splitd against the committed table; a deliberate change of the rule regenerates it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("Y2_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_dump.py"), "--splitd"], check=True, capture_output=True,
                         text=True, env=env).stdout
    assert out == open(TABLE).read(), "tools/plan_dump.py --splitd differs from tests/golden/splitd_plan_table.txt"


def _desc(pd, batch, h, w, c, n, pool=0, **kw):
    return dict(dict(batch=batch, h=h, w=w, c=c, ldx=c, n=n, size=3, stride=1, pad=1, out_h=h, out_w=w, ldy=n, fuse_maxpool2=pool,
                     batch_normalize=1, activation=1, x=0x10000, w_packed=0x20000, y=pd.ALIGNED, bias=0x40000), **kw)


def _with_env(env, fn):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return fn()
    finally:
        for k in env:
            del os.environ[k]


def test_rule_at_the_headline_configuration(pd):
    """yolo.cfg 608x608 batch 32: the rule takes layers 4 and 6 (pooled), 128 filters each, and leaves layers 8 and 10 (256
    filters: the direct 192x256 tile keeps its launches in that network, which tests/test_gpu_configs.py asks for) -- and
    through y2_conv_layer_form those two are the only layers of the network in this form, the Winograd range keeps its forms"""
    lib = pd.the_lib
    rows = {i: f for i, f in pd._descs("yolo", 608, 32, 0, pd.ALIGNED) if f["size"] == 3 and not f.get("x_halo") and not f.get("x_nchw")}
    plans = {i: pd.splitd_plan(lib, f) for i, f in rows.items()}
    assert [plans[i].take for i in (4, 6, 8, 10)] == [1, 1, 0, 0]
    assert [plans[i].eligible for i in (4, 6, 8, 10)] == [1, 1, 1, 1]
    assert [plans[i].bn for i in (4, 6, 8, 10)] == [128, 128, 256, 128]
    forms = {i: pd.layer_form(lib, f) for i, f in rows.items()}
    assert sorted(i for i, (form, _) in forms.items() if pd.FORM_NAMES[form] == "splitd") == [4, 6]
    assert forms[4][1] == "conv_splitd_f32_256x128x16" and forms[6][1] == "conv_splitd_f32_256x128x16+maxpool2"
    assert pd.FORM_NAMES[forms[8][0]] == pd.FORM_NAMES[forms[10][0]] == "direct"
    d8 = pd.Conv(**rows[8])
    lib.y2h_conv_variant.restype = C.c_char_p
    assert lib.y2h_conv_variant(C.byref(d8), 0) == b"conv_mfma_f32_192x256x32_k3"
    for i in (12, 14, 16, 18, 29):
        assert pd.FORM_NAMES[forms[i][0]] == "winox", (i, forms[i])
    for i in (4, 6):
        p = plans[i]
        assert p.splitd_cost == max(p.matrix_cost, p.byte_cost) and p.splitd_cost < 0.9 * p.direct_cost
    with_env = _with_env({"Y2_SPLITD": "1"}, lambda: [pd.layer_form(lib, rows[i])[1] for i in (8, 10)])
    assert with_env == ["conv_splitd_f32_256x256x16", "conv_splitd_f32_256x128x16+maxpool2"]


def test_rule_counts_whole_rounds_and_needs_one(pd):
    """below one round of tiles (256) nothing is taken, whatever the costs say; rounds are whole: 257 tiles cost two rounds"""
    lib = pd.the_lib
    small = _desc(pd, 1, 76, 76, 128, 128)              # 77 * 78 positions = 24 tiles
    p = pd.splitd_plan(lib, small)
    assert p.eligible == 1 and p.tiles == 24 and p.take == 0
    a, b = _desc(pd, 1, 255, 254, 64, 128), _desc(pd, 1, 255, 255, 64, 128)      # 256 * 256 = 65536 positions = 256 tiles; 257
    pa, pb = pd.splitd_plan(lib, a), pd.splitd_plan(lib, b)
    assert pa.eligible == 0                              # a patch of 256 + 2 * 257 positions does not fit LDS twice
    a, b = _desc(pd, 4, 127, 126, 64, 128), _desc(pd, 4, 127, 127, 64, 128)      # 4 * 128 * 128 = 65536 positions; 4 * 128 * 129
    pa, pb = pd.splitd_plan(lib, a), pd.splitd_plan(lib, b)
    assert (pa.eligible, pa.tiles, pb.eligible, pb.tiles) == (1, 256, 1, 258)
    assert pb.matrix_cost == 2 * pa.matrix_cost


def test_shape_gate_and_switches(pd):
    """3x3 stride 1 pad 1, fp32 in and out, c % 16 == 0, n % 4 == 0, ldx % 4 == 0; pooled: H and W even.
    Y2_SPLITD=0 / 1 force the form off / on for every eligible descriptor; Y2_SPLITD_TILE names the filter tile; a named fp32
    tile (Y2_CONV_TILE, a measured tile_bm) keeps the layer direct; no other plan query sees any of it"""
    lib = pd.the_lib
    plan = lambda f: pd.splitd_plan(lib, f)
    small, big = _desc(pd, 2, 5, 7, 32, 296), _desc(pd, 32, 152, 152, 64, 128)
    assert (plan(small).eligible, plan(small).take) == (1, 0) and plan(big).take == 1
    assert plan(dict(big, n=132, ldy=132)).take == 0          # a second filter tile: left to the direct kernel
    for f, bn in ((small, 256), (big, 128)):
        assert _with_env({"Y2_SPLITD": "0"}, lambda: plan(f)).take == 0
        w = _with_env({"Y2_SPLITD": "1"}, lambda: plan(f))
        assert (w.take, w.bm, w.bn, w.bk) == (1, 256, bn, 16)
        assert w.u_bytes == (f["n"] + bn - 1) // bn * (f["c"] // 16) * 9 * 96 * bn
        assert _with_env({"Y2_CONV_TILE": "128x128", "Y2_SPLITD": "1"}, lambda: plan(f)).eligible == 0
        assert _with_env({"Y2_SPLITD": "1"}, lambda: plan(dict(f, tile_bm=128, tile_bn=128))).eligible == 0
        w = _with_env({"Y2_SPLITD_TILE": "256x128", "Y2_SPLITD": "1"}, lambda: plan(f))
        assert (w.take, w.bn) == (1, 128) and w.tiles % ((f["n"] + 127) // 128) == 0
        assert _with_env({"Y2_SPLITD_TILE": "128x256", "Y2_SPLITD": "1"}, lambda: plan(f)).bn == bn        # not a tile: ignored
        assert _with_env({"Y2_SPLITD": "1"}, lambda: pd.wino_plan(lib, f)).take == pd.wino_plan(lib, f).take
        assert _with_env({"Y2_SPLITD": "1"}, lambda: pd.wino_split_plan(lib, f)).take == pd.wino_split_plan(lib, f).take
    for kw in (dict(x_f16=1, y_f16=1, alpha=0x50000, beta=0x60000), dict(y_f16=1), dict(stride=2, out_h=76, out_w=76), dict(size=1, pad=0),
               dict(c=40, ldx=40), dict(n=126, ldy=126), dict(ldx=66), dict(x_halo=1),
               dict(fuse_maxpool2=1, h=151, out_h=151), dict(x=0x10004)):
        w = _with_env({"Y2_SPLITD": "1"}, lambda: plan(dict(big, **kw)))
        assert w.eligible == 0 and w.take == 0, kw
    for kw in (dict(c=48, ldx=48), dict(fuse_maxpool2=1), dict(ldy=232), dict(ldy=130, y=pd.MISALIGNED), dict(n=4, ldy=4),
               dict(fuse_maxpool2=1, n=256, ldy=256)):
        assert _with_env({"Y2_SPLITD": "1"}, lambda: plan(dict(big, **kw))).take == 1, kw
    # the rule itself leaves every layer of more than 128 filters alone, pooled or not
    assert plan(dict(big, n=256, ldy=256)).take == 0 and plan(dict(big, n=256, ldy=256, fuse_maxpool2=1)).take == 0
    # the pooled form has the 128-wide filter tile only, whatever tile is forced: more filters are more tiles
    w = _with_env({"Y2_SPLITD_TILE": "256x256", "Y2_SPLITD": "1"}, lambda: plan(dict(big, fuse_maxpool2=1, n=256, ldy=256)))
    assert (w.take, w.bn) == (1, 128) and w.tiles % 2 == 0


def _table(name):
    """a rule table's fp32 / fp16 take columns by (net, size, batch, layer)"""
    rows = {}
    for line in open(os.path.join(ROOT, "tests", "golden", name)):
        if line.startswith("#"):
            continue
        key, shape, f32, f16 = [p.split() for p in line.split("|")]
        rows[(key[0], int(key[1]), int(key[2][1:]), int(key[3][1:]))] = (int(f32[1]), int(f16[1]), f32[2])
    return rows


def test_layer_form_is_the_winograd_form_or_this_rule(pd):
    """For every row of the committed tables, fp32 and fp16: y2_conv_layer_form answers what y2_conv_form_of answers wherever
    that is a Winograd form (nothing that runs in one moves), and where it says direct the direct split form exactly where
    splitd_plan_table.txt has take set, named after the table's tile and the row's pool"""
    lib, table = pd.the_lib, _table("splitd_plan_table.txt")
    direct, splitd = pd.FORM_NAMES.index("direct"), pd.FORM_NAMES.index("splitd")
    taken = moved = 0
    for net, size, batch in pd.wino_cases():
        for half in (0, 1):
            for i, f in pd._descs(net, size, batch, half, pd.ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                key = (net, size, batch, i)
                wform, wname = pd.conv_form(lib, f)
                form, name = pd.layer_form(lib, f)
                if wform != direct:
                    assert (form, name) == (wform, wname), (key, half)
                    moved += table[key][half]
                    continue
                assert form == (splitd if table[key][half] else direct), (key, half, form, name)
                if form == splitd:
                    taken += 1
                    assert name == "conv_splitd_f32_%s%s" % (table[key][2], "+maxpool2" if f["fuse_maxpool2"] else ""), (key, name)
                else:
                    assert name == "", (key, name)
    print("%d rows in the direct split form; %d rows this rule would take keep their Winograd form" % (taken, moved))
    assert taken > 0


SWITCHES = [
    (dict(Y2_SPLITD="1"), "splitd"),
    (dict(Y2_WINOS="1", Y2_SPLITD="1"), "winos"),                          # a Winograd form keeps the layer
    (dict(Y2_WINO="1", Y2_WINO_SPLIT="1", Y2_WINOS="1", Y2_SPLITD="1"), "winox"),
    (dict(Y2_WINO="0", Y2_SPLITD="1"), "splitd"),                          # no Winograd of any form: not a Winograd form
    (dict(Y2_SPLITD="0"), "direct"),
    (dict(), "direct"),
]


@pytest.mark.parametrize("pool", [0, 1], ids=["nopool", "pool"])
@pytest.mark.parametrize("env,want", SWITCHES, ids=lambda v: "+".join("%s=%s" % kv for kv in v.items()) or "none" if isinstance(v, dict) else None)
def test_layer_form_forced_switches(pd, monkeypatch, env, want, pool):
    """the one descriptor all four rules find eligible: batch 2, 32x32, 32 -> 64 channels"""
    f = dict(batch=2, h=32, w=32, c=32, ldx=32, n=64, size=3, stride=1, pad=1, out_h=32, out_w=32, ldy=64, fuse_maxpool2=pool,
             batch_normalize=1, activation=1, x=0x10000, w_packed=0x20000, y=pd.ALIGNED, bias=0x40000)
    lib = pd.the_lib
    assert pd.splitd_plan(lib, f).eligible == 1 and pd.winos_plan(lib, f).eligible == 1 and pd.wino_split_plan(lib, f).eligible == 1
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    form, name = pd.layer_form(lib, f)
    assert pd.FORM_NAMES[form] == want, (env, form, name)
    if want == "splitd":
        assert name == "conv_splitd_f32_256x128x16" + ("+maxpool2" if pool else ""), name
    if want == "direct":
        assert name == ""
