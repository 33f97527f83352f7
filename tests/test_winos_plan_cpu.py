"""The stationary-Winograd rule (include/y2_winos_rule.h, asked through y2h_winos_plan) is host arithmetic: which layers it takes
can be checked without a GPU.  The committed table pins its answer for every 3x3 layer of every zoo network at batch 1 / 8 /
32 / 128; the other tests state what the table must keep saying."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "winos_plan_table.txt")


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


def _rows():
    rows = {}
    for line in open(TABLE):
        if line.startswith("#"):
            continue
        key, shape, f32, f16 = [p.split() for p in line.split("|")]
        rows[(key[0], int(key[1]), int(key[2][1:]), int(key[3][1:]))] = dict(
            shape=[int(v) for v in shape], eligible=int(f32[0]), take=int(f32[1]), form=int(f32[2]), f16_eligible=int(f16[0]), f16_take=int(f16[1]))
    return rows


def _desc(pd, batch, h, w, n, pool=0, **kw):
    return dict(dict(batch=batch, h=h, w=w, c=32, ldx=32, n=n, size=3, stride=1, pad=1, out_h=h, out_w=w, ldy=n, fuse_maxpool2=pool,
                     batch_normalize=1, activation=1, x=0x10000, w_packed=0x20000, y=pd.ALIGNED, bias=0x40000), **kw)


def test_rule_table_unchanged():
    """tools/plan_dump.py --winos against the committed table; a deliberate change of the rule regenerates it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("Y2_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_dump.py"), "--winos"], check=True, capture_output=True,
                         text=True, env=env).stdout
    assert out == open(TABLE).read(), "tools/plan_dump.py --winos differs from tests/golden/winos_plan_table.txt"


def test_headline_layer():
    """yolo.cfg 608x608 batch 32: layer 2 (304x304, 32 -> 64 + pool) is taken and nothing else"""
    rows = _rows()
    taken = sorted(i for (net, size, b, i), r in rows.items() if (net, size, b) == ("yolo", 608, 32) and r["take"])
    assert taken == [2], taken
    assert rows[("yolo", 608, 32, 2)]["form"] == 32


def test_small_grids_are_left_alone(pd):
    """no layer of a detector at batch 1 is taken, and neither are the shapes the GPU tests force with Y2_WINOS=1 -- which that
    switch, and only that switch, turns on (Y2_WINO=1 and Y2_C32F_MIN_TILES=1 do not)"""
    rows = _rows()
    assert not [k for k, r in rows.items() if k[2] == 1 and r["take"] and k[0] in ("yolo", "yolo9000", "tiny-yolo-voc", "mini-mfma")]
    shapes = [(b, h, w, n) for n in (64, 48, 20) for (w, h) in ((32, 32), (48, 48), (32, 48)) for b in (2, 5)] + [(3, 32, 32, 44)]
    for batch, h, w, n in shapes:
        for pool in (0, 1):
            f = _desc(pd, batch, h, w, n, pool)
            wp = pd.winos_plan(pd.the_lib, f)
            assert wp.eligible == 1 and wp.take == 0 and wp.form == 32, (f, wp.take)
            for k in ("Y2_WINO", "Y2_C32F_MIN_TILES"):
                os.environ[k] = "1"
                try:
                    assert pd.winos_plan(pd.the_lib, f).take == 0, k
                finally:
                    del os.environ[k]
            os.environ["Y2_WINOS"] = "1"
            try:
                assert pd.winos_plan(pd.the_lib, f).take == 1
            finally:
                del os.environ["Y2_WINOS"]


def test_switch_off_and_ineligible_descriptors(pd):
    big = _desc(pd, 32, 304, 304, 64, 1)
    assert pd.winos_plan(pd.the_lib, big).take == 1
    os.environ["Y2_WINOS"] = "0"
    try:
        assert pd.winos_plan(pd.the_lib, big).take == 0
        # every zoo descriptor under Y2_WINOS=0: nothing is taken
        for net, size, batch in pd.wino_cases():
            for i, f in pd._descs(net, size, batch, 0, pd.ALIGNED):
                assert pd.winos_plan(pd.the_lib, f).take == 0, (net, size, batch, i)
    finally:
        del os.environ["Y2_WINOS"]
    os.environ["Y2_WINOS"] = "1"
    try:
        # fp16 storage on either side, strides, other sizes, other channel counts, too many filters, maps off the patch size
        for kw in (dict(x_f16=1, y_f16=1, alpha=0x50000, beta=0x60000), dict(y_f16=1), dict(stride=2, out_h=152, out_w=152), dict(size=1, pad=0),
                   dict(c=64, ldx=64), dict(n=96, ldy=96), dict(n=30, ldy=30), dict(h=300, out_h=300), dict(w=296, out_w=296),
                   dict(tile_bm=128, tile_bn=128)):
            wp = pd.winos_plan(pd.the_lib, dict(big, **kw))
            assert wp.eligible == 0 and wp.take == 0, kw
    finally:
        del os.environ["Y2_WINOS"]
    # fp16 mode in the table: never eligible.  (Strict mode has no descriptor form: the plan pass skips it, tests/test_gpu_winos.py)
    assert not [k for k, r in _rows().items() if r["f16_eligible"] or r["f16_take"]]


def test_existing_queries_do_not_see_the_rule(pd):
    """y2h_conv_variant / y2h_conv_workspace_bytes / y2h_wino_plan answer for a taken layer what they answer without the switch"""
    lib = pd.the_lib
    lib.y2h_conv_variant.restype = C.c_char_p
    lib.y2h_conv_variant.argtypes = [C.POINTER(pd.Conv), C.c_int]
    lib.y2h_conv_workspace_bytes.restype = C.c_size_t
    f = _desc(pd, 32, 304, 304, 64, 1)

    def answers():
        d, w = pd.Conv(**f), pd.wino_plan(lib, f)
        return (lib.y2h_conv_variant(C.byref(d), 0), lib.y2h_conv_variant(C.byref(d), 1), lib.y2h_conv_workspace_bytes(C.byref(d)),
                lib.y2h_conv_uses_mfma(C.byref(d)), w.eligible, w.take, w.bm, w.bn, w.tiles_pad)

    plain = answers()
    assert plain[0] == b"conv_c32_f32_16x16" and plain[2] == 0 and plain[5] == 0
    assert pd.winos_plan(lib, f).take == 1
    for v in ("0", "1"):
        os.environ["Y2_WINOS"] = v
        try:
            assert answers() == plain, v
        finally:
            del os.environ["Y2_WINOS"]
