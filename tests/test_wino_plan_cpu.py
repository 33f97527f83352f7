"""The Winograd rule (include/y2_wino_rule.h, asked through y2h_wino_plan) is host arithmetic: which 3x3 layers it takes can be
checked without a GPU.  The committed table pins its answer for every 3x3 layer of every zoo network at batch 1 / 8 / 32 /
128; the other tests state what the table must keep saying."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wino_plan_table.txt")


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
            shape=[int(v) for v in shape], eligible=int(f32[0]), take=int(f32[1]), tile=f32[2], f16_eligible=int(f16[0]), f16_take=int(f16[1]))
    return rows


def _desc(pd, batch, h, w, c, n, pool=0, **kw):
    return dict(dict(batch=batch, h=h, w=w, c=c, ldx=c, n=n, size=3, stride=1, pad=1, out_h=h, out_w=w, ldy=n, fuse_maxpool2=pool,
                     batch_normalize=1, activation=1, x=0x10000, w_packed=0x20000, y=pd.ALIGNED, bias=0x40000), **kw)


def test_rule_table_unchanged():
    """tools/plan_dump.py --wino against the committed table; a deliberate change of the rule regenerates it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("Y2_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_dump.py"), "--wino"], check=True, capture_output=True,
                         text=True, env=env).stdout
    assert out == open(TABLE).read(), "tools/plan_dump.py --wino differs from tests/golden/wino_plan_table.txt"


def test_headline_layers():
    """yolo.cfg 608x608 batch 32: the 76x76 layers 8 and 10 stay on the direct 192x256 tile (as does everything above them);
    the nine 3x3 layers from 38x38 down are taken"""
    rows = _rows()
    taken = sorted(i for (net, size, b, i), r in rows.items() if (net, size, b) == ("yolo", 608, 32) and r["take"])
    assert taken == [12, 14, 16, 18, 20, 22, 23, 24, 29], taken
    assert rows[("yolo", 608, 32, 8)]["eligible"] and rows[("yolo", 608, 32, 10)]["eligible"]


def test_small_grids_are_left_alone(pd):
    """no layer of a detector at batch 1 is taken (their deep layers are split along K there: the cost model's error exceeds the
    margin; the GPU tests pin those kernel names), and neither are the shapes the tile tests force with Y2_WINO=1 -- which that
    switch, and only that switch, turns on"""
    rows = _rows()
    assert not [k for k, r in rows.items() if k[2] == 1 and r["take"] and k[0] in ("yolo", "yolo9000", "tiny-yolo-voc", "mini-mfma")]
    # what IS taken at batch 1: the one 56x56 256->512 layer of the 448x448 YOLOv1 nets, whose grid fills the machine unsplit
    assert sorted(k[:2] + k[3:] for k, r in rows.items() if k[2] == 1 and r["take"]) == [("yolo-v1", 448, 7), ("yolo-v1-small", 448, 8)]
    shapes = [(2, 5, 7, 32, 296), (3, 6, 8, 96, 36), (2, 26, 26, 96, 168), (3, 26, 26, 32, 36), (3, 19, 19, 96, 296), (2, 9, 13, 96, 136),
              (2, 14, 14, 256, 64), (2, 19, 19, 64, 96), (2, 26, 26, 64, 296), (3, 20, 20, 96, 280)]
    for batch, h, w, c, n in shapes:
        for pool in (0, 1):
            if pool and (h | w) & 1:
                continue
            f = _desc(pd, batch, h, w, c, n, pool)
            wp = pd.wino_plan(pd.the_lib, f)
            assert wp.eligible == 1 and wp.take == 0, (f, wp.take)
            os.environ["Y2_WINO"] = "1"
            try:
                assert pd.wino_plan(pd.the_lib, f).take == 1
            finally:
                del os.environ["Y2_WINO"]


def test_switch_off_and_ineligible_descriptors(pd):
    big = _desc(pd, 32, 19, 19, 1024, 1024)
    assert pd.wino_plan(pd.the_lib, big).take == 1
    os.environ["Y2_WINO"] = "0"
    try:
        assert pd.wino_plan(pd.the_lib, big).take == 0
    finally:
        del os.environ["Y2_WINO"]
    os.environ["Y2_WINO"] = "1"
    try:
        # fp16 storage on either side, strides, other sizes, channels off a multiple of 32, odd maps under the fused pool
        for kw in (dict(x_f16=1, y_f16=1, alpha=0x50000, beta=0x60000), dict(y_f16=1), dict(stride=2, out_h=10, out_w=10), dict(size=1, pad=0),
                   dict(c=48, ldx=48), dict(fuse_maxpool2=1)):
            wp = pd.wino_plan(pd.the_lib, dict(big, **kw))
            assert wp.eligible == 0 and wp.take == 0, kw
    finally:
        del os.environ["Y2_WINO"]
    # fp16 mode in the table: never eligible.  (Strict mode has no descriptor form: the plan pass skips it, tests/test_gpu_wino.py)
    assert not [k for k, r in _rows().items() if r["f16_eligible"] or r["f16_take"]]


def test_existing_queries_do_not_see_the_rule(pd):
    """y2h_conv_variant / y2h_conv_workspace_bytes answer for a taken layer what they answered before"""
    big = pd.Conv(**_desc(pd, 32, 19, 19, 1024, 1024))
    lib = pd.the_lib
    lib.y2h_conv_variant.restype = C.c_char_p
    lib.y2h_conv_variant.argtypes = [C.POINTER(pd.Conv), C.c_int]
    lib.y2h_conv_workspace_bytes.restype = C.c_size_t
    lib.y2h_wino_workspace_bytes.restype = C.c_size_t
    assert lib.y2h_conv_variant(C.byref(big), 0) == b"conv_mfma_f32_192x256x32_k3"
    assert lib.y2h_conv_workspace_bytes(C.byref(big)) == 0
    wp = pd.wino_plan(lib, _desc(pd, 32, 19, 19, 1024, 1024))
    assert lib.y2h_wino_workspace_bytes(C.byref(big)) == wp.v_bytes + wp.m_bytes == 16 * wp.tiles_pad * (1024 + 1024) * 4
