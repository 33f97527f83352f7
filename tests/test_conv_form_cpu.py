"""Which form a convolution runs in -- direct, Winograd, split Winograd or stationary Winograd -- is decided once, by
y2_conv_form_of (y2_plan.c), and is host arithmetic: it can be pinned without a GPU.  The three committed rule tables each pin
one rule alone; this file pins which rule wins."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIRECT, WINO, WINOX, WINOS = range(4)          # csrc/host/y2_internal.h: Y2_FORM_*
PREFIX = {WINO: "conv_wino_f32_", WINOX: "conv_winox_f32_", WINOS: "conv_winos_f32_c"}


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


def _table(name):
    """a rule table's rows by (net, size, batch, layer): pool, the fp32 columns, the fp16 take"""
    rows = {}
    for line in open(os.path.join(GOLDEN, name)):
        if line.startswith("#"):
            continue
        key, shape, f32, f16 = [p.split() for p in line.split("|")]
        rows[(key[0], int(key[1]), int(key[2][1:]), int(key[3][1:]))] = dict(pool=int(shape[4]), f32=f32, take=(int(f32[1]), int(f16[1])))
    return rows


def _expected(split, wino, winos):
    return WINOX if split else WINO if wino else WINOS if winos else DIRECT


def test_every_row_of_the_three_rule_tables(pd):
    """For every (net, size, batch, layer) of wino_plan_table.txt, wino_split_plan_table.txt and winos_plan_table.txt, fp32 and
    fp16, the form is the one the tables' own take columns give: split, else wino, else winos, else direct.  A wino row's name
    carries the wino table's tile, and every name's +maxpool2 suffix follows the row's pool column.

    The test prints how many rows have more than one take set: 175 in the committed tables (layers both the split rule and
    the fp32 Winograd rule take), so the tables themselves exercise split-beats-wino; the rest of the precedence is
    exercised by test_forced_switches."""
    wino, split, winos = _table("wino_plan_table.txt"), _table("wino_split_plan_table.txt"), _table("winos_plan_table.txt")
    assert set(wino) == set(split) == set(winos) and wino
    seen, multi, by_form = set(), {}, [0, 0, 0, 0]
    for net, size, batch in pd.wino_cases():
        for half in (0, 1):
            for i, f in pd._descs(net, size, batch, half, pd.ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                key = (net, size, batch, i)
                seen.add(key)
                takes = [t[key]["take"][half] for t in (split, wino, winos)]
                if sum(takes) > 1:
                    multi[tuple(takes)] = multi.get(tuple(takes), 0) + 1
                want = _expected(*takes)
                form, name = pd.conv_form(pd.the_lib, f)
                assert form == want, (key, half, takes, form, name)
                by_form[form] += 1
                assert wino[key]["pool"] == split[key]["pool"] == winos[key]["pool"] == f["fuse_maxpool2"], key
                if form == DIRECT:
                    assert name == "", (key, name)            # the direct form's name is plan_conv_kernels' business
                    continue
                assert name.startswith(PREFIX[form]) and name.endswith("+maxpool2") == bool(f["fuse_maxpool2"]), (key, name)
                if form == WINO:
                    assert name.split("+")[0] == "conv_wino_f32_%sx32" % wino[key]["f32"][2], (key, name)
    assert seen == set(wino)
    print("%d keys; fp32 + fp16 rows by form (direct, wino, winox, winos): %s; rows with more than one take set, by (split, wino, winos): %s"
          % (len(wino), by_form, multi))
    assert sum(multi.values()) > 0


# the one descriptor all three rules find eligible: batch 2, 32x32, 32 -> 64 channels, 3x3/1 pad 1, ldx 32, ldy 64
SWITCHES = [
    (dict(Y2_WINO="1", Y2_WINO_SPLIT="1", Y2_WINOS="1"), WINOX),
    (dict(Y2_WINO="1", Y2_WINOS="1"), WINO),
    (dict(Y2_WINOS="1"), WINOS),
    (dict(), DIRECT),
    (dict(Y2_WINO="0", Y2_WINO_SPLIT="1", Y2_WINOS="1"), WINOS),           # the split plan returns before take under Y2_WINO=0
    (dict(Y2_CONV_TILE="128x128", Y2_WINO="1", Y2_WINO_SPLIT="1", Y2_WINOS="1"), WINO),   # a named fp32 tile keeps the fp32 forms,
]                                                                                        # and the stationary rule refuses under it


@pytest.mark.parametrize("pool", [0, 1], ids=["nopool", "pool"])
@pytest.mark.parametrize("env,want", SWITCHES, ids=lambda v: "+".join("%s=%s" % kv for kv in v.items()) or "none" if isinstance(v, dict) else None)
def test_forced_switches(pd, monkeypatch, env, want, pool):
    f = dict(batch=2, h=32, w=32, c=32, ldx=32, n=64, size=3, stride=1, pad=1, out_h=32, out_w=32, ldy=64, fuse_maxpool2=pool,
             batch_normalize=1, activation=1, x=0x10000, w_packed=0x20000, y=pd.ALIGNED, bias=0x40000)
    lib = pd.the_lib
    assert pd.wino_split_plan(lib, f).eligible == 1 and pd.wino_plan(lib, f).eligible == 1 and pd.winos_plan(lib, f).eligible == 1
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    form, name = pd.conv_form(lib, f)
    assert form == want, (env, form, name)
    if want == DIRECT:
        assert name == ""
    else:
        assert name.startswith(PREFIX[want]) and name.endswith("+maxpool2") == bool(pool), name
    if want == WINOS:
        assert name.split("+")[0] == "conv_winos_f32_c32", name
