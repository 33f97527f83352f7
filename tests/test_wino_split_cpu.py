"""The 3-way bf16 split of the fp32 Winograd GEMMs (include/y2_split_rule.h) without a GPU: the split itself and the U packer
through a stand-alone C program (tests/wino_split_check.c, run once more under -fsanitize=address,undefined -- no Python in
that process), and the rule through y2h_wino_split_plan against its committed table."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wino_split_plan_table.txt")
SRC = os.path.join(ROOT, "tests", "wino_split_check.c")
CFLAGS = ["-ffp-contract=off", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wino_split")
    plain, san = str(d / "check"), str(d / "check_san")
    subprocess.run(["gcc", "-O2"] + CFLAGS + [SRC, "-o", plain, "-lm"], check=True)
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + CFLAGS + [SRC, "-o", san, "-lm"], check=True)
    return plain, san, d


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


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_split_is_exact(programs, which):
    """>= 1 M random floats over every exponent, +-0, subnormals, +-inf, NaNs, FLT_MAX, integers up to 2^24, values of <= 16
    significant bits: h + m + l == a bit for bit wherever bf16's subnormal grid (2^-133) can carry a, l is a bf16 value and
    zero for <= 16 significant bits, non-finite values give (a, 0, 0), no part of a finite value is infinite"""
    out = subprocess.run([programs[which], "split"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 1000000


def _bf16_rn(a):
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)        # finite values far from overflow only


def _bf16_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("c,n", [(32, 36), (96, 36), (256, 36), (32, 296), (96, 296), (256, 296)])
def test_u_packer_equals_numpy_restatement(programs, c, n):
    """y2_split_pack_u == G g G^T in double rounded to fp32, split three ways, laid out as
    [g][row / 256][c / 16][plane][c % 16 / 8][row % 256][c % 8] with zero rows behind the last filter"""
    path = str(programs[2] / ("u_%d_%d.bin" % (c, n)))
    subprocess.run([programs[1], "pack", str(c), str(n), path], check=True)       # the sanitized build: the packer's indexing
    got = np.fromfile(path, dtype=np.uint16)
    i = np.arange(n * c * 9, dtype=np.uint64)
    w = ((((i * np.uint64(2654435761) + np.uint64(12345)) >> np.uint64(3)) & np.uint64(0xffffff)).astype(np.float64) / 16777216.0 - 0.5)
    g = w.astype(np.float32).astype(np.float64).reshape(n, c, 3, 3)
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    u = np.einsum("ik,nckl,jl->ncij", G, g, G).astype(np.float32).reshape(n, c, 16)       # exact in double: 24-bit dyadic weights
    n_pad = (n + 255) // 256 * 256
    full = np.zeros((16, n_pad, c), dtype=np.float32)
    full[:, :n, :] = u.transpose(2, 0, 1)
    h = _bf16_rn(full)
    r1 = full - _bf16_f32(h)
    m = _bf16_rn(r1)
    r2 = r1 - _bf16_f32(m)
    assert not (r2.view(np.uint32) & 0xffff).any()
    l = (r2.view(np.uint32) >> 16).astype(np.uint16)
    assert m.any() and l.any()
    planes = np.stack([h, m, l])                                                   # [p][g][row][c]
    want = planes.reshape(3, 16, n_pad // 256, 256, c // 16, 2, 8).transpose(1, 2, 4, 0, 5, 3, 6)   # [g][rb][kt][p][half][row][8]
    assert got.size == 16 * n_pad * c * 3
    assert np.array_equal(got, want.reshape(-1))


def test_rule_table_unchanged():
    """tools/plan_dump.py --wino-split against the committed table; a deliberate change of the rule regenerates it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("Y2_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_dump.py"), "--wino-split"], check=True, capture_output=True,
                         text=True, env=env).stdout
    assert out == open(TABLE).read(), "tools/plan_dump.py --wino-split differs from tests/golden/wino_split_plan_table.txt"


@pytest.mark.parametrize("flag,table", [("--wino", "wino_plan_table.txt"), ("--winos", "winos_plan_table.txt")])
def test_fp32_winograd_tables_are_the_parents(flag, table):
    """the two Winograd rules answer what they answered (the third table, --sweep, is tests/test_conv_plan_table.py's)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("Y2_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_dump.py"), flag], check=True, capture_output=True, text=True, env=env).stdout
    assert out == open(os.path.join(ROOT, "tests", "golden", table)).read()


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


def test_switches(pd):
    """Y2_WINO_SPLIT=0 never takes the form and =1 takes every eligible layer; Y2_WINO=1 alone, or a Y2_CONV_TILE that names
    an fp32 tile, does not select it; Y2_WINO_SPLIT_TILE names the split GEMM's own tile; Y2_WINO=0 rules every Winograd form out; fp16 storage and other shapes are not eligible"""
    lib = pd.the_lib
    small, big = _desc(pd, 2, 5, 7, 32, 296), _desc(pd, 32, 19, 19, 1024, 1024)
    plan = lambda f: pd.wino_split_plan(lib, f)
    assert plan(small).eligible == 1 and plan(small).take == 0
    for f in (small, big):
        assert _with_env({"Y2_WINO_SPLIT": "0"}, lambda: plan(f)).take == 0
        w = _with_env({"Y2_WINO_SPLIT": "1"}, lambda: plan(f))
        assert (w.take, w.bm, w.bn, w.bk) == (1, 256, 256, 16) and w.tiles_pad % 256 == 0
        assert w.v_bytes == 16 * w.tiles_pad * f["c"] * 6 and w.u_bytes == 16 * ((f["n"] + 255) // 256 * 256) * f["c"] * 6
        assert _with_env({"Y2_WINO": "1"}, lambda: plan(f)).take == 0
        assert _with_env({"Y2_WINO": "1", "Y2_WINO_SPLIT": "1"}, lambda: plan(f)).take == 1
        assert _with_env({"Y2_WINO": "0", "Y2_WINO_SPLIT": "1"}, lambda: plan(f)).take == 0
        assert _with_env({"Y2_CONV_TILE": "192x256"}, lambda: plan(f)).take == 0
        assert _with_env({"Y2_CONV_TILE": "128x128", "Y2_WINO_SPLIT": "1"}, lambda: plan(f)).take == 0
        assert _with_env({"Y2_WINO_SPLIT_TILE": "256x256", "Y2_WINO_SPLIT": "1"}, lambda: plan(f)).take == 1
        assert _with_env({"Y2_WINO_SPLIT_TILE": "128x256", "Y2_WINO_SPLIT": "1"}, lambda: plan(f)).eligible == 0
        # the fp32 form's own answer does not see any of it
        assert _with_env({"Y2_WINO_SPLIT": "1"}, lambda: pd.wino_plan(lib, f)).take == pd.wino_plan(lib, f).take
    for kw in (dict(x_f16=1, y_f16=1, alpha=0x50000, beta=0x60000), dict(y_f16=1), dict(stride=2, out_h=10, out_w=10), dict(size=1, pad=0),
               dict(c=48, ldx=48), dict(fuse_maxpool2=1)):
        w = _with_env({"Y2_WINO_SPLIT": "1"}, lambda: plan(dict(big, **kw)))
        assert w.eligible == 0 and w.take == 0, kw
    lib.y2h_wino_split_workspace_bytes.restype = C.c_size_t
    d = pd.Conv(**big)
    w = _with_env({"Y2_WINO_SPLIT": "1"}, lambda: plan(big))
    assert _with_env({"Y2_WINO_SPLIT": "1"}, lambda: lib.y2h_wino_split_workspace_bytes(C.byref(d))) == w.v_bytes + w.m_bytes
    assert _with_env({"Y2_WINO_SPLIT": "0"}, lambda: lib.y2h_wino_split_workspace_bytes(C.byref(d))) == 0
