"""The trainer's precision modes without a GPU: the numpy restatement of the rounding (tests/train_bf16_rule.py) equals the C
functions of include/y2_split_rule.h bit for bit on 10^5 patterns, h + m + l == a holds wherever the header says it does;
the mode is the engine's (set, read back, refused by name, kept across set_batch_network, Y2_TRAIN_PRECISION honoured and
refused in a child process); and a mode changes no refusal of the trainer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_bf16_rule as R
from tests import train_rule as T
from tests.test_native_callers import ROOT, build
from tests.test_train_host import refusal_net

N_PATTERNS = 100000
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x007fffff,
           0x00800000, 0x3f800000, 0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f80ffff, 0xbf808000, 0xbf818000,
           0x7f7f7fff, 0x7f7f8000, 0x7f7f8001, 0x7f7fffff, 0xff7f8000, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0x7fc00000,
           0xffc00001, 0x7fffffff, 0xff800001, 0x08800000, 0x08000000, 0x04000001]


def patterns():
    rng = np.random.RandomState(20)
    u = rng.randint(0, 2 ** 32, size=N_PATTERNS, dtype=np.uint64).astype(np.uint32)
    n = len(SPECIAL)
    u[:n] = SPECIAL
    k = (N_PATTERNS - n) // 5
    u[n:n + k] = (u[n:n + k] & 0xffff0000) | 0x8000                         # ties of the first rounding
    u[n + k:n + 2 * k] = (u[n + k:n + 2 * k] & 0x807fffff)                    # subnormals
    top = n + 2 * k                                                           # from the overflow threshold up: finite, then NaNs
    u[top:top + 2000] = 0x7f7f8000 + rng.randint(0, 2 ** 15, size=2000)
    u[top + 2000:top + 4000] = 0xff7f8000 + rng.randint(0, 2 ** 15, size=2000)
    u[top + 4000:top + 5000] = 0x7f800000 + rng.randint(0, 2 ** 23, size=1000)
    u[top + 5000:top + 6000] = 0xff800000 + rng.randint(0, 2 ** 23, size=1000)
    u[n + 3 * k:n + 4 * k] &= 0xffffff00                                      # at most 16 significant bits: l == 0
    return u


@pytest.fixture(scope="module")
def c_results(workdir):
    u = patterns()
    exe = build(workdir, "split_rule_probe", "gcc", "split_rule_probe.c", ["-ffp-contract=off"])
    src, dst = os.path.join(workdir, "patterns.bin"), os.path.join(workdir, "split.bin")
    u.tofile(src)
    subprocess.run([exe, src, dst], check=True, timeout=60)
    out = np.fromfile(dst, np.uint16).reshape(-1, 4)
    assert out.shape[0] == u.size == N_PATTERNS
    return u, out


def test_bf16_rn_is_the_header(c_results):
    u, c = c_results
    a = u.view(np.float32)
    got = R.bf16_rn(a)
    assert np.array_equal(got, c[:, 0])
    fin = (u & 0x7fffffff) < 0x7f800000
    assert np.all(np.isfinite(R.bf16_f32(got[fin])))                        # a finite value never becomes an infinity
    assert np.all(np.isnan(R.bf16_f32(got[(u & 0x7fffffff) > 0x7f800000])))
    # nearest: no other bf16 number is closer (checked where neighbours exist and nothing saturates)
    mid = fin & ((u & 0x7fffffff) < 0x7f7f0000)
    r = R.bf16_f32(got[mid]).astype(np.float64)
    down = (u[mid] & 0xffff0000).view(np.float32).astype(np.float64)
    up = ((u[mid] & 0xffff0000) + 0x10000).astype(np.uint32).view(np.float32).astype(np.float64)
    x = a[mid].astype(np.float64)
    assert np.all(np.abs(r - x) <= np.minimum(np.abs(down - x), np.abs(up - x)))


def test_split3_is_the_header(c_results):
    u, c = c_results
    a = u.view(np.float32)
    h, m, l = R.split3(a)
    assert np.array_equal(h, c[:, 1]) and np.array_equal(m, c[:, 2]) and np.array_equal(l, c[:, 3])
    mag = u & 0x7fffffff
    non = mag >= 0x7f800000
    assert non.sum() > 1000 and not m[non].any() and not l[non].any() and np.array_equal(h[non], c[non, 0])
    # the sum is exact for every finite multiple of 2^-133 (all normal values from 2^-110 up among them), the threshold
    # case |a| >= 0x7f7f8000 included; a tinier bit is rounded away and the sum is then within 2^-134
    fin = ~non
    s = R.bf16_f32(h).astype(np.float64) + R.bf16_f32(m).astype(np.float64) + R.bf16_f32(l).astype(np.float64)
    with np.errstate(invalid="ignore"):
        a64 = a.astype(np.float64)
        exact = fin & (np.mod(np.where(fin, a64, 0) * 2.0 ** 133, 1.0) == 0)
    assert exact.sum() > 60000 and (fin & (mag >= 0x7f7f8000)).sum() > 1000
    assert np.array_equal(s[exact], a64[exact])
    assert np.all(np.abs(s[fin] - a64[fin]) <= 2.0 ** -134)
    assert (fin & ~exact).sum() > 1000
    # at most 16 significant bits: two planes hold it all
    short = fin & ((u & 0xff) == 0) & (mag >= 0x08800000)
    assert short.sum() > 10000 and not (l[short] & 0x7fff).any()
    # every part has at most 8 significant bits by construction (bf16); below the threshold case the remainders shrink
    big = fin & (mag >= 0x08800000) & (mag < 0x7f7f8000)
    assert np.all(np.abs(R.bf16_f32(m[big]).astype(np.float64)) <= np.abs(a64[big]) * 2.0 ** -8)
    assert np.all(np.abs(R.bf16_f32(l[big]).astype(np.float64)) <= np.abs(a64[big]) * 2.0 ** -16)


# ---- the mode ----
def small_net(tmp_path, name="A"):
    cfg = str(tmp_path / ("precision_%s.cfg" % name))
    with open(cfg, "w") as f:
        f.write(T.net_text(T.NETS[name]))
    return darknet.Network.parse_network_cfg(cfg), cfg


def test_mode_is_set_read_back_and_refused_by_name(tmp_path):
    net, _ = small_net(tmp_path)
    L = darknet.lib()
    assert net.train_precision() == "fp32"                                   # the default
    for k, name in enumerate(("fp32", "bf16x3", "bf16")):
        net.train_set_precision(name)
        assert net.train_precision() == name
        assert L.y2_train_precision(net.net) == k
    for bad in (3, -1, 7):
        assert L.y2_train_set_precision(net.net, bad) == -1
        msg = darknet._check()
        assert "fp32" in msg and "bf16x3" in msg and "bf16" in msg and str(bad) in msg
        assert net.train_precision() == "bf16"                               # a refused value changes nothing
    with pytest.raises(darknet.Y2Error, match="fp32, bf16x3, bf16"):
        net.train_set_precision("fp16")
    # the mode is the engine's: a batch change keeps it
    net.set_batch_network(2)
    assert net.train_precision() == "bf16"
    net.train_set_precision("bf16x3")
    net.set_batch_network(T.NETS["A"]["batch"])
    assert net.train_precision() == "bf16x3"
    net.free()


CHILD = """
import sys
sys.path.insert(0, %r)
from sr_object_detection_amd import darknet
try:
    net = darknet.Network.parse_network_cfg(sys.argv[1])
except darknet.Y2Error as e:
    print("REFUSED " + str(e))
else:
    print("MODE " + net.train_precision())
"""


@pytest.mark.parametrize("word,want", [(None, "MODE fp32"), ("fp32", "MODE fp32"), ("bf16x3", "MODE bf16x3"), ("bf16", "MODE bf16"),
                                       ("fp16", "REFUSED"), ("BF16", "REFUSED")])
def test_environment_sets_the_default(tmp_path, word, want):
    net, cfg = small_net(tmp_path)
    net.free()
    env = dict(os.environ)
    env.pop("Y2_TRAIN_PRECISION", None)
    if word is not None:
        env["Y2_TRAIN_PRECISION"] = word
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, cfg], env=env, capture_output=True, text=True, timeout=120, check=True).stdout
    line = [l for l in out.splitlines() if l.startswith(("MODE", "REFUSED"))][-1]
    assert line.startswith(want), out
    if want == "REFUSED":
        assert "Y2_TRAIN_PRECISION=" + word in line and "fp32, bf16x3, bf16" in line


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("what", ["stride", "recurrent", "fp16"])
def test_a_mode_changes_no_refusal(tmp_path, what, mode):
    net, pattern = refusal_net(tmp_path, "stride" if what == "fp16" else what)
    if what == "fp16":
        net.set_half(True)
        pattern = r"fp16 mode"
    net.train_set_precision(mode)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    assert net.train_precision() == mode
    net.free()


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"y2_train_set_precision", "y2_train_precision", "y2h_train_conv_forward_bf16", "y2h_train_conv_dinput_bf16",
            "y2h_train_conv_dweight_bf16"}
    assert want <= have, sorted(want - have)


def test_rule_trainer_rounds_only_the_products():
    """Bf16Trainer on net A: its first convolution's output is the float64 product of the ROUNDED input and weights, and
    with operands that bf16 holds exactly it is the plain Trainer"""
    spec, seed = T.NETS["A"], 5
    params = T.params_for("A", seed)
    x, y = T.inputs(spec, seed, 1)
    plain, rounded = T.Trainer(spec, params), R.Bf16Trainer(spec, params)
    plain.step(x, y)
    rounded.step(x, y)
    assert not np.array_equal(plain.L[0]["x"], rounded.L[0]["x"])
    assert T.err(rounded.L[0]["x"], plain.L[0]["x"]) < 2.0 ** -6            # two operands of 2^-9 relative error each
    xr, wr = R.bf16_round(x.astype(np.float64)), R.bf16_round(params[0]["weights"].astype(np.float64))
    xp = np.zeros((x.shape[0], x.shape[1], x.shape[2] + 2, x.shape[3] + 2))
    xp[:, :, 1:-1, 1:-1] = xr
    want = sum(np.einsum("bchw,nc->bnhw", xp[:, :, ky:ky + x.shape[2], kx:kx + x.shape[3]], wr[:, :, ky, kx]) for ky in range(3) for kx in range(3))
    assert np.allclose(rounded.L[0]["x"], want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(rounded.L[0]["weights"].astype(np.float32), (params[0]["weights"] + (rounded.L[0]["weights"] - params[0]["weights"])).astype(np.float32))
    exact = [None if p is None else {k: (R.bf16_round(v) if k == "weights" else v) for k, v in p.items()} for p in params]
    a, b = T.Trainer(spec, exact), R.Bf16Trainer(spec, exact)
    xq = R.bf16_round(x)
    a._conv_forward(spec["layers"][0], a.L[0], np.array(xq, np.float64))
    b._conv_forward(spec["layers"][0], b.L[0], np.array(xq, np.float64))
    assert np.array_equal(a.L[0]["x"], b.L[0]["x"])
