"""y2h_rec_step and y2h_rnn_sample driven directly (sr_object_detection_amd/csrc/y2_recurrent.hip) against the numpy rules
of tests/rec_rule.py and tests/chargen_rule.py: every row count of every rec_skinny_kernel<MB, VEC> instantiation, the
16-byte and the scalar path, the alignment fallback, exactly 64 KB of staged rows, every mode, batch-norm and the
activations the recurrent cfgs use, on data whose dot products are exact in any order -- so the kernel must EQUAL the
rule -- with a guard row around every output buffer; a real-valued product against float64 under the summation bound; the
refusals; the sampling kernel's edges."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import rec_rule
from tests.chargen_rule import sample_rule
from tests.test_gpu_kernels import Dev

F = np.float32
SENTINEL = F(-7654321.)
ACTS = ["linear", "leaky", "relu", "logistic", "tanh", "loggy"]
# k, x placed 4 bytes past a 16-byte boundary
KS = [(4, False), (30, False), (36, False), (130, False), (200, False), (1024, False), (1024, True)]
# mode, shortcut, out2 set, xcopy set
VARIANTS = [("DENSE", 0, False, False), ("DENSE", 0, False, True), ("RNN", 0, True, False), ("RNN", 1, False, False),
            ("GRU_ZR", 0, True, False), ("GRU_H", 0, True, False)]
MODE = {"DENSE": rec_rule.DENSE, "RNN": rec_rule.RNN, "GRU_ZR": rec_rule.GRU_ZR, "GRU_H": rec_rule.GRU_H}


def mb_of(rows):
    """the MB of the rec_skinny_kernel instantiation y2h_rec_step picks"""
    return 1 if rows <= 1 else (2 if rows <= 2 else (4 if rows <= 4 else 8))


def is_vec(k, misaligned):
    return k % 4 == 0 and not misaligned


def build_matrix():
    """The cases of test_skinny_equals_the_rule: every row count 1..8 with every k (two cases each at 1 and 2 rows, which
    are alone in their instantiation), 2048 at 8 rows; mode, n, batch-norm and activation are dealt so that the value seen
    least often with this instantiation (mode: with this instantiation and path) comes next.  What that covers is asserted
    by test_matrix_covers_every_instantiation below."""
    seen = {}

    def pick(key, values):
        v = min(values, key=lambda c: (seen.get((key, c), 0), values.index(c)))
        seen[(key, v)] = seen.get((key, v), 0) + 1
        return v

    cases = []
    slots = [(rows, k, mis) for rows in range(1, 9) for k, mis in KS for _ in range(2 if rows <= 2 else 1)]
    slots += [(8, 2048, False)] * 4
    for rows, k, mis in slots:
        mb, vec = mb_of(rows), is_vec(k, mis)
        mode = pick((mb, vec, "mode"), ["DENSE", "RNN", "GRU_ZR", "GRU_H"])
        var = pick((mb, "variant", mode), [v for v in VARIANTS if v[0] == mode])
        h = pick((mb, "h2"), [19, 35]) if mode == "GRU_ZR" else pick((mb, "h"), [1, 37, 70])
        act = pick((mb, "act"), ACTS)
        bn = pick((mb, "bn", act), [0, 1])                      # per activation: an even count must not tie the two
        cases.append(dict(rows=rows, k=k, mis=mis, mode=mode, shortcut=var[1], out2=var[2], xcopy=var[3], h=h,
                          n=2 * h if mode == "GRU_ZR" else h, bn=bn, act=act))
    return cases


MATRIX = build_matrix()


def case_id(c):
    return "r%d-k%d%s-%s%s%s%s-n%d-bn%d-%s" % (c["rows"], c["k"], "mis" if c["mis"] else "", c["mode"], "s" if c["shortcut"] else "",
                                                  "" if c["out2"] or c["mode"] == "DENSE" else "-noout2", "-xcopy" if c["xcopy"] else "",
                                                  c["n"], c["bn"], c["act"])


def through_exp(c):
    return c["act"] in rec_rule.TRANSCENDENTAL or c["mode"] in ("GRU_ZR", "GRU_H")


def host_case(c, seed):
    """Host arrays of one launch.  x, proj, state, bias, mean and the batch-norm scales (negative ones among them) are
    small integers, w small integers -- times one power of two, 2^-s, where the value goes through an exp, so that the
    logistic does not sit at 0 or 1 for every sum; the partial sums of a dot product are then integers (times 2^-s) below
    2^24 in any order of summation, and every later operation is one fp32 (or double) operation per value that the rule
    states.  rinv is a power of two for the even columns and not for the odd ones; z lies in [0, 1]."""
    rng = np.random.default_rng(seed)
    rows, k, n, h = c["rows"], c["k"], c["n"], c["h"]
    ints = lambda lo, hi, *shape: rng.integers(lo, hi + 1, size=shape).astype(F)
    a = dict(c)
    a["x"] = ints(-3, 3, rows, k)
    s = int(np.ceil(np.log2(np.sqrt(k)))) + 1 if through_exp(c) else 0
    a["w"] = ints(-4, 4, n, k) * F(2.) ** -s
    a["bias"] = ints(-2, 2, n)
    a["scale"] = None
    if c["bn"]:
        a["mean"] = ints(-3, 3, n)
        a["scale"] = np.where(np.arange(n) % 3 == 1, F(-1), F(1)) * ints(1, 3, n)
        a["rinv"] = np.where(np.arange(n) % 2 == 0, 2. ** -rng.integers(0, 4, size=n), 1. / (1. + rng.integers(1, 9, size=n) / 7.)).astype(np.float64)
    pw = 3 * h if c["mode"] in ("GRU_ZR", "GRU_H") else h
    a["proj"] = ints(-2, 2, rows, pw)
    a["state"] = ints(-3, 3, rows, h)
    a["z"] = (ints(0, 16, rows, h) / F(16)).astype(F)
    return a


def rule_outputs(a):
    """(out, out2 or None, xcopy or None) by the rule"""
    mode = a["mode"]
    xc = a["x"] if a.get("xcopy") else None
    if mode == "DENSE":
        return rec_rule.step_dense(a), None, xc
    if mode == "RNN":
        s = rec_rule.step_rnn(a)
        return s, (s if a["out2"] else None), xc
    if mode == "GRU_ZR":
        z, f = rec_rule.step_gru_zr(a)
        return z, f, xc
    y = rec_rule.step_gru_h(a)
    return y, y, xc


class Launch:
    """device buffers of one case; every output buffer has a guard row in front and behind, filled with SENTINEL"""

    def __init__(self, dev, a):
        self.dev, self.a = dev, a
        rows, k, n, h = a["rows"], a["k"], a["n"], a["h"]
        self.ow = h if a["mode"] != "DENSE" else n              # the width of out and out2
        pad = np.zeros(4 + (1 if a["mis"] else 0), F)           # x: 16 bytes in front, then 4 more for the misaligned case
        self.x = dev.put(np.concatenate([pad, a["x"].reshape(-1)]))
        self.xoff = pad.nbytes
        self.ro = {key: dev.put(a[key]) for key in ("w", "bias", "proj", "z") if a.get(key) is not None}
        if a["scale"] is not None:
            self.ro.update({key: dev.put(a[key]) for key in ("mean", "scale", "rinv")})
        if a.get("pre") is not None:
            self.ro["pre"] = dev.put(a["pre"])
        self.state = dev.empty((rows + 2) * h * 4)
        self.out = dev.empty((rows + 2) * self.ow * 4)
        self.out2 = dev.empty((rows + 2) * self.ow * 4)
        self.xcopy = dev.empty((rows + 2) * k * 4)

    def _fill(self, p, width, inner=None):
        full = np.full((self.a["rows"] + 2, width), SENTINEL, F)
        if inner is not None:
            full[1:-1] = inner
        assert self.dev.L.y2h_memcpy_h2d(p, full.ctypes.data_as(C.c_void_p), full.nbytes, None) == 0

    def run(self, form):
        """one y2h_rec_step on freshly filled buffers: (status, out, out2, xcopy, state), each with its guard rows"""
        a, L = self.a, self.dev.L
        rows, k, h = a["rows"], a["k"], a["h"]
        in_place = a["mode"] == "GRU_H"                         # as y2_rec_forward calls it: out is the state buffer
        self._fill(self.state, h, a["state"])
        self._fill(self.out, self.ow)
        self._fill(self.out2, self.ow)
        self._fill(self.xcopy, k)
        at = lambda p, width: C.c_void_p(p.value + width * 4)   # past the guard row
        r = darknet.RecArgs()
        if a.get("pre") is None or a.get("x_with_pre"):
            r.x, r.w, r.bias = self.x.value + self.xoff, self.ro["w"].value, self.ro["bias"].value
            if a["scale"] is not None:
                r.mean, r.scale, r.rinv = self.ro["mean"].value, self.ro["scale"].value, self.ro["rinv"].value
        if a.get("pre") is not None:
            r.pre = self.ro["pre"].value
        r.bn, r.act = int(a["scale"] is not None), rec_rule.ACT[a["act"]]
        r.rows, r.k, r.n, r.h = rows, k, a["n"], (h if a["mode"] != "DENSE" else 0)
        r.mode, r.shortcut = MODE[a["mode"]], a["shortcut"]
        if a["mode"] != "DENSE":
            r.proj, r.state = self.ro["proj"].value, at(self.state, h).value
        if a["mode"] == "GRU_H":
            r.z = self.ro["z"].value
        r.out = at(self.state, h).value if in_place else at(self.out, self.ow).value
        if a["out2"] or a["mode"] == "DENSE":                   # DENSE gets the pointer too and must leave it alone
            r.out2 = at(self.out2, self.ow).value
        if a["xcopy"]:
            r.xcopy = at(self.xcopy, k).value
        for key, v in a.get("override", {}).items():
            setattr(r, key, v)
        status = L.y2h_rec_step(C.byref(r), form, None)
        get = lambda p, width: self.dev.get(p, (rows + 2, width))
        return status, get(self.out, self.ow), get(self.out2, self.ow), get(self.xcopy, k), get(self.state, h)

    def expected(self):
        """the four buffers as the rule leaves them: SENTINEL wherever the mode does not write"""
        a = self.a
        out, out2, xc = rule_outputs(a)
        full = lambda width, inner: np.concatenate([np.full((1, width), SENTINEL, F), inner, np.full((1, width), SENTINEL, F)])
        blank = lambda width: np.full((a["rows"], width), SENTINEL, F)
        in_place = a["mode"] == "GRU_H"
        return (full(self.ow, blank(self.ow) if in_place else out), full(self.ow, blank(self.ow) if out2 is None else out2),
                full(a["k"], blank(a["k"]) if xc is None else xc), full(a["h"], out if in_place else a["state"]))


NAMES = ("out", "out2", "xcopy", "state")


def compare(got, want, exact, what):
    """bitwise, or -- through an exp -- within one fp32 ulp on at most 1e-3 of the values: the device's double exp and
    libm's are each within an ulp of the true value, which the rounding to float keeps except next to a tie"""
    for name, g, w in zip(NAMES, got, want):
        if np.array_equal(g, w):
            continue
        assert not exact, "%s %s: %d of %d values differ from the rule, max %.3g" % (
            what, name, int((g != w).sum()), w.size, float(np.abs(g - w).max()))
        wrote = w != SENTINEL
        assert np.array_equal(g[~wrote], w[~wrote]), "%s %s: written outside what the mode writes" % (what, name)
        d = rec_rule.ulps(g[wrote], w[wrote])
        print("%s %s: %d of %d values one ulp from the rule" % (what, name, int((d > 0).sum()), d.size))
        assert d.max() <= 1, "%s %s: %d ulp from the rule" % (what, name, int(d.max()))
        assert (d > 0).sum() <= 1e-3 * d.size, "%s %s: %d of %d values differ from the rule" % (what, name, int((d > 0).sum()), d.size)


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    d.L.y2h_set_device(0)
    yield d
    d.close()


def test_matrix_covers_every_instantiation():
    """every value of every axis with every MB; every mode with every MB on the 16-byte and on the scalar path; every
    row count with every k; rows * k * 4 within 64 KB and once exactly there"""
    assert len(MATRIX) <= 100                                   # two launches each
    for mb in (1, 2, 4, 8):
        mine = [c for c in MATRIX if mb_of(c["rows"]) == mb]
        assert {(c["k"], c["mis"]) for c in mine} >= set(KS)
        assert {c["h"] for c in mine if c["mode"] != "GRU_ZR"} == {1, 37, 70}
        assert {c["h"] for c in mine if c["mode"] == "GRU_ZR"} == {19, 35}
        assert {c["bn"] for c in mine} == {0, 1} and {c["act"] for c in mine} == set(ACTS)
        assert {(c["mode"], c["shortcut"], c["out2"], c["xcopy"]) for c in mine} == set(VARIANTS)
        for vec in (True, False):
            assert {c["mode"] for c in mine if is_vec(c["k"], c["mis"]) == vec} == set(MODE), (mb, vec)
    assert {(c["rows"], c["k"], c["mis"]) for c in MATRIX} >= {(r, k, m) for r in range(1, 9) for k, m in KS}
    assert all(c["rows"] * c["k"] * 4 <= 65536 for c in MATRIX)
    assert {c["mode"] for c in MATRIX if c["rows"] * c["k"] * 4 == 65536} == set(MODE)
    exact = [c for c in MATRIX if not through_exp(c)]
    assert {mb_of(c["rows"]) for c in exact} == {1, 2, 4, 8} and {c["mode"] for c in exact} == {"DENSE", "RNN"}


@pytest.mark.gpu
@pytest.mark.parametrize("c", MATRIX, ids=case_id)
def test_skinny_equals_the_rule(dev, c):
    a = host_case(c, 1000 + MATRIX.index(c))
    run = Launch(dev, a)
    assert dev.L.y2h_rec_skinny_ok(c["rows"], c["k"]) == 1
    status, *skinny = run.run(darknet.REC_SKINNY)
    assert status == 0
    status, *ref = run.run(darknet.REC_REF)
    assert status == 0
    compare(skinny, run.expected(), not through_exp(c), "skinny")
    for name, s, r in zip(NAMES, skinny, ref):                  # the same device function on the same fp32 argument
        assert np.array_equal(s, r), "%s: the skinny launch differs from the reference-order launch" % name


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("var", VARIANTS[2:], ids=lambda v: v[0] + ("s" if v[1] else ""))
def test_ref_combines_a_product_made_elsewhere(dev, var, rows):
    """Y2H_REC_REF with `pre` (the matrix-core step form): no product, no epilogue -- the combine of `pre` alone.  The x / w /
    batch-norm pointers are set in one case and absent in the others: they must not be read either way."""
    h = 37 if var[0] != "GRU_ZR" else 19
    c = dict(rows=rows, k=36, mis=False, mode=var[0], shortcut=var[1], out2=var[2], xcopy=False, h=h,
             n=2 * h if var[0] == "GRU_ZR" else h, bn=1, act="leaky")
    a = host_case(c, 77 + rows)
    a["pre"] = (np.random.default_rng(5 + rows).integers(-24, 25, size=(rows, c["n"])) / F(8)).astype(F)
    a["x_with_pre"] = rows == 5
    run = Launch(dev, a)
    status, *got = run.run(darknet.REC_REF)
    assert status == 0
    compare(got, run.expected(), var[0] == "RNN", "ref with pre")


@pytest.mark.gpu
@pytest.mark.parametrize("rows,k", [(1, 1024), (8, 1024), (1, 2048), (8, 2048)])
def test_real_valued_product_within_the_summation_bound(dev, rows, k):
    """DENSE, no batch-norm, linear, on x in [0,1) and w = U(-a,a), a = sqrt(3/k), as synth makes them, against float64.
    Any order of k products and k + 1 sums (the bias included) of fp32 operations obeys |got - exact| <= g * (sum|x_i*w_i|
    + |bias|) with g = (k+2)*u / (1 - (k+2)*u), u = 2^-24 (Higham, Accuracy and Stability, 3.1 / 3.5)."""
    n = 70
    rng = np.random.default_rng(k + rows)
    c = dict(rows=rows, k=k, mis=False, mode="DENSE", shortcut=0, out2=False, xcopy=False, h=n, n=n, bn=0, act="linear")
    a = host_case(c, 1)
    a["x"] = rng.random((rows, k), dtype=F)
    lim = np.sqrt(3. / k)
    a["w"] = rng.uniform(-lim, lim, size=(n, k)).astype(F)
    a["bias"] = rng.uniform(-.1, .1, size=n).astype(F)
    run = Launch(dev, a)
    x64, w64, b64 = (a[key].astype(np.float64) for key in ("x", "w", "bias"))
    exact = x64 @ w64.T + b64
    mass = np.abs(x64) @ np.abs(w64).T + np.abs(b64)
    u = 2. ** -24
    g = (k + 2) * u / (1 - (k + 2) * u)
    for form in (darknet.REC_SKINNY, darknet.REC_REF):
        status, out, out2, xcopy, state = run.run(form)
        assert status == 0
        err = np.abs(out[1:-1].astype(np.float64) - exact)
        print("form %d rows %d k %d: max err / bound %.3g" % (form, rows, k, float((err / (g * mass)).max())))
        assert (err <= g * mass).all(), "form %d: %d values beyond the bound" % (form, int((err > g * mass).sum()))
        assert (out[[0, -1]] == SENTINEL).all() and (out2 == SENTINEL).all() and (xcopy == SENTINEL).all()


REFUSED = {
    "9 rows in skinny form": (dict(rows=9, k=36, mode="DENSE"), {}),
    "more than 64 KB of rows in skinny form": (dict(rows=8, k=2052, mode="DENSE"), {}),
    "one value more than 64 KB in skinny form": (dict(rows=1, k=16385, mode="DENSE"), {}),
    "pre in skinny form": (dict(rows=2, k=36, mode="DENSE", pre=True), {}),
    "GRU_ZR with n != 2h": (dict(rows=2, k=36, mode="GRU_ZR"), {"n": 37}),
    "GRU_H without z": (dict(rows=2, k=36, mode="GRU_H"), {"z": None}),
    "RNN with n != h": (dict(rows=2, k=36, mode="RNN"), {"h": 18}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_are_decided_before_any_launch(dev, what):
    """each is Y2H_EINVAL from y2h_rec_step, and no buffer is touched; y2h_rec_skinny_ok says the same of the shapes"""
    spec, override = REFUSED[what]
    h = 19
    c = dict(rows=spec["rows"], k=spec["k"], mis=False, mode=spec["mode"], shortcut=0, out2=True, xcopy=True, h=h,
             n=2 * h if spec["mode"] == "GRU_ZR" else h, bn=0, act="linear")
    a = host_case(c, 3)
    if spec.get("pre"):
        a["pre"], a["x_with_pre"] = np.zeros((c["rows"], c["n"]), F), True
    a["override"] = override
    run = Launch(dev, a)
    status, out, out2, xcopy, state = run.run(darknet.REC_SKINNY)
    assert status == darknet.Y2H_EINVAL
    assert (out == SENTINEL).all() and (out2 == SENTINEL).all() and (xcopy == SENTINEL).all()
    assert np.array_equal(state[1:-1], a["state"])
    fits = spec["rows"] <= 8 and spec["rows"] * spec["k"] * 4 <= 65536
    assert dev.L.y2h_rec_skinny_ok(spec["rows"], spec["k"]) == int(fits)
    assert ("skinny form" in what and "pre" not in what) == (not fits)


@pytest.mark.gpu
def test_skinny_ok_at_its_edges(dev):
    ok = dev.L.y2h_rec_skinny_ok
    assert [ok(r, 36) for r in (0, 1, 8, 9)] == [0, 1, 1, 0]
    assert [ok(8, k) for k in (0, 1, 2048, 2049)] == [0, 1, 1, 0]
    assert [ok(1, k) for k in (16384, 16385)] == [1, 0] and ok(3, 5461) == 1 and ok(3, 5462) == 0


# ---- y2h_rnn_sample ----

def _rows_for(rng, seqs, outputs, n, kind):
    if kind == "tiny":                                          # every value below .0001: the sum is zero
        return (rng.random((seqs, outputs), dtype=F) * F(9e-5)).astype(F)
    r = rng.random((seqs, outputs), dtype=F) ** 4               # a softmax-like row: a few large values, many below .0001
    r = (r / r[:, :n].sum(axis=1, keepdims=True)).astype(F)
    if kind == "short":                                         # sums below 1
        r = (r * F(.5)).astype(F)
    return r


def _sample(dev, rows, n, u, prev):
    """one y2h_rnn_sample launch with probs set; returns (next, x, probs), the guards checked"""
    seqs, outputs = rows.shape
    u = np.asarray(u, F)
    prev = np.asarray(prev, np.int32)
    x = np.zeros((seqs + 2, n), F)
    x[[0, -1]] = SENTINEL
    x[np.arange(1, seqs + 1), prev] = 1
    nxt = np.full(seqs + 2, -77, np.int32)
    probs = np.full((seqs + 2, outputs), SENTINEL, F)
    d_out, d_u, d_prev, d_x, d_next, d_probs = (dev.put(v) for v in (rows, u, prev, x, nxt, probs))
    assert dev.L.y2h_rnn_sample(d_out, outputs, n, seqs, d_u, d_prev, d_next.value + 4, d_x.value + n * 4,
                                d_probs.value + outputs * 4, None) == 0
    x, nxt, probs = dev.get(d_x, x.shape), dev.get(d_next, nxt.shape, np.int32), dev.get(d_probs, probs.shape)
    assert (x[[0, -1]] == SENTINEL).all() and (probs[[0, -1]] == SENTINEL).all() and nxt[0] == -77 and nxt[-1] == -77
    assert np.array_equal(dev.get(d_out, rows.shape), rows), "the sampled rows were written"
    return nxt[1:-1], x[1:-1], probs[1:-1]


def _check_draws(dev, rows, n, u, prev):
    nxt, x, probs = _sample(dev, rows, n, u, prev)
    want = [sample_rule(rows[b], u[b], n)[0] for b in range(rows.shape[0])]
    assert nxt.tolist() == want
    onehot = np.zeros_like(x)
    onehot[np.arange(len(want)), want] = 1
    assert np.array_equal(x, onehot), "the input rows are not one-hot at the drawn character"
    assert np.array_equal(probs, rows)                          # the copy covers `outputs` values, the draw n
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 7, 8, 9, 30, 33, 256])
def test_sampler_is_the_rule(dev, n):
    rng = np.random.default_rng(n)
    for outputs in (n, n + 5):                                  # outputs > n: values past n are copied, never drawn
        for kind in ("full", "short"):
            rows = _rows_for(rng, 3, outputs, n, kind)          # 3 sequences at once, each its own row, uniform and prev
            _check_draws(dev, rows, n, rng.random(3, dtype=F), rng.integers(0, n, size=3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 9, 256])
def test_sampler_edges(dev, n):
    rng = np.random.default_rng(100 + n)
    outputs = n + 3
    full, short, tiny = (_rows_for(rng, 3, outputs, n, kind) for kind in ("full", "short", "tiny"))
    prev = rng.integers(0, n, size=3)
    full[0, 0] = F(.25)                                         # u = 0 stops at the first value, whatever follows
    assert _check_draws(dev, full, n, np.zeros(3, F), prev)[0] == 0
    _check_draws(dev, short, n, np.ones(3, F), prev)            # u = 1 on rows that sum below 1
    _check_draws(dev, full, n, np.ones(3, F), prev)
    assert _check_draws(dev, tiny, n, rng.random(3, dtype=F), prev) == [n - 1] * 3      # a zero sum: nothing qualifies
    peaked = np.zeros((3, outputs), F)                          # prev[b] == next[b]: the 1 is cleared, then set again
    at = rng.integers(0, n, size=3)
    peaked[np.arange(3), at] = 1
    assert _check_draws(dev, peaked, n, np.full(3, .5, F), at) == at.tolist()
