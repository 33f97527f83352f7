"""The half kernels on real-valued data against the half-storage rule of tests/half_rule.py.

The integer-data tests (tests/test_gpu_fp16.py, the f16 part of tests/test_gpu_tiles.py, DIRECT_F16_CASES of
tests/test_gpu_conv_forms.py, tests/test_gpu_dense_f16.py) pin indexing, taps, tile edges and K order exactly, and by
construction see none of the arithmetic that only exists in this mode: the rounding of the weights to half, the one rounding
of the store, the folded batch-norm epilogue, the fused pool on raw accumulators with a negative alpha.  Here every kernel
form runs on real-valued inputs, weights and batch-norm statistics (the same shapes and switches as the integer tests) and
every stored element must lie between the two halves the float64 result moved by the rule's delta rounds to; at least 3/4 of
the elements of every layer are pinned to a single half that way.  The cases are data in tests/half_rule.py (CASES), where
tests/test_half_rule_host.py checks their premises and that eight wrong variants of the arithmetic fail this rule.

Logistic is left out (its device form uses __expf, whose error bound is not stated in this tree): layers with it are
skipped and the skip is printed by name.  [normalization] and [activation] keep the tests they have."""
import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import half_rule as R
from tests.helpers import materialize
from tests.layer_rule import read_weights

pytestmark = pytest.mark.gpu


def _open(cfg, wts, fuse=True):
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    net.set_half(True)
    if not fuse:
        net.set_fusion(False)
    return net


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.ident)
def test_half_kernel_values_follow_the_rule(workdir, monkeypatch, case):
    for k in R.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    cfg, wts, x, params = R.materialize(workdir, case)
    L = darknet.lib()
    before = getattr(L, case.counter)() if case.counter else 0
    net = _open(cfg, wts, case.fuse)
    net.network_predict(x)
    names = [net.layer_kernel(i) for i in range(net.n)]
    print(case.ident, names)
    rows = R.check_network(net, x, params)
    moved = getattr(L, case.counter)() - before if case.counter else 1
    last = net.pull_layer_output(net.n - 1)
    net.free()
    for layer, name, exact in case.kernels:
        assert names[layer] == name if exact else names[layer].startswith(name), names
    assert moved > 0, case.counter
    assert not R.failures(rows)
    assert sum(r.what in ("half", "f32") for r in rows) == sum(p["type"] in ("convolutional", "connected", "local", "avgpool") for p in params)
    if case.edit:
        li, what = case.edit
        alpha, beta = R.fold(params[li])
        out = last.reshape(case.batch, params[-1]["out_c"], -1)
        if what == "zero_scale":
            want = R.activate(beta[5:6].astype(np.float64), params[li]["activation"])
            assert alpha[5] == 0 and np.array_equal(out[:, 5], np.broadcast_to(R.half(want).astype(np.float32), out[:, 5].shape))
        elif what == "negative_alpha":
            assert (alpha < 0).all()
        elif what == "overflow":
            assert np.isinf(out[:, 3]).sum() > 10 and np.isfinite(out).mean() > 0.99


@pytest.mark.parametrize("name,size,batch", R.WHOLE_NETWORKS)
def test_whole_networks_follow_the_rule_layer_by_layer(workdir, name, size, batch):
    """route, reorg, the unfused maxpools, the fp32 conv in front of [region], the half avgpool: every layer of the network
    from the stored activations of its producers"""
    cfg, wts, _ = materialize(workdir, name, size, batch, R.WHOLE_SEED, 1.0)
    x = synth.image_batch(batch, 3, size, size, seed=R.WHOLE_INPUT_SEED)
    layers = zoo.resolve(name, size)
    params = R.attach(layers, read_weights(wts, layers))
    net = _open(cfg, wts)
    net.network_predict(x)
    print("%s %d b%d" % (name, size, batch), [net.layer_kernel(i) for i in range(net.n)])
    rows = R.check_network(net, x, params)
    net.free()
    assert not R.failures(rows)
    skipped = [r for r in rows if r.what.startswith("skipped")]
    assert all(r.what.split(": ")[1] in R.HEADS + ("logistic",) for r in skipped), [r.what for r in skipped]
    convs = sum(l["type"] == "convolutional" for l in layers)
    assert sum(r.what in ("half", "f32") and "conv" in r.kernel for r in rows) == convs
    if name == "mini-mfma":
        assert {"route", "reorg", "maxpool"} <= {params[r.layer]["type"] for r in rows if r.what == "select"}
        assert [r.what for r in rows if params[r.layer]["type"] == "convolutional"][-1] == "f32"
