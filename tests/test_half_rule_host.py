"""tests/half_rule.py on the CPU: the rule agrees with the oracle where everything is exact, its fold is pack_dense's, every
case of tests/test_gpu_half_values.py keeps the rule's conditions with the rule's own float32 evaluation standing in for the
device, and each of the eight wrong variants leaves elements outside their intervals: the GPU test can fail."""
import math

import numpy as np
import pytest

from sr_object_detection_amd import synth, zoo
from tests import half_rule as R
from tests.helpers import materialize
from tests.layer_rule import read_weights
from tests.test_gpu_kernels import _small_int_conv_case

F = np.float32


def _as_half(a):
    return a.astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("spec,size,seed", [([("conv", 32, 3, 0, "linear"), ("conv", 128, 3, 0, "linear")], 19, 9162),
                                            ([("conv", 32, 3, 0, "linear"), ("conv", 64, 3, 0, "linear"), ("max", 2, 2)], 24, 9620)],
                         ids=["conv", "conv+maxpool2"])
def test_rule_equals_the_oracle_on_integer_data(oracle, workdir, spec, size, seed):
    """two cases of tests/test_gpu_fp16.py: every product and sum is exact, so the float32 evaluation, the float64 one and the
    oracle rounded once to half are the same values"""
    cfg, wts, x = _small_int_conv_case(workdir, spec, size, 2, seed)
    layers = zoo.resolve(spec, size)
    params = R.attach(layers, read_weights(wts, layers))
    on = oracle.OracleNet(cfg, wts)
    ref = on.predict(x)
    net = R.RuleNet(params, x)
    fused = len(spec) == 3
    assert ("+maxpool2" in net.layer_kernel(1)) == fused
    assert np.abs(on.layer_output(0)).max() <= 2048 and 0 < np.abs(ref).max() < 60000
    assert np.array_equal(net.pull_layer_output(0), _as_half(on.layer_output(0)).reshape(-1))
    assert np.array_equal(net.pull_layer_output(len(spec) - 1), _as_half(ref).reshape(-1))
    rows = R.check_network(net, x, params)
    on.close()
    assert [r.layer for r in rows] == ([0, 2] if fused else [0, 1])
    # (integer data is full of exact zeros: the share condition on the subnormal range is for the real-valued cases)
    assert all(r.equal == 1.0 and r.worst == 0.0 and not len(r.outside) for r in rows)


def test_fold_is_the_float32_of_the_double_formula():
    p = dict(bias=np.array([0.25, -0.1, 0.3], F), scale=np.array([1.25, -0.7, 0.0], F), mean=np.array([0.3, -0.2, 0.1], F),
             var=np.array([0.9, 1.3, 0.5], F))
    alpha, beta = R.fold(p)
    assert alpha.dtype == F and beta.dtype == F
    for f in range(3):
        a = float(p["scale"][f]) / (math.sqrt(float(p["var"][f])) + float(F(.000001)))
        assert alpha[f] == F(a) and beta[f] == F(float(p["bias"][f]) - float(p["mean"][f]) * a)
    a1, b1 = R.fold(p, first=True)                      # the first-layer kernels multiply by the reciprocal: an ulp at the most
    assert np.abs(a1.astype(np.float64) - alpha).max() <= np.spacing(np.abs(alpha)).max() and b1[2] == beta[2] == p["bias"][2]
    alpha, beta = R.fold(dict(bias=p["bias"]))
    assert np.array_equal(alpha, np.ones(3, F)) and np.array_equal(beta, p["bias"])


def test_half_is_round_to_nearest_even_with_infinities():
    v = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.9, 65520.0, -65520.0, 2.0 ** -25, 2.0 ** -25 * 1.01], np.float64)
    assert np.array_equal(R.half(v).astype(np.float64), [1.0, 1 + 2.0 ** -9, 65504.0, np.inf, -np.inf, 0.0, 2.0 ** -24])
    assert np.array_equal(R.trunc_half(np.array([1 + 3 * 2.0 ** -11, -1 - 3 * 2.0 ** -11, 0.5], F)).astype(F), [1 + 2.0 ** -10, -1 - 2.0 ** -10, 0.5])


_NETS = {}
for _c in R.CASES:
    _NETS.setdefault(_c.net_key(), _c)


@pytest.mark.parametrize("case", list(_NETS.values()), ids=lambda c: c.ident)
def test_every_gpu_case_keeps_the_conditions(case):
    """every network of the GPU table (cases that differ only in their switches share one): inside, >= 3/4 pinned, < 1 % tiny"""
    _, layers, arrays, x = R.build_case(case)
    params = R.attach(layers, arrays)
    rows = R.check_network(R.RuleNet(params, x, fuse=case.fuse), x, params)
    assert not R.failures(rows)
    assert sum(r.what in ("half", "f32") for r in rows) >= 1
    if case.edit and case.edit[1] == "overflow":
        got = R.RuleNet(params, x).pull_layer_output(1)
        assert np.isinf(got).sum() > 10 and np.isfinite(got).mean() > 0.99


@pytest.mark.parametrize("name,size,batch", R.WHOLE_NETWORKS)
def test_whole_networks_keep_the_conditions(workdir, name, size, batch):
    cfg, wts, _ = materialize(workdir, name, size, batch, R.WHOLE_SEED, 1.0)
    x = synth.image_batch(batch, 3, size, size, seed=R.WHOLE_INPUT_SEED)
    layers = zoo.resolve(name, size)
    params = R.attach(layers, read_weights(wts, layers))
    rows = R.check_network(R.RuleNet(params, x), x, params)
    assert not R.failures(rows)
    assert sum(r.what in ("half", "f32") for r in rows) == sum(l["type"] in ("convolutional", "avgpool") for l in layers)


def test_case_table_covers_the_listed_forms():
    idents = set(R.CASE_BY_IDENT)
    assert len([i for i in idents if i.startswith("tile-")]) == 7 * 2 * 2 * 2
    assert len([i for i in idents if i.startswith("scalar-store-")]) == 12 and len([i for i in idents if i.startswith("first-")]) == 24
    for c in R.CASES:
        assert c.size <= 48 and c.batch <= 5, c.ident
        assert set(k for k, _ in c.env) <= set(R.SWITCHES), c.ident


@pytest.mark.parametrize("name", R.MUTATIONS)
@pytest.mark.parametrize("ident", R.MUTATION_CASES)
def test_wrong_variants_leave_elements_outside(ident, name):
    case = R.CASE_BY_IDENT[ident]
    _, layers, arrays, x = R.build_case(case)
    params = R.attach(layers, arrays)
    li = case.kernels[0][0]
    K = layers[li]["c"] * layers[li]["size"] ** 2
    assert K == (27 if li == 0 else 576)
    rows = R.check_network(R.RuleNet(params, x, mutate=(li, name)), x, params, echo=lambda s: None)
    row = next(r for r in rows if r.layer == li)
    print("%s, K = %d, %s: share inside %.4f" % (ident, K, name, 1 - len(row.outside) / row.n))
    assert len(row.outside) >= 1
    # and the layers the variant does not touch still pass: the failure is the variant's
    assert not R.failures([r for r in rows if r.layer != li])
