"""Detector training without a GPU: the float64 rule (tests/train_det_rule.py) is pinned to the compiled reference's arrays
(goldens E, F and G, tests/golden/gen_train_det_golden.py) within 1e-5 relative per tensor; the fixtures keep the margins
they claim; route / reorg of the rule are permutations that invert each other; the new entry points are exported; the
truth of a [region] network is l.truths floats per image; every new refusal happens before the device is touched and names
the layer."""
import subprocess

import numpy as np
import pytest

from sr_object_detection_amd import darknet
from tests import train_det_rule as D
from tests import train_rule as T
from tests.helpers import load_golden

RULE_BOUND = 1e-5
_CACHE = {}


def rule_run(name):
    if name not in _CACHE:
        g = load_golden("train_" + name)
        _CACHE[name] = (g,) + D.rule_snapshots(name, int(g["seed"]))
    return _CACHE[name]


@pytest.mark.parametrize("name", ["E", "F", "G"])
def test_rule_is_the_reference(name):
    g, t, snaps, losses, _ = rule_run(name)
    checked = 0
    for key in g:
        if key.startswith("s") and key.endswith("_loss"):
            k = int(key[1])
            e = abs(float(g[key][0]) - losses[k - 1]) / abs(losses[k - 1])
        elif key.startswith("s") and "_l" in key:
            k, i, a = int(key[1]), int(key.split("_")[1][1:]), key.split("_", 2)[2]
            e = T.err(g[key], snaps[k - 1][i][a].reshape(-1))
        else:
            continue
        assert e <= RULE_BOUND, "%s %s: rule vs reference %.3g" % (name, key, e)
        checked += 1
    assert checked > 60
    # step 1 holds every array of every layer, in full
    for i, l in enumerate(D.NETS[name]["layers"]):
        for a in (T.CONV_ARRAYS if l[0] == "conv" and l[4] else ("output", "delta")):
            assert g["s1_l%d_%s" % (i, a)].size == snaps[0][i][a].size


@pytest.mark.parametrize("name", ["E", "F", "G"])
def test_fixture_keeps_its_margins(name):
    g, t, _, _, stats = rule_run(name)
    assert D.margins_ok(t), (t.min_preact, t.min_gap, t.margins)
    assert t.min_preact == float(g["min_preact"])
    for k in ("thresh", "anchor", "recall", "cell"):
        assert t.margins[k] == float(g["margin_" + k]) >= T.KINK
    reg = D.NETS[name]["layers"][-1][1]
    if name == "E":
        assert t.margins["max_best_iou"] > reg["thresh"]           # the thresh branch is taken
        assert stats[0]["count"] == 4 and D.truths("E", 1)[1, 0, 0] == 0  # image 1 has no truth
        assert D.NETS["E"]["seen"] + D.STEPS * D.NETS["E"]["batch"] < 12800
    elif name == "F":
        assert D.NETS["F"]["seen"] >= 12800 and stats[0]["count"] == 3


def test_multi_writer_deltas_of_F():
    """layer 2 is written by the route behind it and by its successor; layer 5 only by a route; layer 8 (reorg) only by a
    route: none of those deltas is zero, and layer 2's is not its successor's contribution alone"""
    _, t, snaps, _, _ = rule_run("F")
    for i in (2, 5, 8):
        assert np.abs(snaps[0][i]["delta"]).max() > 0
    layers = D.NETS["F"]["layers"]
    assert layers[6] == ("route", (-4,)) and layers[9] == ("route", (-1, -4)) and layers[8] == ("reorg", 2)


def test_reorg_assigns_the_delta_of_the_route_in_front_of_it_in_G():
    """layer 5 (route) is written by the reorg behind it alone, an assignment; layer 2 by that route and by its successor;
    layer 4, whose successor is a route that does not read it, by the last route alone"""
    _, t, snaps, _, _ = rule_run("G")
    layers = D.NETS["G"]["layers"]
    assert layers[5] == ("route", (-3,)) and layers[6] == ("reorg", 2) and layers[7] == ("route", (-1, -3))
    d5, d6 = snaps[0][5]["delta"], snaps[0][6]["delta"]
    assert np.array_equal(d5, D.reorg_backward(d6, 2, 8, 6, 8)) and np.abs(d5).max() > 0
    assert np.array_equal(snaps[0][4]["delta"] != 0, np.ones_like(snaps[0][4]["delta"], bool))


@pytest.mark.parametrize("c,h,w,s", [(4, 6, 4, 2), (8, 4, 6, 2), (12, 2, 4, 2), (9, 3, 6, 3)])
def test_rule_reorg_is_a_permutation_and_backward_inverts_it(c, h, w, s):
    x = np.arange(2 * c * h * w, dtype=np.float64).reshape(2, c, h, w) + 1
    y = D.reorg_forward(x, s)
    assert y.shape == (2, c * s * s, h // s, w // s) and np.array_equal(np.sort(y.reshape(-1)), x.reshape(-1))
    assert np.array_equal(D.reorg_backward(y, s, c, h, w), x)


def test_region_rule_skips_truths_outside_the_grid_and_honours_the_terminator():
    reg = dict(D.E_REGION)
    rng = np.random.RandomState(5)
    x = rng.randn(2, 27, 5, 6) * .3
    truth = np.zeros((2, 150), np.float32)
    truth[0, :5] = (.3, .4, .2, .3, 1)
    base = D.region_train(x, truth, reg, 12800)
    more = truth.copy()
    more[0, 5:10] = (1.0, .4, .2, .3, 1)            # x == 1.0: cell w, outside
    skipped = D.region_train(x, more, reg, 12800)
    # the skipped truth still takes part in phase (a)'s best IoU, so compare the counts and the phase (b) rows only
    assert skipped[3]["count"] == base[3]["count"] == 1
    after = truth.copy()
    after[0, 10:15] = (.5, .5, .2, .2, 0)           # behind the terminator (row 1 has x == 0)
    assert np.array_equal(D.region_train(x, after, reg, 12800)[1], base[1])


def test_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", darknet.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    want = {"y2_train_region_stats", "y2_train_truth_floats", "y2h_train_region_loss", "y2h_train_region_scratch_bytes",
            "y2h_train_route_forward", "y2h_train_route_backward", "y2h_train_reorg_backward", "y2h_train_add"}
    assert want <= have, sorted(want - have)


def test_truth_is_sized_by_the_region_layer(tmp_path):
    """150 floats per image behind a [region] head; a classifier keeps its [cost] layer's inputs.  No device is touched."""
    cfg, wts, _ = D.materialize(str(tmp_path), "E", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    assert net.truth_floats() == 150
    with pytest.raises(ValueError):
        net.train_step(np.zeros(net.net.batch * net.net.inputs, np.float32), np.zeros(net.net.batch * net.net.layers[net.net.n - 1].inputs, np.float32))
    net.free()
    cfg, _, _ = T.materialize(str(tmp_path), "A", 1)
    net = darknet.Network.parse_network_cfg(cfg)
    assert net.truth_floats() == 5
    net.free()


HEAD = "[net]\nbatch=2\nwidth=6\nheight=6\nchannels=3\n[convolutional]\nfilters=12\nsize=1\nstride=1\npad=1\nactivation=linear\n"
REGION = "[region]\nanchors=1,1,2,2\nclasses=1\ncoords=4\nnum=2\nsoftmax=1\n"
CONV4 = "[convolutional]\nfilters=4\nsize=3\nstride=1\npad=1\nactivation=leaky\n"
DET_REFUSALS = {
    # {tree}: a one-node tree; {map}: a one-line map
    "region_tree": (HEAD + REGION + "tree={tree}\n", r"layer 1 \(region\).*tree"),
    "region_map": (HEAD + REGION + "map={map}\n", r"layer 1 \(region\).*map"),
    "region_classfix": (HEAD + REGION + "classfix=1\n", r"layer 1 \(region\).*classfix"),
    "region_no_softmax": (HEAD + REGION.replace("softmax=1\n", ""), r"layer 1 \(region\).*softmax=1"),
    "region_not_last": (HEAD + REGION + "[route]\nlayers=-2\n", r"layer 1 \(region\).*last layer"),
    "reorg_reverse": ("[net]\nbatch=2\nwidth=6\nheight=6\nchannels=3\n" + CONV4 + "[reorg]\nstride=2\nreverse=1\n"
                      "[convolutional]\nfilters=12\nsize=1\nstride=1\npad=1\nactivation=linear\n" + REGION, r"layer 1 \(reorg\).*reverse"),
    "route_in_classifier": ("[net]\nbatch=2\nwidth=6\nheight=6\nchannels=3\n" + CONV4 + "[route]\nlayers=-1\n[avgpool]\n[softmax]\n[cost]\n",
                            r"layer 1 \(route\).*\[region\]"),
    "reorg_in_classifier": ("[net]\nbatch=2\nwidth=6\nheight=6\nchannels=3\n" + CONV4 + "[reorg]\nstride=2\n[avgpool]\n[softmax]\n[cost]\n",
                            r"layer 1 \(reorg\).*\[region\]"),
    "strided_conv_in_detector": ("[net]\nbatch=2\nwidth=12\nheight=12\nchannels=3\n[convolutional]\nfilters=12\nsize=3\nstride=2\npad=1\n"
                                 "activation=linear\n" + REGION, r"layer 0 \(convolutional\).*stride 2"),
}


def det_refusal_net(tmp_path, what):
    text, pattern = DET_REFUSALS[what]
    tree, mp = str(tmp_path / "one.tree"), str(tmp_path / "one.map")
    with open(tree, "w") as f:
        f.write("a -1\n")
    with open(mp, "w") as f:
        f.write("0\n")
    cfg = str(tmp_path / "r.cfg")
    with open(cfg, "w") as f:
        f.write(text.replace("{tree}", tree).replace("{map}", mp))
    return darknet.Network.parse_network_cfg(cfg), pattern


@pytest.mark.parametrize("what", sorted(DET_REFUSALS))
def test_new_refusals_name_the_layer(tmp_path, what):
    net, pattern = det_refusal_net(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=pattern):
        net.train_prepare()
    with pytest.raises(darknet.Y2Error, match=pattern):      # train_network_datum prepares lazily and refuses alike
        net.train_step(np.zeros(net.net.batch * net.net.inputs, np.float32), np.zeros(net.net.batch * 150, np.float32))
    net.free()
