"""CPU-only checks of the hierarchical classifier head ([softmax] tree=): the rule of tests/hier_rule.py reproduces the
reference-run fixture tests/golden/hier_mini.npz bit for bit; the reference's tree API the library exports on the host
(hierarchy_predictions, get_hierarchy_probability, change_leaves) equals it through ctypes; the refusals -- a tree that
does not cover the layer's rows, a net.hierarchy that is not the output head's tree -- come before any device work; a
caller written against the reference's header names compiles and links."""
import ctypes as C
import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet, zoo
from tests import hier_rule as H
from tests import tta_rule as R
from tests.conftest import has_gpu
from tests.helpers import load_golden
from tests.test_native_callers import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("y2h_softmax_tree_rows", "y2h_hierarchy_rows", "y2_hierarchy_enqueue", "y2_classify_frames", "hierarchy_predictions",
           "get_hierarchy_probability", "change_leaves")
SINGLE = [n for n, (_, _, g) in H.MINI_CFGS.items() if g == 1]


@pytest.fixture(scope="module")
def g():
    return load_golden("hier_mini")


def test_library_exports_the_hierarchy_entries():
    L = darknet.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    for name in ("classify", "hierarchy_enqueue"):
        assert hasattr(darknet.Network, name), name
    for name in ("hierarchy_predictions", "get_hierarchy_probability", "change_leaves", "read_tree"):
        assert hasattr(darknet, name), name
    header = open(os.path.join(ROOT, "include", "sr_yolo2.h")).read()
    for name in ENTRIES[2:]:
        assert name + "(" in header, name
    assert "tree.c:37" in header and "tree.c:27" in header and "tree.c:7" in header


def test_read_tree_grouping_of_the_named_trees(g):
    """siblings separated by another parent's children form separate groups; the tables equal the reference's read_tree"""
    mini = H.tree("MINI")
    assert mini.n == 24 and int(mini.depth.max()) == 3
    assert mini.group_size.tolist() == [3, 3, 2, 1, 4, 1, 3, 2, 3, 2]
    assert mini.group[8] != mini.group[3] and mini.parent[8] == mini.parent[3]          # one parent, two groups
    assert mini.leaf[2] == 1 and 2 not in mini.parent                                    # a childless root
    assert H.tree("FLAT").groups == 1 and H.tree("FLAT").group_size.tolist() == [7]
    assert H.tree("WIDE").group_size.max() == 700
    assert H.tree("MANY").groups > 512 and H.tree("BIG").n * 4 > 64 * 1024 and H.tree("NINE_K").n == 9418
    assert not H.tree("BACK").parents_first and all(H.tree(n).parents_first for n in H.NAMES if n != "BACK")
    for name in H.NAMES:
        t = H.tree(name)
        assert np.array_equal(g["tree_%s_group_size" % name], t.group_size), name
        assert np.array_equal(g["tree_%s_group_offset" % name], t.group_offset), name
        assert np.array_equal(g["tree_%s_leaf" % name], t.leaf), name
        assert int(t.group_size.sum()) == t.n and np.array_equal(np.repeat(np.arange(t.groups), t.group_size), t.group), name


@pytest.mark.parametrize("name", list(H.MINI_CFGS))
def test_rule_reproduces_the_reference_fixture(oracle, g, name):
    tname, temp, groups = H.MINI_CFGS[name]
    t = H.tree(tname)
    cond = g[name + "_cond"]
    assert np.array_equal(H.softmax_tree(g[name + "_logits"], t, temp).reshape(cond.shape), cond)
    sums = cond.reshape(-1, t.n)[:, t.group_offset[1]:t.group_offset[1] + t.group_size[1]].sum(axis=1)
    assert np.allclose(sums, 1, atol=1e-6)
    if groups != 1:
        return
    new_leaf = t.leaves_from([t.names[i] for i in g["new_leaves"]])
    assert np.array_equal(new_leaf, g["leaf2"])
    assert np.array_equal(H.hierarchy_predictions(cond, t, False), g[name + "_hp0"])
    assert np.array_equal(H.hierarchy_predictions(cond, t, True), g[name + "_hp1"])
    assert np.array_equal(H.hierarchy_predictions(cond, t, True, leaf=new_leaf), g[name + "_hp1b"])
    assert np.array_equal(np.stack([H.hierarchy_sequential(r, t) for r in cond]), g[name + "_hp0"])
    ghp = np.array([[H.get_hierarchy_probability(r, t, c) for c in range(t.n)] for r in cond], np.float32)
    assert np.array_equal(ghp, g[name + "_ghp"])
    assert np.array_equal(np.stack([R.top_k(r, 3) for r in g[name + "_hp0"]]), g[name + "_top3"])
    for rows in (g[name + "_hp0"], g[name + "_hp1"], g[name + "_hp1b"]):            # the margin the fixture promises
        for r in rows:
            top = np.sort(r.astype(np.float64))[::-1][:4]
            assert np.min(-np.diff(top)) >= 1e-3


def test_a_child_before_its_parent_meets_the_unmultiplied_value(g):
    t = H.tree("BACK")
    cond = g["back_t1_cond"][0]
    hp = g["back_t1_hp0"][0]
    assert hp[8] == np.float32(cond[8] * cond[9]) and hp[9] == np.float32(cond[9] * hp[3])
    assert hp[8] != H.get_hierarchy_probability(cond, t, 8)


@pytest.mark.parametrize("mode", ["crop10", "multi", "full"])
def test_view_sums_of_the_fixture_follow_the_rule(g, mode):
    """the sums are hierarchy_predictions(.., 1) rows added in order -- except MULTI's flipped views, added as they are"""
    t = H.tree("MINI")
    rows = g[mode + "_rows"]
    per = rows.shape[1]
    flat = rows.reshape(-1, t.n)
    hp = H.hierarchy_predictions(flat, t, True)
    flipped = np.array([mode == "multi" and (i % per) % 2 == 1 for i in range(len(flat))])
    sums = R.sums_of(np.where(flipped[:, None], flat, hp), per)
    assert np.array_equal(sums, g[mode + "_sums"])
    assert np.array_equal(np.stack([R.top_k(s, 3) for s in sums]), g[mode + "_top3"])
    if mode == "multi":
        assert np.abs(R.sums_of(hp, per) - sums).max() > 0.1        # the quirk is no rounding matter


def test_host_tree_api_equals_the_reference(g, workdir, capfd):
    for name in SINGLE:
        t = H.tree(H.MINI_CFGS[name][0])
        path = t.write(os.path.join(workdir, "host_%s.tree" % name))
        hier = darknet.read_tree(path)
        assert hier.contents.n == t.n and hier.contents.groups == t.groups
        assert np.array_equal(np.ctypeslib.as_array(hier.contents.leaf, (t.n,)), t.leaf)
        assert np.array_equal(np.ctypeslib.as_array(hier.contents.group, (t.n,)), t.group)
        cond = g[name + "_cond"]
        for r in range(len(cond)):
            assert np.array_equal(darknet.hierarchy_predictions(cond[r], hier, False), g[name + "_hp0"][r])
            assert np.array_equal(darknet.hierarchy_predictions(cond[r], hier, True), g[name + "_hp1"][r])
            ghp = np.array([darknet.get_hierarchy_probability(cond[r], hier, c) for c in range(t.n)], np.float32)
            assert np.array_equal(ghp, g[name + "_ghp"][r])
        leaves = os.path.join(workdir, "host_%s.leaves" % name)
        with open(leaves, "w") as f:
            f.write("".join("%s\n" % t.names[i] for i in g["new_leaves"]) + "no-such-node\n")
        capfd.readouterr()
        darknet.change_leaves(hier, leaves)
        assert "Found %d leaves." % len(g["new_leaves"]) in capfd.readouterr().err
        assert np.array_equal(np.ctypeslib.as_array(hier.contents.leaf, (t.n,)), g["leaf2"])
        for r in range(len(cond)):
            assert np.array_equal(darknet.hierarchy_predictions(cond[r], hier, True), g[name + "_hp1b"][r])


def _hier_net(workdir, tname="MINI", temp=1.0, groups=1, batch=2, classes=H.MINI_CLASSES, tag="hh"):
    path = H.tree(tname).write(os.path.join(workdir, "hh_%s.tree" % tname))
    spec = H.mini_spec(path, temp, groups)
    if classes != H.MINI_CLASSES:
        spec[4] = ("conv", classes * groups, 1, 0, "linear")
    cfg, wts = R.write_mini(workdir, 5, batch=batch, spec=spec, tag="%s_%s_c%d_g%d" % (tag, tname, classes, groups))
    return darknet.Network.parse_network_cfg(cfg)


def test_a_tree_that_does_not_cover_the_rows_is_refused_without_a_device(workdir):
    for classes, groups, want in ((25, 1, ("24 nodes", "= 25")), (23, 1, ("24 nodes", "= 23")), (12, 2, ("24 nodes", "= 12"))):
        net = _hier_net(workdir, classes=classes, groups=groups)
        assert net.net.hierarchy                                          # it parses, as the reference's does
        with pytest.raises(darknet.Y2Error) as e:
            net.prepare()
        assert all(w in str(e.value) for w in want) and "softmax layer" in str(e.value), str(e.value)
        net.free()
    if not has_gpu():                                                     # a good tree is refused by nothing but the missing device
        net = _hier_net(workdir)
        with pytest.raises(darknet.Y2Error) as e:
            net.prepare()
        assert "tree" not in str(e.value) and "device" in str(e.value).lower(), str(e.value)
        net.free()


FRAMES = [np.zeros((3, 40, 50), np.float32), np.zeros((3, 50, 40), np.float32)]
SENTENCE = "hierarchical classifiers (softmax tree=) are not implemented on the device"


def _entry_points(net):
    x = np.zeros((2, 3, 32, 32), np.float32)
    return (lambda: net.classify(x, 3), lambda: net.hierarchy_enqueue(False), lambda: net.validate_classifier_frames(x, [0, 0], 10, 3),
            lambda: net.classifier_view_sums(R.CROP10, FRAMES), lambda: net.classifier_view_sums(R.MULTI, FRAMES, [24]),
            lambda: net.classifier_view_sums(R.FULL, FRAMES))


def test_a_foreign_hierarchy_is_refused_by_every_entry_point(workdir):
    """a tree hung on a flat classifier, and a head with groups=2 (rows of outputs/2): the sentence, and both numbers"""
    cfg, _ = R.write_mini(workdir, 5, batch=2)
    flat = darknet.Network.parse_network_cfg(cfg)
    tree = darknet.Tree()
    flat.net.hierarchy = C.pointer(tree)
    for call in _entry_points(flat):
        with pytest.raises(darknet.Y2Error) as e:
            call()
        assert SENTENCE in str(e.value) and "n = 0, outputs = 10" in str(e.value), str(e.value)
    flat.net.hierarchy = None
    with pytest.raises(darknet.Y2Error, match="no hierarchy"):
        flat.hierarchy_enqueue(False)
    flat.free()
    g2 = _hier_net(workdir, groups=2)
    for call in _entry_points(g2):
        with pytest.raises(darknet.Y2Error) as e:
            call()
        assert SENTENCE in str(e.value) and "n = 24, outputs = 48" in str(e.value), str(e.value)
    g2.free()


def test_the_head_own_hierarchy_is_refused_by_nothing_but_the_device(workdir):
    if has_gpu():
        return                    # with a device the calls run: tests/test_gpu_hier.py
    net = _hier_net(workdir)
    for call in _entry_points(net):
        with pytest.raises(darknet.Y2Error) as e:
            call()
        assert SENTENCE not in str(e.value), str(e.value)
    net.free()


def test_classifier_like_caller_compiles_against_the_reference_header_names(workdir):
    build(workdir, "classifier_like", "gcc", "classifier_like.c")


def test_zoo_spec_forms(workdir):
    text = zoo.cfg_text("x", 32, 32, 2, spec=H.mini_spec("/some/where.tree", 2.5, 2))
    assert "[softmax]\ngroups=2\ntemperature=2.5\ntree=/some/where.tree\n" in text
    assert "[softmax]\ngroups=1\n\n" in zoo.cfg_text("x", 32, 32, 2, spec=R.MINI_SPEC)      # the plain form is what it was
    size, spec = zoo.HIER["darknet19_9k"]
    text = zoo.cfg_text("darknet19_9k", 64, 64, 2, spec=spec)
    path = [l for l in text.splitlines() if l.startswith("tree=")][0][5:]
    assert sum(1 for _ in open(path)) == 9418 and "filters=9418" in text
    assert zoo.resolve(spec, 64)[-2]["outputs"] == 9418
