"""The rule of the hierarchical classifier head ([softmax] tree=), stated in numpy float32: read_tree's grouping
(tree.c:53-101), the per-group softmax of softmax_tree (softmax_layer.c:35-47; every group through the oracle's softmax,
which is pinned to blas.c:205), hierarchy_predictions (tree.c:37-51) and get_hierarchy_probability (tree.c:27-35), and the
named trees the fixtures, the host tests and the GPU tests are made of."""
from __future__ import annotations

import os
import tempfile

import numpy as np

from oracle import oracle_capi
from sr_object_detection_amd import synth

F = np.float32


class Tree:
    """what read_tree makes of a parent list: n, parent, groups, group_size, group_offset, group (every node's group) and
    leaf.  The running group closes whenever the parent CHANGES from one line to the next (tree.c:72-80), so siblings that
    are separated by another parent's children form separate groups; a first node with a parent opens with an empty group."""

    def __init__(self, parents):
        self.parent = np.asarray(parents, dtype=np.int32)
        self.n = n = int(self.parent.size)
        size, offset, group = [], [], np.zeros(n, np.int32)
        last, run = -1, 0
        for j, p in enumerate(self.parent.tolist()):
            if p != last:
                offset.append(j - run)
                size.append(run)
                run, last = 0, p
            group[j] = len(size)
            run += 1
        offset.append(n - run)
        size.append(run)
        self.groups = len(size)
        self.group_size = np.asarray(size, np.int32)
        self.group_offset = np.asarray(offset, np.int32)
        self.group = group
        self.leaf = np.ones(n, np.int32)
        self.leaf[self.parent[self.parent >= 0]] = 0
        self.names = ["n%08d" % i for i in range(n)]

    @property
    def parents_first(self) -> bool:
        """every parent precedes its child: the level-parallel walk applies"""
        return bool(np.all(self.parent < np.arange(self.n)))

    @property
    def depth(self) -> np.ndarray:
        """ancestors of every node (0 for a root), whatever the order of the nodes"""
        d = np.zeros(self.n, np.int32)
        for j in range(self.n):
            c = int(self.parent[j])
            while c >= 0:
                d[j] += 1
                c = int(self.parent[c])
        return d

    def levels(self):
        """(order, level_off): the nodes sorted by depth and the offset of every level, as the plan uploads them"""
        d = self.depth
        order = np.argsort(d, kind="stable").astype(np.int32)
        off = np.searchsorted(d[order], np.arange(int(d.max()) + 2)).astype(np.int32)
        return order, off

    def write(self, path: str) -> str:
        with open(path, "w") as f:
            for name, p in zip(self.names, self.parent.tolist()):
                f.write("%s %d\n" % (name, p))
        return path

    def leaves_from(self, names) -> np.ndarray:
        """change_leaves (tree.c:7-25): the leaf flags after the listed names became the leaves"""
        keep = set(names)
        return np.asarray([1 if nm in keep else 0 for nm in self.names], np.int32)


def softmax_tree(rows: np.ndarray, tree: Tree, temp: float = 1.0) -> np.ndarray:
    """rows [r][tree.n]: softmax(in + off[g], size[g], temp, out + off[g]) for every group of every row"""
    rows = np.ascontiguousarray(rows, dtype=F).reshape(-1, tree.n)
    out = np.zeros_like(rows)
    with np.errstate(all="ignore"):
        for r in range(rows.shape[0]):
            for o, s in zip(tree.group_offset.tolist(), tree.group_size.tolist()):
                if s > 0:
                    out[r, o:o + s] = oracle_capi.softmax(rows[r, o:o + s], temp)
    return out


def hierarchy_predictions(p: np.ndarray, tree: Tree, only_leaves: bool = False, leaf=None) -> np.ndarray:
    """p[j] *= p[parent[j]] for j ascending -- a child that stands before its parent meets the parent's value as it was --
    then p[j] = 0 where !leaf[j].  One row or [r][n] rows; returns a copy."""
    p = np.array(p, dtype=F, copy=True)
    flat = p.reshape(-1, tree.n)
    par = tree.parent.tolist()
    if tree.parents_first:
        order, off = tree.levels()
        for lv in range(1, len(off) - 1):                       # level by level: the same products
            js = order[off[lv]:off[lv + 1]]
            flat[:, js] = flat[:, js] * flat[:, tree.parent[js]]
    else:
        for j in range(tree.n):
            if par[j] >= 0:
                flat[:, j] = flat[:, j] * flat[:, par[j]]
    if only_leaves:
        flat[:, np.asarray(tree.leaf if leaf is None else leaf) == 0] = 0
    return p


def hierarchy_sequential(p: np.ndarray, tree: Tree) -> np.ndarray:
    """the loop of tree.c:40-45 as it stands, one row"""
    p = np.array(p, dtype=F, copy=True)
    for j, par in enumerate(tree.parent.tolist()):
        if par >= 0:
            p[j] = F(p[j] * p[par])
    return p


def get_hierarchy_probability(x: np.ndarray, tree: Tree, c: int) -> np.float32:
    p = F(1)
    while c >= 0:
        p = F(p * F(x[c]))
        c = int(tree.parent[c])
    return p


# ---- the named trees, as parent lists ------------------------------------------------------------------------------
FLAT = [-1] * 7                                   # 7 roots, one group
# 24 nodes, four levels: root 2 has no child, node 8 is a child of 0 behind the children of 1 (siblings in two groups, and
# a group of one), node 13 is the only child of 4
MINI = [-1, -1, -1, 0, 0, 0, 1, 1, 0, 3, 3, 3, 3, 4, 6, 6, 6, 9, 9, 10, 10, 10, 14, 14]
BACK = list(MINI)
BACK[8] = 9                                       # node 8 stands before its parent
WIDE = [-1] * 3 + [0] * 700                       # a group larger than any workgroup


def _synth(n: int, roots: int = 10):
    with tempfile.TemporaryDirectory() as tmp:
        return synth.write_tree(os.path.join(tmp, "t"), n, roots)["parents"]


_CACHE: dict = {}
NAMES = ("FLAT", "MINI", "BACK", "WIDE", "MANY", "BIG", "NINE_K")


def tree(name: str) -> Tree:
    """MANY: synth.write_tree(5000, 3), more groups than a workgroup has threads; BIG: 16500 nodes, a row past the 64 KB
    LDS budget; NINE_K: synth.write_tree(9418), the yolo9000 tree"""
    if name not in _CACHE:
        parents = {"FLAT": lambda: FLAT, "MINI": lambda: MINI, "BACK": lambda: BACK, "WIDE": lambda: WIDE,
                   "MANY": lambda: _synth(5000, 3), "BIG": lambda: _synth(16500), "NINE_K": lambda: _synth(9418)}[name]()
        _CACHE[name] = Tree(parents)
    return _CACHE[name]


# ---- the test networks: the trunk of tta_rule's mini classifier with a 24-way tree head ----------------------------
MINI_CLASSES = 24


def mini_spec(tree_path: str, temperature: float = 1.0, groups: int = 1):
    """tta_rule.MINI_SPEC with groups * 24 outputs and [softmax] tree="""
    head = {"tree": tree_path, "groups": groups}
    if temperature != 1.0:
        head["temperature"] = temperature
    return [("conv", 16, 3, 1, "leaky"), ("max", 2, 2), ("conv", 32, 3, 1, "leaky"), ("max", 2, 2),
            ("conv", MINI_CLASSES * groups, 1, 0, "linear"), ("avg",), ("softmax", head), ("cost",)]


# the cfgs of tests/golden/hier_mini.npz: name -> (tree, temperature, groups)
MINI_CFGS = {"mini_t1": ("MINI", 1.0, 1), "mini_t25": ("MINI", 2.5, 1), "back_t1": ("BACK", 1.0, 1), "back_t25": ("BACK", 2.5, 1),
             "mini_g2": ("MINI", 1.0, 2)}
MINI_BATCH = 3
