#!/usr/bin/env python3
"""Device time of the classifier head at 9418 outputs (engine timing events, median over iterations):
  tree    the [softmax] tree= layer of zoo.HIER["darknet19_9k"] (synth.write_tree's 9418-node tree), and one
          y2h_hierarchy_rows launch on its [batch][9418] output rows (level-parallel form, with and without leaf flags)
  plain   the plain [softmax] layer of the same network without the tree: as many double exps, one group
usage: softmax_tree_times.py tree|plain [size=224] [batches=1,128] [iters=30]
`plain` uses nothing this tool's commit added, so the same file runs in a checkout of an earlier commit."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

OUTPUTS = 9418


def layer_time(spec, size, batch, iters, tree_path=None):
    tmp = tempfile.mkdtemp()
    cfg = os.path.join(tmp, "n.cfg")
    kw = {"tree_path": tree_path} if tree_path else {}
    open(cfg, "w").write(zoo.cfg_text("head", size, size, batch, spec=spec, **kw))
    layers = zoo.resolve(spec, size)
    wts = os.path.join(tmp, "n.weights")
    synth.write_weights(wts, layers, 7)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    x = synth.image_batch(batch, 3, size, size)
    net.set_timing(True)
    i = [l["type"] for l in layers].index("softmax")
    ts = []
    for _ in range(iters + 3):
        net.network_predict(x)
        ts.append(net.layer_times_ms())
    t = np.array(ts[3:])
    return net, i, float(np.median(t[:, i])), float(t[:, i].min()), float(np.median(t.sum(axis=1)))


def hierarchy_time(net, batch, iters, leaf):
    """one y2h_hierarchy_rows launch on the network's own output rows, between two events on the engine's stream"""
    L = darknet.lib()
    a, b = C.c_void_p(), C.c_void_p()
    L.y2h_event_create(C.byref(a))
    L.y2h_event_create(C.byref(b))
    stream = C.c_void_p(net.stream())
    ms = C.c_float()
    ts = []
    for _ in range(iters + 3):
        net.forward_device(0)               # the engine's own input slot, filled by the predicts before
        L.y2h_event_record(a, stream)
        net.hierarchy_enqueue(leaf)
        L.y2h_event_record(b, stream)
        net.sync()
        L.y2h_event_elapsed_ms(a, b, C.byref(ms))
        ts.append(ms.value)
    L.y2h_event_destroy(a)
    L.y2h_event_destroy(b)
    return float(np.median(ts[3:])), float(min(ts[3:]))


def main():
    what = sys.argv[1]
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 224
    batches = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "1,128").split(",")]
    iters = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    trunk = zoo.SPECS["darknet19"][:-4]
    for batch in batches:
        if what == "plain":
            spec = trunk + [("conv", OUTPUTS, 1, 0, "linear"), ("avg",), ("softmax",), ("cost",)]
            net, i, med, best, fwd = layer_time(spec, size, batch, iters)
            print("plain [softmax] %d outputs, batch %3d: layer %d %-14s %.4f ms median, %.4f ms best of %d (forward %.3f ms)" %
                  (OUTPUTS, batch, i, net.layer_kernel(i), med, best, iters, fwd))
        else:
            spec = zoo.HIER["darknet19_9k"][1]
            net, i, med, best, fwd = layer_time(spec, size, batch, iters)
            print("tree  [softmax] %d outputs, batch %3d: layer %d %-14s %.4f ms median, %.4f ms best of %d (forward %.3f ms)" %
                  (OUTPUTS, batch, i, net.layer_kernel(i), med, best, iters, fwd))
            for leaf in (False, True):
                med, best = hierarchy_time(net, batch, iters, leaf)
                print("      y2h_hierarchy_rows on those %3d rows, only_leaves %d: %.4f ms median, %.4f ms best of %d" % (batch, leaf, med, best, iters))
        net.free()


if __name__ == "__main__":
    main()
