#!/usr/bin/env python3
"""`darknet nightmare` on the device: run_nightmare (nightmare.c:182-307) with the reference's options, the picture kept in
HBM between the steps of a round (y2_nightmare).

    python tools/nightmare.py cfg/vgg-conv.cfg vgg-conv.weights picture.png 10 [-range 1] [-norm 1] [-rounds 1] [-iters 10]
                              [-octaves 4] [-zoom 1.] [-rate .04] [-thresh 1.] [-rotate 0] [-prefix DIR] [-seed 0]

The picture is a .npy file (float [3][h][w] in 0..1, or uint8 [h][w][3]) or a PNG / baseline JPEG / binary PNM read by the
library's own reader (y2_decode_image_rgb), as load_image_color scales it: bytes / 255.  One output per round, named as the
reference names them, <picture>_<cfg>_<layer>_<round>, written as .npy (float32 [3][h][w]) and as a binary .ppm; the round's
picture then goes through rotate, zoom and resize on the device.  -reconstruct is not implemented.
srand(-seed) comes first, as run_nightmare's srand(0)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet  # noqa: E402


def read_picture(path):
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype == np.uint8:
            a = a.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
        return np.ascontiguousarray(a, dtype=np.float32)
    L = darknet.lib()
    L.y2_decode_image_rgb.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_ubyte)), C.c_char_p, C.c_int]
    L.y2_free_image_rgb.argtypes = [C.POINTER(C.c_ubyte)]
    w, h, p = C.c_int(0), C.c_int(0), C.POINTER(C.c_ubyte)()
    err = C.create_string_buffer(256)
    if L.y2_decode_image_rgb(path.encode(), C.byref(w), C.byref(h), C.byref(p), err, 256) != 0:
        sys.exit("%s: %s" % (path, err.value.decode()))
    a = np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    L.y2_free_image_rgb(p)
    return np.ascontiguousarray(a.astype(np.float32).transpose(2, 0, 1) / np.float32(255))


def write_picture(stem, pic):
    np.save(stem + ".npy", pic)
    rgb = (np.nan_to_num(pic, nan=0.0).clip(0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)
    with open(stem + ".ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb).tobytes())


def base(path):
    return os.path.splitext(os.path.basename(path))[0]         # utils.c basecfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, prefix_chars="-")
    ap.add_argument("cfg")
    ap.add_argument("weights")
    ap.add_argument("picture")
    ap.add_argument("layer", type=int)
    for name, kind, default in (("range", int, 1), ("norm", int, 1), ("rounds", int, 1), ("iters", int, 10), ("octaves", int, 4),
                                ("zoom", float, 1.), ("rate", float, .04), ("thresh", float, 1.), ("rotate", float, 0.), ("seed", int, 0)):
        ap.add_argument("-" + name, type=kind, default=default)
    ap.add_argument("-prefix", default=None)
    a = ap.parse_args()
    net = darknet.Network.parse_network_cfg(a.cfg)
    net.load_weights(a.weights)
    net.set_batch_network(1)
    pic = read_picture(a.picture)
    stem = "%s_%s_%d_" % (base(a.picture), base(a.cfg), a.layer)
    if a.prefix:
        os.makedirs(a.prefix, exist_ok=True)
        stem = os.path.join(a.prefix, stem)

    def per_round(r, p):
        write_picture("%s%06d" % (stem, r), p)
        print("%d %s%06d" % (r, stem, r))
    # the first device work of the process comes before srand: the HIP runtime draws from libc's rand() while it starts up
    warm = net.dream_open(pic)
    warm.round_end(0., 1.)
    warm.fetch()
    warm.close()
    darknet.srand(a.seed)
    net.nightmare(pic, a.layer, a.range, a.norm, a.rounds, a.iters, a.octaves, a.zoom, a.rate, a.thresh, a.rotate, per_round)
    net.free()


if __name__ == "__main__":
    main()
