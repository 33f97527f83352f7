#!/usr/bin/env python3
"""The tile plan of the fp32 matrix-core convolutions WITHOUT a GPU: for every conv layer of a zoo network at a given size and
batch, what pick_variant (y2_conv.hip, host arithmetic only) would launch -- kernel name and the candidate list.  Used to
check that a change of the cost model leaves the plan of the headline configuration alone.
    tools/plan_dump.py yolo 608 32 [yolo 416 8 ...]
    tools/plan_dump.py --sweep       every dispatch query for every zoo network, a digest per configuration (tests/golden/conv_plan_table.txt)
    tools/plan_dump.py --sweep-rows  the same queries, one line per conv layer: diff two builds' output (Y2_LIB) to see what moved
    tools/plan_dump.py --wino        the Winograd rule's answer for every 3x3 layer of every zoo network (tests/golden/wino_plan_table.txt)
    tools/plan_dump.py --winos       the stationary-Winograd rule's answer for the same layers (tests/golden/winos_plan_table.txt)
    tools/plan_dump.py --wino-split  the split rule's answer for the same layers (tests/golden/wino_split_plan_table.txt)
    tools/plan_dump.py --splitd      the direct split rule's answer for the same layers (tests/golden/splitd_plan_table.txt)
    tools/plan_dump.py --forms       the form the four rules together give each of those layers, and its kernel name (y2_conv_layer_form)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import zoo  # noqa: E402


class Conv(C.Structure):          # include/y2_hip.h: y2h_conv
    _fields_ = [("batch", C.c_int), ("h", C.c_int), ("w", C.c_int), ("c", C.c_int), ("ldx", C.c_int), ("x_halo", C.c_int),
                ("n", C.c_int), ("size", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
                ("ldy", C.c_int), ("fuse_maxpool2", C.c_int), ("batch_normalize", C.c_int), ("activation", C.c_int),
                ("x", C.c_void_p), ("w_packed", C.c_void_p), ("w_ref", C.c_void_p), ("mean", C.c_void_p), ("rinv", C.c_void_p),
                ("scale", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("x_f16", C.c_int), ("y_f16", C.c_int), ("alpha", C.c_void_p), ("beta", C.c_void_p),
                ("tile_bm", C.c_int), ("tile_bn", C.c_int), ("ksplit", C.c_int), ("x_nchw", C.c_int)]


ACT = {"linear": 0, "leaky": 1, "logistic": 2, "relu": 3}
ALIGNED, MISALIGNED = 0x30000, 0x30004          # y: 16-byte aligned, or not (the vec_ok branches)


def _descs(net, size, batch, half, y):
    """The descriptors of a zoo network's conv layers as the engine would build them (no device pointers needed)."""
    layers = zoo.resolve(net, size)
    for i, l in enumerate(layers):
        if l["type"] != "convolutional":
            continue
        pool = i + 1 < len(layers) and layers[i + 1]["type"] == "maxpool" and layers[i + 1]["size"] == 2 and layers[i + 1]["stride"] == 2
        base = dict(batch=batch, h=l["h"], w=l["w"], c=l["c"], ldx=l["c"], n=l["filters"], size=l["size"], stride=l["stride"],
                    pad=l["pad"], out_h=l["out_h"], out_w=l["out_w"], ldy=l["filters"], fuse_maxpool2=1 if pool else 0,
                    batch_normalize=l.get("batch_normalize", 0), activation=ACT.get(l["activation"], 0),
                    x=0x10000, w_packed=0x20000, y=y, bias=0x40000, y_f16=half)
        if half:
            base.update(alpha=0x50000, beta=0x60000)
        if i > 0:
            yield i, dict(base, x_f16=half)
            continue
        # the first layer in every input form the engine may give it: plain, one-pixel halo, padding-wide halo, NCHW planes,
        # and (fp16) the half NHWC4 haloed copy
        forms = [dict(base), dict(base, x_halo=1), dict(base, x_nchw=1)]
        if l["pad"] > 1:
            forms.append(dict(base, x_halo=l["pad"]))
        if half:
            forms.append(dict(base, x_f16=1, x_halo=1, ldx=4))
        for f in forms:
            yield i, f


def _row(lib, f, first):
    d = Conv(**f)
    names = [lib.y2h_conv_variant(C.byref(d), s) for s in (0, 1)]
    bm, bn, ks = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_int * 64)()
    nc = lib.y2h_conv_candidates(C.byref(d), bm, bn, ks, 64)
    cols = [" ".join(str(f.get(k, 0)) for k in KEY), " ".join(n.decode() if n else "-" for n in names),
            "mfma %d" % lib.y2h_conv_uses_mfma(C.byref(d)), "ws %d" % lib.y2h_conv_workspace_bytes(C.byref(d)),
            "cand " + (" ".join("%dx%d/%d" % (bm[k], bn[k], ks[k]) for k in range(nc)) or "-")]
    if first:
        cols.append("first %d %d %d stem %d" % (lib.y2h_conv_first_layer_ok(C.byref(d)), lib.y2h_conv_first_layer_f16_ok(C.byref(d)),
                                                lib.y2h_conv_first_layer_nchw_ok(C.byref(d)), lib.y2h_conv_stem_halo(C.byref(d))))
    return " | ".join(cols)


KEY = ("batch", "h", "w", "c", "ldx", "x_halo", "n", "size", "stride", "pad", "fuse_maxpool2", "batch_normalize", "activation",
       "x_f16", "y_f16", "x_nchw")

# forcing switches, set in-process between calls as the tile tests do; each applies to the FORCED configurations below
FORCED_ENV = [("Y2_CONV_TILE", "128x64"), ("Y2_CONV_TILE", "256x128"), ("Y2_CONV_KSPLIT", "2"), ("Y2_CONV_GRID", "64"),
              ("Y2_SKF", "0"), ("Y2_SKF_WGS", "200"), ("Y2_SK", "0"), ("Y2_SK_TILES", "4"), ("Y2_SK_WGS", "96"),
              ("Y2_TAIL", "0"), ("Y2_TAIL_TILE", "128x128"), ("Y2_TAIL_TILES", "8"), ("Y2_C32F_MIN_TILES", "1"),
              ("Y2_C64_MIN_TILES", "1"), ("Y2_NO_C32F", "1"), ("Y2_NO_C64", "1"), ("Y2_NO_M16", "1"), ("Y2_F16_NO_P8", "1"),
              ("Y2_NO_FIRST_NCHW", "1")]
FORCED = [("yolo", 608, 32), ("yolo", 416, 1), ("yolo9000", 544, 8), ("darknet19", 448, 128), ("tiny-yolo-voc", 416, 1)]
FORMS = [(0, ALIGNED, "f32"), (0, MISALIGNED, "f32 y+4"), (1, ALIGNED, "f16"), (1, MISALIGNED, "f16 y+4")]


def sweep(lib, rows):
    """For every zoo network (default size; 416 and 608 too for the full-size detectors) at batch 1, 8, 32 and 128, fp32 and fp16,
    with y 16-byte aligned and not, and for a few of them under each forcing switch: every conv layer's descriptor with
    y2h_conv_variant (strict 0 and 1), y2h_conv_uses_mfma, y2h_conv_workspace_bytes, the y2h_conv_candidates list and, for
    the first layer, the four first-layer / stem queries.  rows: print those lines; else one line per configuration with a
    digest of each form's lines (tests/golden/conv_plan_table.txt) -- where a digest moves, --sweep-rows of the two builds shows why."""
    import hashlib
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]

    def show(tag, cases):
        for net, size, batch in cases:
            name = "%s%s %d b%d" % (tag, net, size, batch)
            digests = []
            for half, y, form in FORMS:
                lines = [_row(lib, f, i == 0) for i, f in _descs(net, size, batch, half, y)]
                if rows:
                    print("\n".join("%s %s | %s" % (name, form, l) for l in lines))
                digests.append(hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12])
            if not rows:
                print("%s | %s" % (name, " ".join(digests)))

    if not rows:
        print("# configuration | digest of its layers' answers: " + ", ".join(f for _, _, f in FORMS))
    cases = []
    for net in zoo.SPECS:
        sizes = [zoo.DEFAULT_SIZE[net]]
        if sizes[0] >= 416 and any(l["type"] == "region" for l in zoo.resolve(net, sizes[0])):     # the full-size detectors
            sizes += [s for s in (416, 608) if s not in sizes]
        cases += [(net, s, b) for s in sizes for b in (1, 8, 32, 128)]
    show("", cases)
    for k, v in FORCED_ENV:
        os.environ[k] = v
        show("%s=%s " % (k, v), FORCED)
        del os.environ[k]


class Wino(C.Structure):          # include/y2_hip.h: y2h_wino
    _fields_ = [("eligible", C.c_int), ("take", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("tiles", C.c_long), ("tiles_pad", C.c_long),
                ("u_bytes", C.c_size_t), ("v_bytes", C.c_size_t), ("m_bytes", C.c_size_t),
                ("direct_cost", C.c_double), ("gemm_cost", C.c_double), ("wino_cost", C.c_double)]


def wino_plan(lib, f):
    """y2h_wino_plan for one descriptor (a dict of y2h_conv fields)"""
    d, w = Conv(**f), Wino()
    assert lib.y2h_wino_plan(C.byref(d), C.byref(w)) == 0
    return w


def wino_cases():
    """every zoo network at its default size (the full-size detectors at 416 and 608 too), batch 1, 8, 32 and 128"""
    for net in zoo.SPECS:
        sizes = [zoo.DEFAULT_SIZE[net]]
        if sizes[0] >= 416 and any(l["type"] == "region" for l in zoo.resolve(net, sizes[0])):
            sizes += [s for s in (416, 608) if s not in sizes]
        for s in sizes:
            for b in (1, 8, 32, 128):
                yield net, s, b


def wino_rows(lib):
    """The Winograd rule's answer (include/y2_wino_rule.h through y2h_wino_plan) for every 3x3 conv layer of every zoo
    network: tests/golden/wino_plan_table.txt.  Costs in thousands of CU cycles."""
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]
    yield "# net size batch layer | h w c n pool | fp32: eligible take tile tiles_pad direct gemm wino (kcycles) | fp16: eligible take"
    for net, size, batch in wino_cases():
        rows = {}
        for half in (0, 1):
            for i, f in _descs(net, size, batch, half, ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                rows.setdefault(i, (f, []))[1].append(wino_plan(lib, f))
        for i, (f, (w, wh)) in sorted(rows.items()):
            yield "%s %d b%d L%d | %d %d %d %d %d | %d %d %dx%d %d %.0f %.0f %.0f | %d %d" % (
                net, size, batch, i, f["h"], f["w"], f["c"], f["n"], f["fuse_maxpool2"], w.eligible, w.take, w.bm, w.bn, w.tiles_pad,
                w.direct_cost / 1e3, w.gemm_cost / 1e3, w.wino_cost / 1e3, wh.eligible, wh.take)


class Winos(C.Structure):         # include/y2_hip.h: y2h_winos
    _fields_ = [("eligible", C.c_int), ("take", C.c_int), ("form", C.c_int), ("patches", C.c_long), ("u_bytes", C.c_size_t)]


def winos_plan(lib, f):
    """y2h_winos_plan for one descriptor (a dict of y2h_conv fields)"""
    d, w = Conv(**f), Winos()
    assert lib.y2h_winos_plan(C.byref(d), C.byref(w)) == 0
    return w


def winos_rows(lib):
    """The stationary-Winograd rule's answer (include/y2_winos_rule.h through y2h_winos_plan) for every 3x3 conv layer of
    every zoo network: tests/golden/winos_plan_table.txt."""
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]
    yield "# net size batch layer | h w c n pool | fp32: eligible take form patches u_bytes | fp16: eligible take"
    for net, size, batch in wino_cases():
        rows = {}
        for half in (0, 1):
            for i, f in _descs(net, size, batch, half, ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                rows.setdefault(i, (f, []))[1].append(winos_plan(lib, f))
        for i, (f, (w, wh)) in sorted(rows.items()):
            yield "%s %d b%d L%d | %d %d %d %d %d | %d %d %d %d %d | %d %d" % (
                net, size, batch, i, f["h"], f["w"], f["c"], f["n"], f["fuse_maxpool2"], w.eligible, w.take, w.form, w.patches,
                w.u_bytes, wh.eligible, wh.take)


class WinoSplit(C.Structure):     # include/y2_hip.h: y2h_wino_split
    _fields_ = [("eligible", C.c_int), ("take", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("bk", C.c_int), ("tiles", C.c_long),
                ("tiles_pad", C.c_long), ("u_bytes", C.c_size_t), ("v_bytes", C.c_size_t), ("m_bytes", C.c_size_t),
                ("present_cost", C.c_double), ("gemm_cost", C.c_double), ("split_cost", C.c_double)]


def wino_split_plan(lib, f):
    """y2h_wino_split_plan for one descriptor (a dict of y2h_conv fields)"""
    d, w = Conv(**f), WinoSplit()
    assert lib.y2h_wino_split_plan(C.byref(d), C.byref(w)) == 0
    return w


def wino_split_rows(lib):
    """The split rule's answer (include/y2_split_rule.h through y2h_wino_split_plan) for every 3x3 conv layer of every zoo
    network: tests/golden/wino_split_plan_table.txt.  Costs in thousands of CU cycles."""
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]
    yield "# net size batch layer | h w c n pool | fp32: eligible take tile tiles_pad v_bytes u_bytes present gemm split (kcycles) | fp16: eligible take"
    for net, size, batch in wino_cases():
        rows = {}
        for half in (0, 1):
            for i, f in _descs(net, size, batch, half, ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                rows.setdefault(i, (f, []))[1].append(wino_split_plan(lib, f))
        for i, (f, (w, wh)) in sorted(rows.items()):
            yield "%s %d b%d L%d | %d %d %d %d %d | %d %d %dx%dx%d %d %d %d %.0f %.0f %.0f | %d %d" % (
                net, size, batch, i, f["h"], f["w"], f["c"], f["n"], f["fuse_maxpool2"], w.eligible, w.take, w.bm, w.bn, w.bk, w.tiles_pad,
                w.v_bytes, w.u_bytes, w.present_cost / 1e3, w.gemm_cost / 1e3, w.split_cost / 1e3, wh.eligible, wh.take)


class SplitD(C.Structure):        # include/y2_hip.h: y2h_splitd
    _fields_ = [("eligible", C.c_int), ("take", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("bk", C.c_int), ("tiles", C.c_long),
                ("u_bytes", C.c_size_t), ("lds_bytes", C.c_size_t),
                ("direct_cost", C.c_double), ("matrix_cost", C.c_double), ("byte_cost", C.c_double), ("splitd_cost", C.c_double)]


def splitd_plan(lib, f):
    """y2h_conv_splitd_plan for one descriptor (a dict of y2h_conv fields)"""
    d, w = Conv(**f), SplitD()
    assert lib.y2h_conv_splitd_plan(C.byref(d), C.byref(w)) == 0
    return w


def splitd_rows(lib):
    """The direct split rule's answer (include/y2_splitd_rule.h through y2h_conv_splitd_plan) for every 3x3 conv layer of every
    zoo network: tests/golden/splitd_plan_table.txt.  Costs in thousands of CU cycles.  The rule is asked after the three
    Winograd rules (y2_conv_layer_form): a layer one of them takes keeps that form whatever this table says."""
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]
    yield "# net size batch layer | h w c n pool | fp32: eligible take tile tiles lds u_bytes direct matrix bytes (kcycles) | fp16: eligible take"
    for net, size, batch in wino_cases():
        rows = {}
        for half in (0, 1):
            for i, f in _descs(net, size, batch, half, ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                rows.setdefault(i, (f, []))[1].append(splitd_plan(lib, f))
        for i, (f, (w, wh)) in sorted(rows.items()):
            yield "%s %d b%d L%d | %d %d %d %d %d | %d %d %dx%dx%d %d %d %d %.0f %.0f %.0f | %d %d" % (
                net, size, batch, i, f["h"], f["w"], f["c"], f["n"], f["fuse_maxpool2"], w.eligible, w.take, w.bm, w.bn, w.bk, w.tiles,
                w.lds_bytes, w.u_bytes, w.direct_cost / 1e3, w.matrix_cost / 1e3, w.byte_cost / 1e3, wh.eligible, wh.take)


FORM_NAMES = ("direct", "wino", "winox", "winos", "splitd")          # csrc/host/y2_internal.h: Y2_FORM_*


def conv_form(lib, f):
    """y2_conv_form_of (y2_plan.c) for one descriptor (a dict of y2h_conv fields): the form and, unless it is direct, the name"""
    d, name = Conv(**f), C.create_string_buffer(80)
    lib.y2_conv_form_of.argtypes = [C.POINTER(Conv), C.c_int, C.c_char_p, C.c_size_t]
    form = lib.y2_conv_form_of(C.byref(d), f.get("fuse_maxpool2", 0), name, len(name))
    return form, name.value.decode()


def layer_form(lib, f):
    """y2_conv_layer_form (y2_plan.c) for one descriptor: y2_conv_form_of, then the direct split rule among what it leaves direct"""
    d, name = Conv(**f), C.create_string_buffer(80)
    lib.y2_conv_layer_form.argtypes = [C.POINTER(Conv), C.c_int, C.c_char_p, C.c_size_t]
    form = lib.y2_conv_layer_form(C.byref(d), f.get("fuse_maxpool2", 0), name, len(name))
    return form, name.value.decode()


def form_rows(lib):
    """The form every 3x3 conv layer of every zoo network runs in, the four rules combined (y2_conv_layer_form).  For people:
    tests/test_conv_form_cpu.py derives what it expects from the three rule tables, not from this dump."""
    for k in [k for k in os.environ if k.startswith("Y2_")]:
        del os.environ[k]
    yield "# net size batch layer | h w c n pool | fp32: form name | fp16: form name"
    for net, size, batch in wino_cases():
        rows = {}
        for half in (0, 1):
            for i, f in _descs(net, size, batch, half, ALIGNED):
                if f["size"] != 3 or f.get("x_halo") or f.get("x_nchw"):
                    continue
                rows.setdefault(i, (f, []))[1].append(layer_form(lib, f))
        for i, (f, forms) in sorted(rows.items()):
            yield "%s %d b%d L%d | %d %d %d %d %d | %s" % (net, size, batch, i, f["h"], f["w"], f["c"], f["n"], f["fuse_maxpool2"],
                                                           " | ".join("%s %s" % (FORM_NAMES[k], n or "-") for k, n in forms))


def main():
    lib = C.CDLL(os.environ.get("Y2_LIB") or os.path.join(ROOT, "sr_object_detection_amd", "libsr_yolo2.so"))
    lib.y2h_conv_variant.restype = C.c_char_p
    lib.y2h_conv_variant.argtypes = [C.POINTER(Conv), C.c_int]
    lib.y2h_conv_workspace_bytes.restype = C.c_size_t
    args = sys.argv[1:]
    if args in (["--sweep"], ["--sweep-rows"]):
        return sweep(lib, args == ["--sweep-rows"])
    if args == ["--wino"]:
        return print("\n".join(wino_rows(lib)))
    if args == ["--winos"]:
        return print("\n".join(winos_rows(lib)))
    if args == ["--wino-split"]:
        return print("\n".join(wino_split_rows(lib)))
    if args == ["--splitd"]:
        return print("\n".join(splitd_rows(lib)))
    if args == ["--forms"]:
        return print("\n".join(form_rows(lib)))
    for k in range(0, len(args), 3):
        net, size, batch = args[k], int(args[k + 1]), int(args[k + 2])
        layers = zoo.resolve(net, size)
        print("%s %d b%d" % (net, size, batch))
        for i, l in enumerate(layers):
            if l["type"] != "convolutional" or l["c"] % 16:
                continue
            pool = i + 1 < len(layers) and layers[i + 1]["type"] == "maxpool" and layers[i + 1]["size"] == 2 and layers[i + 1]["stride"] == 2
            d = Conv(batch=batch, h=l["h"], w=l["w"], c=l["c"], ldx=l["c"], n=l["filters"], size=l["size"], stride=l["stride"],
                     pad=l["size"] // 2 if l["pad"] else 0, out_h=l["out_h"], out_w=l["out_w"], ldy=l["filters"],
                     fuse_maxpool2=1 if pool else 0, batch_normalize=l.get("batch_normalize", 0), activation=1,
                     x=0x10000, w_packed=0x20000, y=0x30000, bias=0x40000)
            name = lib.y2h_conv_variant(C.byref(d), 0).decode()
            ws = lib.y2h_conv_workspace_bytes(C.byref(d))
            print("  L%-2d %3dx%-3d c%-4d n%-5d k%d%s  %-34s ws %d" % (i, l["h"], l["w"], l["c"], l["filters"], l["size"],
                                                                  "+p" if pool else "  ", name, ws))


if __name__ == "__main__":
    main()
