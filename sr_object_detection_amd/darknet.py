"""Python mirror of the reference's C interface for the forward path, bound with
ctypes to libsr_yolo2.so (the C-ABI library built from csrc/).

The method names, argument meaning and results follow the reference functions
(src_yolo2/parser.h:5-11, network.h:83-127, region_layer.h:12, box.h:13-17,
test_detector.h:2) so that the parity tests read like calls into Darknet:

    net = Network.parse_network_cfg("yolo.cfg")
    net.load_weights("yolo.weights")
    net.set_batch_network(1)
    out = net.network_predict(x)                      # float32 [batch*outputs]
    boxes, probs = net.get_region_boxes(1, 1, thresh)
    probs = do_nms_sort(boxes, probs, nms)

There is no fallback: if the shared library is missing or no GPU is visible the
calls raise (the library itself has no CPU compute path).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Y2_LIB points at another build of the same library (A/B runs of kernel variants on one GPU box)
LIB_PATH = os.environ.get("Y2_LIB") or os.path.join(_HERE, "libsr_yolo2.so")


class Y2Error(RuntimeError):
    pass


class Tree(C.Structure):
    _fields_ = [("leaf", C.POINTER(C.c_int)), ("n", C.c_int), ("parent", C.POINTER(C.c_int)),
                ("group", C.POINTER(C.c_int)), ("name", C.POINTER(C.c_char_p)), ("groups", C.c_int),
                ("group_size", C.POINTER(C.c_int)), ("group_offset", C.POINTER(C.c_int))]


class Box(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float)]


class Image(C.Structure):
    _fields_ = [("h", C.c_int), ("w", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


class Object(C.Structure):   # utils.h:14-28
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float), ("name", C.c_char * 20),
                ("prob", C.c_float), ("objClass", C.c_int), ("CameraX", C.c_float), ("CameraY", C.c_float),
                ("CameraZ", C.c_float), ("CameraWidth", C.c_float), ("CameraHeight", C.c_float),
                ("flagBelong2Person", C.c_ubyte), ("boxRGB", C.c_float * 3), ("bodyId", C.c_int)]


class KcfBox(C.Structure):          # include/sr_yolo2.h y2_kcf_box
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("w", C.c_double), ("h", C.c_double)]


class KcfGeometry(C.Structure):     # include/sr_yolo2.h y2_kcf_geometry
    _fields_ = [("resized", C.c_int), ("win_w", C.c_int), ("win_h", C.c_int), ("cells_w", C.c_int), ("cells_h", C.c_int),
                ("cx", C.c_double), ("cy", C.c_double), ("w", C.c_double), ("h", C.c_double), ("output_sigma", C.c_double)]


KCF_PATCH, KCF_FEATURES, KCF_XF, KCF_ALPHAF, KCF_RESPONSE = range(5)
KCF_MAX_TRACKERS, KCF_MAX_CELLS, KCF_CHANNELS = 32, 256, 31


def kcf_plan(box) -> dict:
    """y2_kcf_plan: init's arithmetic of one (cx, cy, w, h) box in pixels -> dict of y2_kcf_geometry's fields"""
    b, g = KcfBox(*[float(v) for v in box]), KcfGeometry()
    if lib().y2_kcf_plan(C.byref(b), C.byref(g)) != 0:
        raise Y2Error(_check())
    return {k: getattr(g, k) for k, _ in KcfGeometry._fields_}


def _kcf_frame(frame):
    """uint8 [h][w] or [h][w][c]; a view with padded rows is passed with its step -> (array kept alive, h, w, c, step)"""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim not in (2, 3):
        raise ValueError("a frame is uint8 [h][w] or [h][w][c]")
    c = 1 if f.ndim == 2 else f.shape[2]
    inner_ok = f.strides[-1] == 1 and (f.ndim == 2 or f.strides[1] == c)
    if not inner_ok or f.strides[0] < f.shape[1] * c:
        f = np.ascontiguousarray(f)
    return f, f.shape[0], f.shape[1], c, f.strides[0]


class Layer(C.Structure):    # include/sr_yolo2.h struct layer
    pass


Layer._fields_ = [
        ("type", C.c_int), ("activation", C.c_int), ("cost_type", C.c_int),
        ("batch_normalize", C.c_int), ("batch", C.c_int), ("flipped", C.c_int),
        ("inputs", C.c_int), ("outputs", C.c_int),
        ("h", C.c_int), ("w", C.c_int), ("c", C.c_int),
        ("out_h", C.c_int), ("out_w", C.c_int), ("out_c", C.c_int),
        ("n", C.c_int), ("groups", C.c_int),
        ("size", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("reverse", C.c_int), ("index", C.c_int), ("binary", C.c_int), ("xnor", C.c_int),
        ("softmax", C.c_int), ("classes", C.c_int), ("coords", C.c_int), ("classfix", C.c_int), ("log", C.c_int),
        ("sqrt", C.c_int), ("max_boxes", C.c_int), ("rescore", C.c_int), ("bias_match", C.c_int), ("random", C.c_int),
        ("absolute", C.c_int), ("truths", C.c_int),
        ("jitter", C.c_float), ("thresh", C.c_float), ("coord_scale", C.c_float), ("object_scale", C.c_float),
        ("noobject_scale", C.c_float), ("class_scale", C.c_float),
        ("temperature", C.c_float), ("scale", C.c_float),
        ("dontload", C.c_int), ("dontloadscales", C.c_int),
        ("softmax_tree", C.POINTER(Tree)), ("map", C.POINTER(C.c_int)),
        ("input_layers", C.POINTER(C.c_int)), ("input_sizes", C.POINTER(C.c_int)),
        ("biases", C.POINTER(C.c_float)), ("scales", C.POINTER(C.c_float)), ("weights", C.POINTER(C.c_float)),
        ("rolling_mean", C.POINTER(C.c_float)), ("rolling_variance", C.POINTER(C.c_float)),
        ("output", C.POINTER(C.c_float)), ("delta", C.POINTER(C.c_float)), ("cost", C.POINTER(C.c_float)),
        ("workspace_size", C.c_size_t), ("dev", C.c_void_p),
        ("side", C.c_int), ("forced", C.c_int), ("probability", C.c_float),
        ("flip", C.c_int), ("noadjust", C.c_int), ("angle", C.c_float), ("saturation", C.c_float),
        ("exposure", C.c_float), ("shift", C.c_float),
        ("steps", C.c_int), ("hidden", C.c_int), ("shortcut", C.c_int),
        ("input_layer", C.POINTER(Layer)), ("self_layer", C.POINTER(Layer)), ("output_layer", C.POINTER(Layer)),
        ("input_z_layer", C.POINTER(Layer)), ("state_z_layer", C.POINTER(Layer)), ("input_r_layer", C.POINTER(Layer)),
        ("state_r_layer", C.POINTER(Layer)), ("input_h_layer", C.POINTER(Layer)), ("state_h_layer", C.POINTER(Layer)),
        ("alpha", C.c_float), ("beta", C.c_float), ("kappa", C.c_float),
    ]


class CNetwork(C.Structure):  # include/sr_yolo2.h struct network
    _fields_ = [
        ("workspace", C.POINTER(C.c_float)), ("n", C.c_int), ("batch", C.c_int), ("seen", C.POINTER(C.c_int)),
        ("subdivisions", C.c_int), ("learning_rate", C.c_float), ("momentum", C.c_float), ("decay", C.c_float),
        ("max_batches", C.c_int), ("time_steps", C.c_int), ("layers", C.POINTER(Layer)), ("outputs", C.c_int),
        ("output", C.POINTER(C.c_float)), ("inputs", C.c_int), ("h", C.c_int), ("w", C.c_int), ("c", C.c_int),
        ("gpu_index", C.c_int), ("hierarchy", C.POINTER(Tree)), ("engine", C.c_void_p),
    ]


class Recall(C.Structure):   # include/sr_yolo2.h y2_recall
    _fields_ = [("total", C.c_int), ("correct", C.c_int), ("proposals", C.c_int), ("avg_iou", C.c_float)]


class Det(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float), ("prob", C.c_float),
                ("obj_id", C.c_int)]


class Region(C.Structure):   # include/sr_yolo2.h y2_region
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("c", C.c_int), ("step", C.c_int),
                ("x", C.c_int), ("y", C.c_int), ("rw", C.c_int), ("rh", C.c_int)]


class DepthFrame(C.Structure):   # include/sr_yolo2.h y2_depth_frame
    _fields_ = [("depth", C.c_void_p), ("body", C.c_void_p), ("map", C.c_void_p), ("dh", C.c_int), ("dw", C.c_int),
                ("H", C.c_int), ("W", C.c_int)]


class Det3d(C.Structure):        # include/sr_yolo2.h y2_det3d
    _fields_ = [("valid", C.c_int), ("left", C.c_int), ("top", C.c_int), ("right", C.c_int), ("bot", C.c_int),
                ("otsu", C.c_int), ("mean_all_mm", C.c_int), ("avg_mm", C.c_float), ("body_id", C.c_int),
                ("belongs", C.c_int), ("cam_x", C.c_float), ("cam_y", C.c_float), ("cam_z", C.c_float),
                ("cam_w", C.c_float), ("cam_h", C.c_float), ("pts", (C.c_float * 2) * 5)]


class PlaneOpts(C.Structure):    # include/sr_yolo2.h y2_plane_opts
    _fields_ = [("far_m", C.c_float), ("dist_m", C.c_float), ("iters", C.c_int), ("seed", C.c_uint), ("samples", C.c_void_p)]


class Plane(C.Structure):        # include/sr_yolo2.h y2_plane
    _fields_ = [("found", C.c_int), ("best", C.c_int), ("valid_points", C.c_int), ("best_count", C.c_int),
                ("removed", C.c_int), ("a", C.c_double), ("b", C.c_double), ("c", C.c_double), ("d", C.c_double)]


EVENT_DEMO_WHAT, EVENT_GRASP = 0, 1                         # include/sr_yolo2.h Y2_EVENT_*


class View(C.Structure):     # include/y2_hip.h y2h_view: one view of y2h_views_to_input
    _fields_ = [("src", C.c_longlong), ("sw", C.c_int), ("sh", C.c_int), ("dx", C.c_int), ("dy", C.c_int),
                ("flip", C.c_int), ("pad_", C.c_int)]


VIEWS_CROP10, VIEWS_MULTI, VIEWS_FULL = 0, 1, 2             # include/sr_yolo2.h Y2_VIEWS_*


TRAIN_PRECISIONS = ("fp32", "bf16x3", "bf16")      # include/sr_yolo2.h Y2_TRAIN_FP32 / Y2_TRAIN_BF16X3 / Y2_TRAIN_BF16


class TrainConv(C.Structure):  # include/y2_hip.h y2h_train_conv: the shape of one trainable convolution
    _fields_ = [(k, C.c_int) for k in ("batch", "h", "w", "c", "n", "size", "pad", "out_h", "out_w")]


class TrainDense(C.Structure):  # include/y2_hip.h y2h_train_dense: the shape of one trainable [connected] layer
    _fields_ = [(k, C.c_int) for k in ("batch", "inputs", "outputs")]


class TrainRegion(C.Structure):  # include/y2_hip.h y2h_train_region: one [region] head in training mode
    _fields_ = [(k, C.c_int) for k in ("batch", "h", "w", "n", "classes", "bias_match", "rescore")] + \
               [(k, C.c_float) for k in ("thresh", "coord_scale", "object_scale", "noobject_scale", "class_scale")]


class TrainDetection(C.Structure):  # include/y2_hip.h y2h_train_detection: one [detection] head in training mode (coords = 4)
    _fields_ = [(k, C.c_int) for k in ("batch", "side", "n", "classes", "softmax", "sqrt", "rescore", "forced")] + \
               [(k, C.c_float) for k in ("coord_scale", "object_scale", "noobject_scale", "class_scale")]


class DetectionStats(C.Structure):  # include/sr_yolo2.h y2_detection_stats == include/y2_hip.h y2h_train_detection_stats
    _fields_ = [(k, C.c_float) for k in ("avg_iou", "avg_cat", "avg_allcat", "avg_obj", "avg_anyobj")] + [("count", C.c_int)]


class RegionStats(C.Structure):  # include/sr_yolo2.h y2_region_stats == include/y2_hip.h y2h_train_region_stats
    _fields_ = [(k, C.c_float) for k in ("avg_iou", "avg_class", "avg_obj", "avg_noobj", "recall")] + \
               [("count", C.c_int), ("class_count", C.c_int)]


class DreamDraws(C.Structure):    # include/sr_yolo2.h y2_dream_draws: the five rand() calls of one run_nightmare iteration
    _fields_ = [("layer_offset", C.c_int), ("octave", C.c_int), ("dx", C.c_int), ("dy", C.c_int), ("flip", C.c_int)]


class DreamCounters(C.Structure):  # include/sr_yolo2.h y2_dream_counters
    _fields_ = [("selected", C.c_int), ("h2d_bytes", C.c_ulonglong), ("d2h_bytes", C.c_ulonglong), ("allocations", C.c_ulong),
                ("steps", C.c_ulong)]


class DreamResample(C.Structure):  # include/y2_hip.h y2h_dream_resample: crop -> resize -> crop with flips and layouts
    _fields_ = [(k, C.c_int) for k in ("c", "sh", "sw", "src_nhwc", "src_flip", "cx", "cy", "ch", "cw", "oh", "ow", "px", "py",
                                       "dst_nhwc", "dst_flip")]


class AugItem(C.Structure):  # include/sr_yolo2.h y2_aug_item: one image of y2_train_load_detection
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("c", C.c_int), ("step", C.c_int),
                ("pleft", C.c_int), ("ptop", C.c_int), ("swidth", C.c_int), ("sheight", C.c_int), ("flip", C.c_int),
                ("dhue", C.c_float), ("dsat", C.c_float), ("dexp", C.c_float),
                ("boxes", C.c_void_p), ("nboxes", C.c_int), ("swaps", C.c_void_p)]


class Aug(C.Structure):      # include/y2_hip.h y2h_aug: one item of y2h_augment_to_input
    _fields_ = [("src", C.c_longlong), ("pitch", C.c_int), ("c", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("rw", C.c_int),
                ("rh", C.c_int), ("ow", C.c_int), ("oh", C.c_int), ("pleft", C.c_int), ("ptop", C.c_int), ("swidth", C.c_int),
                ("sheight", C.c_int), ("flip", C.c_int), ("dhue", C.c_float), ("dsat", C.c_float), ("dexp", C.c_float),
                ("w_scale", C.c_float), ("h_scale", C.c_float)]


class AugClsItem(C.Structure):  # include/sr_yolo2.h y2_aug_cls_item: one image of y2_train_load_classification
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("c", C.c_int), ("step", C.c_int),
                ("aspect", C.c_float), ("scale", C.c_float), ("rad", C.c_float), ("dx", C.c_float), ("dy", C.c_float),
                ("flip", C.c_int), ("dhue", C.c_float), ("dsat", C.c_float), ("dexp", C.c_float)]


class AugCls(C.Structure):   # include/y2_hip.h y2h_aug_cls: one item of y2h_augment_cls_to_input
    _fields_ = [("src", C.c_longlong)] + [(k, C.c_double) for k in ("cosr", "sinr", "s", "aspect", "ax", "ay")] + \
               [("cx", C.c_float), ("cy", C.c_float)] + \
               [(k, C.c_int) for k in ("pitch", "c", "x0", "y0", "rw", "rh", "ow", "oh", "flip")] + \
               [("dhue", C.c_float), ("dsat", C.c_float), ("dexp", C.c_float)]


class RecArgs(C.Structure):  # include/y2_hip.h y2h_rec_args: one launch of y2h_rec_step
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("mean", C.c_void_p), ("scale", C.c_void_p),
                ("rinv", C.c_void_p), ("bn", C.c_int), ("act", C.c_int), ("pre", C.c_void_p), ("rows", C.c_int), ("k", C.c_int),
                ("n", C.c_int), ("h", C.c_int), ("mode", C.c_int), ("shortcut", C.c_int), ("proj", C.c_void_p),
                ("state", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p), ("z", C.c_void_p), ("xcopy", C.c_void_p)]


REC_DENSE, REC_RNN, REC_GRU_ZR, REC_GRU_H = 0, 1, 2, 3      # y2h_rec_args.mode
REC_REF, REC_SKINNY = 0, 1                                  # y2h_rec_step's form
REC_SKINNY_MAX_ROWS = 8
Y2H_EINVAL = -2

DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("prob", "<f4"), ("obj_id", "<i4")])

DET3D_DTYPE = np.dtype([("valid", "<i4"), ("left", "<i4"), ("top", "<i4"), ("right", "<i4"), ("bot", "<i4"), ("otsu", "<i4"),
                        ("mean_all_mm", "<i4"), ("avg_mm", "<f4"), ("body_id", "<i4"), ("belongs", "<i4"), ("cam_x", "<f4"),
                        ("cam_y", "<f4"), ("cam_z", "<f4"), ("cam_w", "<f4"), ("cam_h", "<f4"), ("pts", "<f4", (5, 2))])

LAYER_TYPES = ["CONVOLUTIONAL", "DECONVOLUTIONAL", "CONNECTED", "MAXPOOL", "SOFTMAX", "DETECTION", "DROPOUT", "CROP",
               "ROUTE", "COST", "NORMALIZATION", "AVGPOOL", "LOCAL", "SHORTCUT", "ACTIVE", "RNN", "GRU", "CRNN",
               "BATCHNORM", "NETWORK", "XNOR", "REGION", "REORG", "BLANK"]

_lib = None


def lib():
    """Load libsr_yolo2.so; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Y2Error("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(make -C sr_object_detection_amd/csrc). There is no Python/CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    L.y2_set_error_mode.argtypes = [C.c_int]
    L.y2_set_error_mode(1)          # report errors as return values; this binding raises Y2Error
    L.y2_last_error.restype = C.c_char_p
    L.parse_network_cfg.restype = CNetwork
    L.parse_network_cfg.argtypes = [C.c_char_p]
    L.load_weights.argtypes = [C.POINTER(CNetwork), C.c_char_p]
    L.load_weights_upto.argtypes = [C.POINTER(CNetwork), C.c_char_p, C.c_int]
    L.save_weights.argtypes = [CNetwork, C.c_char_p]
    L.y2_denormalize_network.argtypes = [C.POINTER(CNetwork)]
    L.set_batch_network.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.resize_network.argtypes = [C.POINTER(CNetwork), C.c_int, C.c_int]
    L.free_network.argtypes = [CNetwork]
    L.network_predict.restype = C.POINTER(C.c_float)
    L.network_predict.argtypes = [CNetwork, C.c_void_p]
    L.get_network_output.restype = C.POINTER(C.c_float)
    L.get_network_output.argtypes = [CNetwork]
    L.get_network_output_size.argtypes = [CNetwork]
    L.reset_rnn_state.argtypes = [CNetwork, C.c_int]
    L.get_network_input_size.argtypes = [CNetwork]
    L.get_region_boxes.argtypes = [Layer, C.c_int, C.c_int, C.c_float, C.POINTER(C.POINTER(C.c_float)),
                                   C.c_void_p, C.c_int, C.c_void_p]
    L.do_nms_sort.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.c_int, C.c_int, C.c_float]
    L.do_nms.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.c_int, C.c_int, C.c_float]
    L.box_iou.restype = C.c_float
    L.box_iou.argtypes = [Box, Box]
    L.test_detector_img.argtypes = [C.POINTER(C.c_char_p), C.c_void_p, CNetwork, Image, C.c_float,
                                    C.POINTER(Object), C.POINTER(C.c_int)]
    L.resize_image.restype = Image
    L.resize_image.argtypes = [Image, C.c_int, C.c_int]
    L.free_image.argtypes = [Image]
    L.print_detector_detections.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_void_p, C.POINTER(C.POINTER(C.c_float)),
                                            C.c_int, C.c_int, C.c_int, C.c_int]
    L.print_imagenet_detections.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.POINTER(C.c_float)),
                                            C.c_int, C.c_int, C.c_int, C.c_int]
    L.print_cocos.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.POINTER(C.c_float)),
                              C.c_int, C.c_int, C.c_int, C.c_int]
    L.get_coco_image_id.argtypes = [C.c_char_p]
    L.basecfg.restype = C.c_void_p
    L.basecfg.argtypes = [C.c_char_p]
    L.y2_validate_detector_frames.argtypes = [CNetwork, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p,
                                              C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_void_p]
    L.y2_validate_recall_frames.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Recall)]
    L.letterbox_image.restype = Image
    L.letterbox_image.argtypes = [Image, C.c_int, C.c_int]
    L.letterbox_image_into.argtypes = [Image, C.c_int, C.c_int, Image]
    L.y2_ingest_u8.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.y2_detect_u8.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.y2_ingest_regions.argtypes = [CNetwork, C.POINTER(Region), C.c_int, C.c_int, C.c_int]
    L.y2_detect_regions.argtypes = [CNetwork, C.POINTER(Region), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_int]
    L.y2_region_box_to_frame.argtypes = [C.POINTER(Region), C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 4
    L.test_detector_regions.argtypes = [C.POINTER(C.c_char_p), CNetwork, C.POINTER(Region), C.c_int, C.c_float,
                                        C.POINTER(C.POINTER(Object)), C.POINTER(C.c_int)]
    L.y2_depth_upload.argtypes = [CNetwork, C.POINTER(DepthFrame)]
    L.y2_depth_set_camera_table.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int]
    L.y2_depth_aligned.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2_otsu_threshold.argtypes = [C.c_void_p]
    L.y2_depth_roi.argtypes = [Box, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4
    L.y2_depth_boxes.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_void_p]
    L.y2_ingest_regions_depth.argtypes = [CNetwork, C.POINTER(Region), C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.y2_detect_regions_depth.argtypes = [CNetwork, C.POINTER(Region), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.test_detector_regions_depth.argtypes = [C.POINTER(C.c_char_p), CNetwork, C.POINTER(Region), C.c_int, C.c_void_p,
                                              C.c_float, C.POINTER(C.c_void_p), C.c_void_p]
    L.y2_depth_set_plane_removal.argtypes = [CNetwork, C.POINTER(PlaneOpts)]
    L.y2_depth_plane.argtypes = [CNetwork, C.POINTER(Plane)]
    L.y2_depth_grasp_aligned.argtypes = [CNetwork, C.c_void_p, C.c_void_p]
    L.y2_depth_set_event.argtypes = [CNetwork, C.c_int]
    L.y2_depth_set_grasp_filter.argtypes = [CNetwork, C.c_int]
    L.y2_plane_samples.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint, C.c_void_p]
    L.y2_plane_from_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_connected_f16_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                         C.c_void_p, C.c_int]
    L.y2_plane_fit.argtypes = [C.c_void_p, C.c_void_p]
    L.test_detector_img_for_grasping.argtypes = [C.POINTER(C.c_char_p), C.c_void_p, CNetwork, Image, Image, C.c_float,
                                                 C.POINTER(Object), C.POINTER(C.c_int)]
    L.y2h_u8_to_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p]
    L.top_predictions.argtypes = [CNetwork, C.c_int, C.c_void_p]
    L.cuda_set_device.argtypes = [C.c_int]
    L.y2_prepare.argtypes = [C.POINTER(CNetwork)]
    L.y2_set_strict.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_half.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_fusion.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_autotune.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_detect_overlap.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_graph.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_set_timing.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_layer_times_ms.argtypes = [CNetwork, C.c_void_p, C.c_int]
    L.y2_layer_kernel.restype = C.c_char_p
    L.y2_layer_kernel.argtypes = [CNetwork, C.c_int]
    L.y2_weights_arena.argtypes = [C.POINTER(CNetwork), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.y2_weights_resident.argtypes = [C.POINTER(CNetwork)]
    L.y2_feed_open.argtypes = [C.POINTER(CNetwork), C.c_int, C.c_size_t]
    L.y2_feed_close.argtypes = [C.POINTER(CNetwork)]
    L.y2_feed_host.restype = C.c_void_p
    L.y2_feed_host.argtypes = [CNetwork, C.c_int]
    L.y2_feed_device.restype = C.c_void_p
    L.y2_feed_device.argtypes = [CNetwork, C.c_int]
    L.y2_feed_slot_bytes.restype = C.c_size_t
    L.y2_feed_slot_bytes.argtypes = [CNetwork]
    L.y2_feed_submit.argtypes = [CNetwork, C.c_int, C.c_size_t]
    L.y2_feed_wait_host.argtypes = [CNetwork, C.c_int]
    L.y2_feed_forward.argtypes = [CNetwork, C.c_int]
    L.y2_feed_forward_u8.argtypes = [CNetwork, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.y2_comm_library.restype = C.c_char_p
    L.y2_comm_unique_id.argtypes = [C.c_void_p]
    L.y2_comm_init_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.y2_comm_destroy.argtypes = [C.c_void_p]
    L.y2_broadcast_weights.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_int]
    L.y2_comm_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.y2_detector_create.restype = C.c_void_p
    L.y2_detector_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.y2_detector_destroy.argtypes = [C.c_void_p]
    L.y2_detector_net_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.y2_detector_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int,
                                     C.c_void_p, C.c_int]
    L.y2_weights_layout.argtypes = [C.POINTER(CNetwork), C.POINTER(C.c_ulonglong), C.POINTER(C.c_size_t)]
    L.y2_network_predict_device.restype = C.POINTER(C.c_float)
    L.y2_network_predict_device.argtypes = [CNetwork, C.c_void_p]
    L.y2_forward_device.argtypes = [CNetwork, C.c_void_p]
    L.y2_detect_resident.argtypes = [CNetwork, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.y2_detect.argtypes = [CNetwork, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.y2_pull_layer_output.argtypes = [CNetwork, C.c_int, C.c_void_p]
    L.y2_stream.restype = C.c_void_p
    L.y2_stream.argtypes = [CNetwork]
    L.y2_sync.argtypes = [CNetwork]
    for name in ("y2h_event_create", "y2h_event_destroy"):
        pass
    L.y2h_event_create.argtypes = [C.POINTER(C.c_void_p)]
    L.y2h_event_destroy.argtypes = [C.c_void_p]
    L.y2h_event_record.argtypes = [C.c_void_p, C.c_void_p]
    L.y2h_event_elapsed_ms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.y2h_device_count.restype = C.c_int
    L.y2h_device_name.restype = C.c_char_p
    L.y2h_clock_probe.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_void_p]
    L.y2h_device_pci_bus_id.restype = C.c_char_p
    L.y2h_device_pci_bus_id.argtypes = [C.c_int]
    L.y2h_last_error.restype = C.c_char_p
    L.y2h_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.y2h_free.argtypes = [C.c_void_p]
    L.y2h_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.y2h_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.y2h_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.y2h_stream_sync.argtypes = [C.c_void_p]
    L.y2h_set_device.argtypes = [C.c_int]
    L.y2h_rec_skinny_ok.argtypes = [C.c_int, C.c_int]
    L.y2h_rec_step.argtypes = [C.POINTER(RecArgs), C.c_int, C.c_void_p]
    L.y2h_rnn_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.y2h_views_to_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_accumulate_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.y2h_lrn_fast_ok.argtypes = [C.c_int, C.c_int]
    L.y2h_lrn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                          C.c_int, C.c_void_p]
    L.y2h_lrn_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                              C.c_void_p]
    L.y2h_activate_array.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.y2h_activate_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.y2h_activate_copy_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "y2h_wino_split_plan"):          # (an older build under Y2_LIB has no split form)
        L.y2h_wino_split_plan.argtypes = [C.c_void_p, C.c_void_p]        # (y2h_conv *, y2h_wino_split *): tools/plan_dump.py has the structs
        L.y2h_wino_split_workspace_bytes.restype = C.c_size_t
        L.y2h_wino_split_launches.restype = C.c_ulong
    if hasattr(L, "y2h_conv_splitd_plan"):         # (an older build under Y2_LIB has no direct split form)
        L.y2h_conv_splitd_plan.argtypes = [C.c_void_p, C.c_void_p]       # (y2h_conv *, y2h_splitd *)
        L.y2h_conv_splitd_launches.restype = C.c_ulong
    L.y2h_d2h_copies.restype = C.c_ulong
    L.y2h_stream_syncs.restype = C.c_ulong
    L.y2_set_view_block_bytes.argtypes = [C.c_size_t]
    L.y2_view_resizes.restype = C.c_ulong
    L.y2_classifier_view_sums.argtypes = [C.POINTER(CNetwork), C.c_int, C.POINTER(Image), C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.y2_validate_classifier_10_frames.argtypes = [CNetwork, C.POINTER(Image), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.y2_validate_classifier_multi_frames.argtypes = [C.POINTER(CNetwork), C.POINTER(Image), C.c_int, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.y2_validate_classifier_full_frames.argtypes = [C.POINTER(CNetwork), C.POINTER(Image), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                     C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.y2_classify_frames.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2_hierarchy_enqueue.argtypes = [CNetwork, C.c_int]
    L.read_tree.restype = C.POINTER(Tree)
    L.read_tree.argtypes = [C.c_char_p]
    L.hierarchy_predictions.restype = None
    L.hierarchy_predictions.argtypes = [C.c_void_p, C.c_int, C.POINTER(Tree), C.c_int]
    L.get_hierarchy_probability.restype = C.c_float
    L.get_hierarchy_probability.argtypes = [C.c_void_p, C.POINTER(Tree), C.c_int]
    L.change_leaves.restype = None
    L.change_leaves.argtypes = [C.POINTER(Tree), C.c_char_p]
    L.y2h_softmax_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_void_p]
    L.y2h_softmax_tree_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.y2h_hierarchy_rows.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_p8_stream_k_plan.argtypes = [C.c_long, C.c_int, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "y2h_sk_shares"):     # (an A/B library with an older revision's conv kernels, tools/build_variant.sh --src-rev, has none)
        L.y2h_sk_shares.argtypes = [C.c_long, C.c_int, C.c_long, C.POINTER(C.c_int)]
        L.y2h_sk_first.argtypes = [C.c_long, C.c_int, C.c_long, C.POINTER(C.c_int)]
        L.y2h_sk_walk.argtypes = [C.c_long, C.c_int, C.c_long, C.POINTER(C.c_int), C.c_int]
    L.train_network_datum.restype = C.c_float
    L.train_network_datum.argtypes = [CNetwork, C.c_void_p, C.c_void_p]
    L.get_current_rate.restype = C.c_float
    L.get_current_rate.argtypes = [CNetwork]
    L.get_current_batch.argtypes = [CNetwork]
    L.get_network_cost.restype = C.c_float
    L.get_network_cost.argtypes = [CNetwork]
    L.y2_train_prepare.argtypes = [C.POINTER(CNetwork)]
    L.y2_train_step.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.y2_train_step_device.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.y2_train_sync.argtypes = [C.POINTER(CNetwork)]
    L.y2_train_pull.argtypes = [C.POINTER(CNetwork), C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.y2_train_free.restype = None
    L.y2_train_free.argtypes = [C.POINTER(CNetwork)]
    L.y2_train_pack_weights.restype = None
    L.y2_train_pack_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.y2_train_unpack_weights.restype = None
    L.y2_train_unpack_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for f in (L.y2_train_pack_dense_weights, L.y2_train_unpack_dense_weights):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.y2h_train_dense_plan.argtypes = [C.POINTER(TrainDense), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                       C.c_void_p, C.c_int]
    L.y2h_train_dense_forward.argtypes = [C.POINTER(TrainDense), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.y2h_train_dense_dinput.argtypes = [C.POINTER(TrainDense), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p]
    L.y2h_train_dense_dweight.argtypes = [C.POINTER(TrainDense), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_train_conv_forward.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_train_conv_dinput.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_train_dweight_splits.argtypes = [C.POINTER(TrainConv)]
    L.y2h_train_dweight_ws_bytes.restype = C.c_size_t
    L.y2h_train_dweight_ws_bytes.argtypes = [C.POINTER(TrainConv)]
    L.y2h_train_conv_dweight.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_train_conv_forward_bf16.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.y2h_train_conv_dinput_bf16.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.y2h_train_conv_dweight_bf16.argtypes = [C.POINTER(TrainConv), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.y2_train_set_precision.argtypes = [C.POINTER(CNetwork), C.c_int]
    L.y2_train_precision.argtypes = [C.POINTER(CNetwork)]
    L.y2h_train_reduce_scratch_bytes.restype = C.c_size_t
    L.y2h_train_reduce_scratch_bytes.argtypes = [C.c_long, C.c_int]
    L.y2h_train_bn_stats.argtypes = [C.c_void_p, C.c_long, C.c_int] + [C.c_void_p] * 6
    L.y2h_train_bn_stats_rate.argtypes = [C.c_void_p, C.c_long, C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.y2h_train_dropout.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.y2h_train_bias_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int] + [C.c_void_p] * 4
    L.y2h_train_bn_deltas.argtypes = [C.c_void_p] * 5 + [C.c_long, C.c_int] + [C.c_void_p] * 4
    L.y2h_train_bn_backward.argtypes = [C.c_void_p] * 7 + [C.c_long, C.c_int, C.c_void_p]
    L.y2h_train_bn_apply.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_long, C.c_int, C.c_void_p]
    L.y2h_train_act_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p]
    L.y2h_train_maxpool_forward.argtypes = [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_void_p]
    L.y2h_train_maxpool_backward.argtypes = [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_void_p]
    L.y2h_train_avgpool_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.y2h_train_avgpool_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.y2h_train_softmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    L.y2h_train_cost_sse.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_long, C.c_void_p, C.c_void_p]
    L.y2h_train_sgd.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_void_p]
    # y2_train_rnn.hip: tensors [T][B][C]
    L.y2h_train_rnn_bn_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_void_p]
    L.y2h_train_rnn_bn_apply.argtypes = [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p]
    L.y2h_train_rnn_step_finish.argtypes = [C.c_void_p] * 7 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    L.y2h_train_cost_sse_chunked.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_long] + [C.c_void_p] * 3
    L.y2h_train_rnn_fused_fits.argtypes = [C.c_int, C.c_int]
    L.y2h_train_rnn_fused_ws_bytes.argtypes = [C.c_int, C.c_int]
    L.y2h_train_rnn_fused_ws_bytes.restype = C.c_size_t
    L.y2h_train_rnn_fused_forward.argtypes = [C.c_void_p] * 9 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    L.y2h_train_rnn_fused_backward.argtypes = [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p] * 8
    L.y2h_train_rnn_delta.argtypes = [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p] * 5
    L.y2h_train_rnn_sum_steps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_train_rnn_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.y2h_train_rnn_add_transposed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.y2h_train_rnn_onehot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2_train_region_stats.argtypes = [C.POINTER(CNetwork), C.c_int, C.POINTER(RegionStats)]
    L.y2_train_truth_floats.argtypes = [C.POINTER(CNetwork)]
    L.y2_train_detection_stats.argtypes = [C.POINTER(CNetwork), C.c_int, C.POINTER(DetectionStats)]
    L.y2h_train_detection_scratch_bytes.restype = C.c_size_t
    L.y2h_train_detection_scratch_bytes.argtypes = [C.POINTER(TrainDetection)]
    L.y2h_train_detection_loss.argtypes = [C.POINTER(TrainDetection)] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4
    L.y2h_train_region_scratch_bytes.restype = C.c_size_t
    L.y2h_train_region_scratch_bytes.argtypes = [C.POINTER(TrainRegion)]
    L.y2h_train_region_loss.argtypes = [C.POINTER(TrainRegion), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    L.y2h_train_route_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p]
    L.y2h_train_route_backward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]
    L.y2h_train_add.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.y2h_train_reorg_backward.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.y2_aug_draw_detection.restype = None
    L.y2_aug_draw_detection.argtypes = [C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int, C.POINTER(AugItem), C.c_void_p]
    L.y2_aug_random_paths.restype = None
    L.y2_aug_random_paths.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.y2_aug_truth_detection.argtypes = [C.POINTER(AugItem), C.c_int, C.c_void_p]
    L.y2_net_augment.argtypes = [CNetwork] + [C.POINTER(C.c_float)] * 4 + [C.POINTER(C.c_int)]
    L.y2_train_load_detection.argtypes = [C.POINTER(CNetwork), C.POINTER(AugItem), C.c_int, C.c_int]
    L.y2_train_step_loaded.argtypes = [C.POINTER(CNetwork), C.POINTER(C.c_float)]
    L.y2_get_rnn_data.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2_train_load_rnn_data.argtypes = [C.POINTER(CNetwork), C.c_char_p, C.c_size_t, C.c_void_p]
    L.y2_train_pull_input.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_void_p]
    L.y2_train_load_times.argtypes = [C.POINTER(CNetwork), C.c_void_p]
    L.y2h_augment_to_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2_aug_draw_classification.argtypes = [C.c_int] * 5 + [C.c_float] * 5 + [C.POINTER(AugClsItem)]
    L.y2_aug_labels.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(Tree), C.c_void_p]
    L.y2_net_augment_classifier.argtypes = [CNetwork] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_float)] * 5
    L.y2_train_load_classification.argtypes = [C.POINTER(CNetwork), C.POINTER(AugClsItem), C.c_void_p, C.c_int, C.c_int]
    L.y2_aug_cls_rect.restype = None
    L.y2_aug_cls_rect.argtypes = [C.POINTER(AugClsItem), C.c_int] + [C.POINTER(C.c_int)] * 4
    L.y2_aug_cls_pack_bytes.restype = C.c_size_t
    L.y2_aug_cls_pack_bytes.argtypes = [C.POINTER(AugClsItem), C.c_int, C.c_int]
    L.y2_aug_cls_pack.restype = None
    L.y2_aug_cls_pack.argtypes = [C.POINTER(AugClsItem), C.c_int, C.c_int, C.POINTER(AugCls), C.c_void_p]
    L.y2h_augment_cls_to_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2_dream_draw.restype = None
    L.y2_dream_draw.argtypes = [C.c_int, C.c_int, C.POINTER(DreamDraws)]
    L.y2_dream_scale.restype = C.c_float
    L.y2_dream_scale.argtypes = [C.c_int]
    L.y2_dream_size.restype = None
    L.y2_dream_size.argtypes = [C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.y2_dream_check.argtypes = [C.POINTER(CNetwork), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    L.y2_dream_open.restype = C.c_void_p
    L.y2_dream_open.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.y2_dream_step.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.y2_dream_round_end.argtypes = [C.c_void_p, C.c_float, C.c_float]
    L.y2_dream_fetch.argtypes = [C.c_void_p, C.c_void_p]
    L.y2_dream_stats.argtypes = [C.c_void_p, C.POINTER(DreamCounters)]
    L.y2_dream_pull.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.y2_dream_close.restype = None
    L.y2_dream_close.argtypes = [C.c_void_p]
    L.optimize_picture.restype = None
    L.optimize_picture.argtypes = [C.POINTER(CNetwork), Image, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
    L.y2_nightmare.argtypes = [C.POINTER(CNetwork), Image, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.y2h_dream_resample_tmp_floats.restype = C.c_size_t
    L.y2h_dream_resample_tmp_floats.argtypes = [C.POINTER(DreamResample)]
    L.y2h_dream_resample_run.argtypes = [C.POINTER(DreamResample), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_dream_chunks.argtypes = [C.c_long]
    L.y2h_dream_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_dream_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_dream_rotate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    L.y2h_stream_k_launches.restype = C.c_ulong
    L.y2h_tail_launches.restype = C.c_ulong
    L.y2h_xcd_order_launches.restype = C.c_ulong
    L.y2h_f32_stream_k_launches.restype = C.c_ulong
    L.y2_kcf_plan.argtypes = [C.POINTER(KcfBox), C.POINTER(KcfGeometry)]
    L.y2_kcf_init.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.y2_kcf_track.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2_kcf_count.argtypes = [CNetwork]
    L.y2_kcf_fetch.argtypes = [CNetwork, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.y2_kcf_dft.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.y2_kcf_free.argtypes = [CNetwork]
    L.y2_kcf_free.restype = None
    L.y2_kcf_init_objects.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Object), C.c_int]
    L.y2_kcf_init_objects.restype = None
    L.y2_kcf_track_objects.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Object), C.POINTER(C.c_int)]
    L.y2_kcf_track_objects.restype = None
    # Go (go.c; include/sr_yolo2.h, include/y2_hip.h y2h_go_*)
    for f in (L.string_to_board, L.board_to_string, L.flip_board, L.move_go, L.print_board, L.predict_move, L.y2_go_free_moves):
        f.restype = None
    L.string_to_board.argtypes = [C.c_void_p, C.c_void_p]
    L.board_to_string.argtypes = [C.c_void_p, C.c_void_p]
    L.flip_board.argtypes = [C.c_void_p]
    L.calculate_liberties.restype = C.POINTER(C.c_int)
    L.calculate_liberties.argtypes = [C.c_void_p]
    L.move_go.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.suicide_go.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.legal_go.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.print_board.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.load_go_moves.restype = GoMoves
    L.load_go_moves.argtypes = [C.c_char_p]
    L.y2_go_free_moves.argtypes = [GoMoves]
    L.y2_go_draw_moves.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.predict_move.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_int]
    L.generate_move.argtypes = [CNetwork, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int]
    L.y2_go_predict.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.y2_go_rules.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2_go_generate.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.y2_go_valid.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.y2_go_selfplay.argtypes = [CNetwork, CNetwork, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.y2_go_set_poll.argtypes = [CNetwork, C.c_int]
    L.y2_train_load_go.argtypes = [C.POINTER(CNetwork), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_go_views.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_go_merge.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_go_rules.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_go_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_go_play.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.y2h_go_pick.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.y2h_go_argmax.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.y2h_go_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def _check():
    L = lib()
    msg = L.y2_last_error()
    L.y2_failed_and_clear()          # the error is being raised here: do not let the flag leak into the next call
    return msg.decode() if msg else ""


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def regions(items):
    """items: list of (frame uint8 [h][w][c] or [h][w], (x, y, rw, rh) or None = the whole frame) -> (Region array,
    frames kept alive for the call).  A frame whose rows are padded (a view of a wider buffer) is passed with its
    row pitch as `step`, without a copy."""
    arr = (Region * max(len(items), 1))()
    keep = []
    for i, (frame, rect) in enumerate(items):
        f = np.asarray(frame)
        if f.ndim == 2:
            f = f[:, :, None]
        if f.dtype != np.uint8 or f.strides[2] != 1 or f.strides[1] != f.shape[2] or f.strides[0] < f.shape[1] * f.shape[2]:
            f = np.ascontiguousarray(f, dtype=np.uint8)
        keep.append(f)
        h, w, c = f.shape
        x, y, rw, rh = rect if rect is not None else (0, 0, 0, 0)
        arr[i] = Region(f.ctypes.data, h, w, c, f.strides[0], x, y, rw, rh)
    return arr, keep


def aug_items(items):
    """items: list of dicts -- frame (uint8 [h][w][c >= 3]; a view of a wider buffer keeps its row pitch), the draws pleft,
    ptop, swidth, sheight, flip, dhue, dsat, dexp (default: the whole frame, unchanged), boxes (float32 [n][5] = id x y w h, or
    None) and swaps (int32 [n], or None) -> (AugItem array, arrays kept alive for the call)"""
    arr = (AugItem * max(len(items), 1))()
    keep = []
    for i, it in enumerate(items):
        f = np.asarray(it["frame"])
        if f.ndim != 3 or f.dtype != np.uint8 or f.strides[2] != 1 or f.strides[1] != f.shape[2] or f.strides[0] < f.shape[1] * f.shape[2]:
            f = np.ascontiguousarray(f, dtype=np.uint8)
            if f.ndim == 2:
                f = f[:, :, None]
        h, w, c = f.shape
        boxes = it.get("boxes")
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 5) if boxes is not None and len(boxes) else None
        swaps = it.get("swaps")
        swaps = np.ascontiguousarray(swaps, dtype=np.int32) if swaps is not None and boxes is not None else None
        keep += [f, boxes, swaps]
        arr[i] = AugItem(f.ctypes.data, h, w, c, f.strides[0], it.get("pleft", 0), it.get("ptop", 0), it.get("swidth", w),
                         it.get("sheight", h), int(it.get("flip", 0)), it.get("dhue", 0.), it.get("dsat", 1.), it.get("dexp", 1.),
                         boxes.ctypes.data if boxes is not None else None, len(boxes) if boxes is not None else 0,
                         swaps.ctypes.data if swaps is not None else None)
    return arr, keep


def aug_random_paths(n: int, m: int) -> np.ndarray:
    """y2_aug_random_paths: get_random_paths' n draws of random_gen() % m, from libc rand()"""
    out = np.zeros(max(n, 1), np.int32)
    lib().y2_aug_random_paths(n, m, _ptr(out))
    return out[:n]


def aug_draw_detection(ow: int, oh: int, jitter: float, hue: float, saturation: float, exposure: float, nboxes: int) -> dict:
    """y2_aug_draw_detection: one image's draws of load_data_detection, in the reference's rand() order -> the keys of
    aug_items (without frame and boxes)"""
    it = AugItem()
    swaps = np.zeros(max(nboxes, 1), np.int32)
    lib().y2_aug_draw_detection(ow, oh, jitter, hue, saturation, exposure, nboxes, C.byref(it), _ptr(swaps))
    d = {k: getattr(it, k) for k in ("pleft", "ptop", "swidth", "sheight", "flip", "dhue", "dsat", "dexp")}
    d["swaps"] = swaps[:nboxes]
    return d


def aug_random_dim() -> int:
    """y2_aug_random_dim: train_detector's random=1 size, (rand() % 10 + 10) * 32"""
    return int(lib().y2_aug_random_dim())


def aug_truth_detection(item: dict, num_boxes: int = 30) -> np.ndarray:
    """y2_aug_truth_detection: the truth row [num_boxes * 5] of one aug_items dict (its frame gives ow, oh)"""
    arr, keep = aug_items([item])
    out = np.zeros(num_boxes * 5, np.float32)
    if lib().y2_aug_truth_detection(arr, num_boxes, _ptr(out)) != 0:
        raise Y2Error("y2_aug_truth_detection: " + _check())
    return out


CLS_DRAWS = ("aspect", "scale", "rad", "dx", "dy", "flip", "dhue", "dsat", "dexp")


def aug_cls_items(items):
    """items: list of dicts -- frame (uint8 [h][w][c >= 3]; a view of a wider buffer keeps its row pitch) and the draws
    aspect, scale, rad, dx, dy, flip, dhue, dsat, dexp (default: the centred crop at scale 1, unchanged) -> (AugClsItem
    array, arrays kept alive for the call)"""
    arr = (AugClsItem * max(len(items), 1))()
    keep = []
    for i, it in enumerate(items):
        f = np.asarray(it["frame"])
        if f.ndim != 3 or f.dtype != np.uint8 or f.strides[2] != 1 or f.strides[1] != f.shape[2] or f.strides[0] < f.shape[1] * f.shape[2]:
            f = np.ascontiguousarray(f, dtype=np.uint8)
            if f.ndim == 2:
                f = f[:, :, None]
        h, w, c = f.shape
        keep.append(f)
        arr[i] = AugClsItem(f.ctypes.data, h, w, c, f.strides[0], it.get("aspect", 1.), it.get("scale", 1.), it.get("rad", 0.),
                            it.get("dx", 0.), it.get("dy", 0.), int(it.get("flip", 0)), it.get("dhue", 0.), it.get("dsat", 1.),
                            it.get("dexp", 1.))
    return arr, keep


def aug_draw_classification(ow: int, oh: int, min_crop: int, max_crop: int, size: int, angle: float, aspect: float, hue: float,
                            saturation: float, exposure: float) -> dict:
    """y2_aug_draw_classification: one image's draws of load_image_augment_paths, in the reference's rand() order -> the
    draw keys of aug_cls_items; Y2Error when the frame's shorter side truncates to 0"""
    it = AugClsItem()
    if lib().y2_aug_draw_classification(ow, oh, min_crop, max_crop, size, angle, aspect, hue, saturation, exposure, C.byref(it)) != 0:
        raise Y2Error("y2_aug_draw_classification: " + _check())
    return {k: getattr(it, k) for k in CLS_DRAWS}


def aug_labels(path: str, labels, hierarchy=None):
    """y2_aug_labels: fill_truth (and fill_hierarchy with a Tree) -> (truth float32 [len(labels)], matching labels)"""
    names = (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels])
    out = np.zeros(max(len(labels), 1), np.float32)
    n = lib().y2_aug_labels(path.encode(), names, len(labels), hierarchy, _ptr(out))
    if n < 0:
        raise Y2Error("y2_aug_labels: " + _check())
    return out[:len(labels)], n


def aug_cls_rect(item: dict, size: int) -> tuple:
    """the frame rectangle (x0, y0, rw, rh) the packer sends up for one aug_cls_items dict"""
    arr, keep = aug_cls_items([item])
    v = [C.c_int(0) for _ in range(4)]
    lib().y2_aug_cls_rect(arr, size, *[C.byref(k) for k in v])
    return tuple(k.value for k in v)


def srand(seed: int) -> None:
    """libc srand: the loader's draws come from libc rand(), as the reference's do"""
    C.CDLL(None).srand(C.c_uint(seed))


def images(frames):
    """frames: list of float32 [c][h][w] arrays of any size -> (Image array, arrays kept alive for the call)"""
    keep = [np.ascontiguousarray(f, dtype=np.float32) for f in frames]
    for f in keep:
        if f.ndim != 3:
            raise ValueError("a frame is [c][h][w]")
    arr = (Image * max(len(keep), 1))()
    for i, f in enumerate(keep):
        arr[i] = Image(f.shape[1], f.shape[2], f.shape[0], f.ctypes.data_as(C.POINTER(C.c_float)))
    return arr, keep


def set_view_block_bytes(nbytes: int = 0) -> None:
    """HBM budget of one block of frames in the classifier view modes (0: the default, Y2_VIEW_BLOCK_BYTES)"""
    lib().y2_set_view_block_bytes(nbytes)


def view_resizes() -> int:
    """resize_network calls the classifier view modes made so far (one per distinct resized size per block)"""
    return int(lib().y2_view_resizes())


def d2h_copies() -> int:
    return int(lib().y2h_d2h_copies())


def stream_syncs() -> int:
    """y2h_stream_sync calls so far: the host waits of this process"""
    return int(lib().y2h_stream_syncs())


def otsu_threshold(hist) -> int:
    """y2_otsu_threshold: otsuThreshold (KinectUtil_with_cam.cpp:1564-1630) of a 256-bin histogram, on the host"""
    h = np.ascontiguousarray(hist, dtype=np.int32)
    if h.shape != (256,):
        raise ValueError("a histogram has 256 bins")
    return int(lib().y2_otsu_threshold(_ptr(h)))


def plane_samples(depth, far_m: float, iters: int, seed: int) -> np.ndarray:
    """y2_plane_samples: the sampler of include/y2_plane_rule.h over a depth frame -> int32 [iters][3], -1 = void"""
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    out = np.zeros((max(iters, 1), 3), np.int32)
    if lib().y2_plane_samples(_ptr(depth), depth.shape[0], depth.shape[1], far_m, iters, seed & 0xFFFFFFFF, _ptr(out)) < 0:
        raise Y2Error("y2_plane_samples: bad arguments")
    return out[:iters]


DENSE_FORWARD, DENSE_DINPUT = 0, 1     # include/y2_hip.h Y2H_DENSE_FORWARD / Y2H_DENSE_DINPUT


def get_rnn_data(text: bytes, offsets: np.ndarray, characters: int, batch: int, steps: int):
    """rnn.c:86-114 through the library: (x, y) float32 [steps*batch][characters]; `offsets` (uint64 [batch]) advances in place"""
    if offsets.dtype != np.uint64 or not offsets.flags.c_contiguous or offsets.size != batch:
        raise ValueError("get_rnn_data: offsets must be a contiguous uint64 array of `batch` values")
    x = np.empty((steps * batch, characters), np.float32)
    y = np.empty((steps * batch, characters), np.float32)
    if lib().y2_get_rnn_data(text, _ptr(offsets), characters, len(text), batch, steps, _ptr(x), _ptr(y)) != 0:
        raise Y2Error("get_rnn_data: " + _check())
    return x, y


def train_dense_plan(batch: int, inputs: int, outputs: int, product: int = DENSE_FORWARD, forced: int = 0):
    """y2h_train_dense_plan: how the trainer cuts the reduction of a dense layer's forward (over inputs) or input-gradient
    (over outputs) product, on the host (no GPU) -> (ranges, workspace bytes, bounds[ranges + 1])"""
    g = TrainDense(batch, inputs, outputs)
    n, ws = C.c_int(0), C.c_size_t(0)
    if lib().y2h_train_dense_plan(C.byref(g), product, forced, C.byref(n), C.byref(ws), None, 0) != 0:
        raise Y2Error("y2h_train_dense_plan: bad arguments")
    bounds = np.zeros(n.value + 1, np.int32)
    lib().y2h_train_dense_plan(C.byref(g), product, forced, C.byref(n), C.byref(ws), _ptr(bounds), bounds.size)
    return n.value, ws.value, bounds


def connected_f16_plan(rows: int, inputs: int, outputs: int, forced: int = 0):
    """y2h_connected_f16_plan: how fp16 mode cuts a dense layer of `inputs` x `outputs` along K, on the host (no GPU) ->
    (K ranges, bytes of partial-sum workspace, int32 [ranges + 1] range bounds); forced > 0 sets the number of ranges"""
    n, ws = C.c_int(0), C.c_size_t(0)
    bounds = np.zeros((inputs + 31) // 32 + 1, np.int32)
    if lib().y2h_connected_f16_plan(rows, inputs, outputs, forced, C.byref(n), C.byref(ws), _ptr(bounds), bounds.size) != 0:
        raise Y2Error("y2h_connected_f16_plan: bad arguments")
    return n.value, ws.value, bounds[:n.value + 1].copy()


def plane_from_points(p0, p1, p2):
    """y2_plane_from_points: three float32 points -> (ok, float32 [4] = nx, ny, nz, d)"""
    pts = [np.ascontiguousarray(p, dtype=np.float32) for p in (p0, p1, p2)]
    out = np.zeros(4, np.float32)
    ok = lib().y2_plane_from_points(_ptr(pts[0]), _ptr(pts[1]), _ptr(pts[2]), _ptr(out))
    return int(ok), out


def plane_fit(sums):
    """y2_plane_fit: float64 [10] = n, x, y, z, xx, xy, xz, yy, yz, zz -> (ok, float64 [4] = a, b, c, d)"""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    out = np.zeros(4, np.float64)
    ok = lib().y2_plane_fit(_ptr(sums), _ptr(out))
    return int(ok), out


def depth_roi(box, W: int, H: int):
    """y2_depth_roi: (valid, left, top, right, bot) of a frame-relative (x, y, w, h) box in a W x H frame"""
    v = [C.c_int(0) for _ in range(4)]
    ok = lib().y2_depth_roi(Box(*[float(np.float32(b)) for b in box]), W, H, *[C.byref(t) for t in v])
    return (int(ok),) + tuple(t.value for t in v)


def region_box_to_frame(item, net_w: int, net_h: int, letterbox: bool, box):
    """y2_region_box_to_frame: (x, y, w, h) relative to the network input -> relative to the item's frame (fp32)"""
    arr, keep = regions([item])
    v = [C.c_float(float(b)) for b in box]
    lib().y2_region_box_to_frame(arr, net_w, net_h, int(letterbox), *[C.byref(t) for t in v])
    return np.array([t.value for t in v], dtype=np.float32)


def _rows(probs: np.ndarray):
    """float** view of a C-contiguous [total][classes] array."""
    total = probs.shape[0]
    arr = (C.POINTER(C.c_float) * total)()
    base = probs.ctypes.data
    stride = probs.strides[0]
    for i in range(total):
        arr[i] = C.cast(base + i * stride, C.POINTER(C.c_float))
    return arr


class Network:
    """Owns a `network` struct of libsr_yolo2 (the by-value struct of the reference API)."""

    def __init__(self, cnet: CNetwork):
        self.net = cnet
        self._freed = False

    # --- parser.h ---
    @classmethod
    def parse_network_cfg(cls, filename: str, gpu: int = 0) -> "Network":
        L = lib()
        C.c_int.in_dll(L, "gpu_index").value = gpu
        net = L.parse_network_cfg(filename.encode())
        if not net.layers:
            raise Y2Error("parse_network_cfg(%s): %s" % (filename, _check()))
        return cls(net)

    def load_weights(self, filename: str) -> None:
        L = lib()
        if not os.path.exists(filename):
            raise Y2Error("Couldn't open file: %s" % filename)
        L.load_weights(C.byref(self.net), filename.encode())

    def save_weights(self, filename: str) -> None:
        lib().save_weights(self.net, filename.encode())

    # --- network.h ---
    def denormalize(self) -> None:
        """darknet.c:309 denormalize_net: fold batch-norm into weights/biases of every conv layer, clear the flag."""
        lib().y2_denormalize_network(C.byref(self.net))

    def set_batch_network(self, b: int) -> None:
        lib().set_batch_network(C.byref(self.net), b)

    def resize_network(self, w: int, h: int) -> None:
        if lib().resize_network(C.byref(self.net), w, h) != 0:
            raise Y2Error("resize_network: " + _check())

    def network_predict(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if x.size != self.net.batch * self.net.inputs:
            raise ValueError("input has %d floats, network wants %d x %d" % (x.size, self.net.batch, self.net.inputs))
        p = lib().network_predict(self.net, _ptr(x))
        if not p:
            raise Y2Error("network_predict: " + _check())
        return np.ctypeslib.as_array(p, shape=(self.net.batch * self.output_size,)).copy()

    def reset_rnn_state(self, b: int = -1) -> None:
        """rnn.c:116: zero item b's state in every [rnn] / [gru] layer (b = -1: every item), ordered with the forwards"""
        L = lib()
        L.reset_rnn_state(self.net, b)
        if L.y2_failed_and_clear():
            raise Y2Error("reset_rnn_state: " + _check())

    def set_temperature(self, t: float) -> None:
        """test_char_rnn (rnn.c:244): the temperature on every layer; [softmax] reads it at each call"""
        for i in range(self.net.n):
            self.net.layers[i].temperature = t

    @property
    def output_size(self) -> int:
        return lib().get_network_output_size(self.net)

    @property
    def n(self) -> int:
        return self.net.n

    @property
    def batch(self) -> int:
        return self.net.batch

    def layer(self, i: int) -> Layer:
        return self.net.layers[i]

    @property
    def last(self) -> Layer:
        return self.net.layers[self.net.n - 1]

    def layer_table(self):
        rows = []
        for i in range(self.net.n):
            l = self.net.layers[i]
            rows.append(dict(type=LAYER_TYPES[l.type].lower(), w=l.w, h=l.h, c=l.c, out_w=l.out_w, out_h=l.out_h,
                             out_c=l.out_c, outputs=l.outputs, n=l.n, size=l.size, stride=l.stride, pad=l.pad,
                             batch_normalize=l.batch_normalize, classes=l.classes, coords=l.coords))
        return rows

    # --- region_layer.h / box.h ---
    def get_region_boxes(self, w: int, h: int, thresh: float, only_objectness: int = 0, use_map: bool = False,
                         batch_item: int = 0, output: np.ndarray | None = None):
        """-> (boxes[total,4], probs[total,classes]) for one batch item (the reference reads item 0:
        region_layer.c:331; other items are reached the way Detector does it, by offsetting l.output)."""
        L = lib()
        l = Layer.from_buffer_copy(self.last)
        total = l.w * l.h * l.n
        if output is not None:
            buf = np.ascontiguousarray(output, dtype=np.float32)
            l.output = buf.ctypes.data_as(C.POINTER(C.c_float))
        elif batch_item:
            l.output = C.cast(C.addressof(l.output.contents) + batch_item * l.outputs * 4, C.POINTER(C.c_float))
        boxes = np.zeros((total, 4), dtype=np.float32)
        probs = np.zeros((total, l.classes), dtype=np.float32)
        rows = _rows(probs)
        mp = l.map if (use_map and l.map) else None
        L.get_region_boxes(l, w, h, thresh, rows, _ptr(boxes), only_objectness, mp)
        if L.y2_failed_and_clear():
            raise Y2Error("get_region_boxes: " + _check())
        return boxes, probs

    def get_detection_boxes(self, w: int, h: int, thresh: float, only_objectness: int = 0, batch_item: int = 0):
        """YOLOv1 head: detection_layer.c:222 -> (boxes[side*side*num,4], probs[side*side*num,classes])"""
        L = lib()
        L.get_detection_boxes.argtypes = [Layer, C.c_int, C.c_int, C.c_float, C.POINTER(C.POINTER(C.c_float)), C.c_void_p, C.c_int]
        l = Layer.from_buffer_copy(self.last)
        total = l.side * l.side * l.n
        if batch_item:
            l.output = C.cast(C.addressof(l.output.contents) + batch_item * l.outputs * 4, C.POINTER(C.c_float))
        boxes = np.zeros((total, 4), dtype=np.float32)
        probs = np.zeros((total, l.classes), dtype=np.float32)
        L.get_detection_boxes(l, w, h, thresh, _rows(probs), _ptr(boxes), only_objectness)
        if L.y2_failed_and_clear():
            raise Y2Error("get_detection_boxes: " + _check())
        return boxes, probs

    def test_detector_img(self, im: np.ndarray, thresh: float, names=None):
        """im: [c][h][w] float32 -> list of dicts (x,y,w,h,prob,objClass,name,boxRGB) (detector.c:558)."""
        L = lib()
        im = np.ascontiguousarray(im, dtype=np.float32)
        c, h, w = im.shape
        cim = Image(h, w, c, im.ctypes.data_as(C.POINTER(C.c_float)))
        objs = (Object * 2048)()
        cnt = C.c_int(0)
        cnames = None
        if names:
            cnames = (C.c_char_p * len(names))(*[n.encode() for n in names])
        L.test_detector_img(cnames, None, self.net, cim, thresh, objs, C.byref(cnt))
        if L.y2_failed_and_clear():
            raise Y2Error("test_detector_img: " + _check())
        out = []
        for i in range(cnt.value):
            o = objs[i]
            out.append(dict(x=o.x, y=o.y, w=o.w, h=o.h, prob=o.prob, objClass=o.objClass, name=o.name.decode(),
                            boxRGB=tuple(o.boxRGB)))
        return out

    def test_detector_img_for_grasping(self, im: np.ndarray, im_filter: np.ndarray, thresh: float, names=None):
        """detector.c:514: test_detector_img on im_filter; im is what the reference draws on"""
        L = lib()
        im = np.ascontiguousarray(im, dtype=np.float32)
        imf = np.ascontiguousarray(im_filter, dtype=np.float32)
        cim = Image(im.shape[1], im.shape[2], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_float)))
        cimf = Image(imf.shape[1], imf.shape[2], imf.shape[0], imf.ctypes.data_as(C.POINTER(C.c_float)))
        objs = (Object * 2048)()
        cnt = C.c_int(0)
        cnames = (C.c_char_p * len(names))(*[n.encode() for n in names]) if names else None
        L.test_detector_img_for_grasping(cnames, None, self.net, cim, cimf, thresh, objs, C.byref(cnt))
        if L.y2_failed_and_clear():
            raise Y2Error("test_detector_img_for_grasping: " + _check())
        return [dict(x=o.x, y=o.y, w=o.w, h=o.h, prob=o.prob, objClass=o.objClass, name=o.name.decode(), boxRGB=tuple(o.boxRGB))
                for o in objs[:cnt.value]]

    # --- training (include/sr_yolo2.h: train_network_datum and the y2_train_* calls it is written on) ---
    TRAIN_ARRAYS = ("output", "delta", "x", "x_norm", "mean", "variance", "mean_delta", "variance_delta", "weight_updates",
                    "bias_updates", "scale_updates", "weights", "biases", "scales", "rolling_mean", "rolling_variance", "rand")
    RNN_SUBS = ("input", "self", "output")

    def train_prepare(self) -> None:
        if lib().y2_train_prepare(C.byref(self.net)) != 0:
            raise Y2Error("y2_train_prepare: " + _check())

    def train_set_precision(self, mode: str) -> None:
        """y2_train_set_precision: "fp32" (the default), "bf16x3" (3-way bf16 split, fp32 results) or "bf16" (operands
        rounded to bf16, fp32 accumulation) for the three products of every convolution of a step; before train_prepare
        or between steps"""
        if mode not in TRAIN_PRECISIONS:
            raise Y2Error("train_set_precision: unknown mode %r (%s)" % (mode, ", ".join(TRAIN_PRECISIONS)))
        if lib().y2_train_set_precision(C.byref(self.net), TRAIN_PRECISIONS.index(mode)) != 0:
            raise Y2Error("y2_train_set_precision: " + _check())

    def train_precision(self) -> str:
        mode = lib().y2_train_precision(C.byref(self.net))
        if mode < 0:
            raise Y2Error("y2_train_precision: " + _check())
        return TRAIN_PRECISIONS[mode]

    def train_step(self, x: np.ndarray, y: np.ndarray) -> float:
        """one train_network_datum: x [batch][c][h][w]; y [batch][outputs] for a network that ends in [cost],
        [batch][30][x, y, w, h, class] (relative units, the list ends at the first x == 0) for one that ends in [region]
        -> the loss"""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
        if x.size != self.net.batch * self.net.inputs or y.size != self.net.batch * self.truth_floats():
            raise ValueError("train_step: x has %d floats, y has %d" % (x.size, y.size))
        loss = C.c_float(0)
        if lib().y2_train_step(C.byref(self.net), _ptr(x), _ptr(y), C.byref(loss)) != 0:
            raise Y2Error("y2_train_step: " + _check())
        return float(loss.value)

    def train_step_device(self, d_x: int, d_y: int) -> float:
        loss = C.c_float(0)
        if lib().y2_train_step_device(C.byref(self.net), C.c_void_p(d_x), C.c_void_p(d_y), C.byref(loss)) != 0:
            raise Y2Error("y2_train_step_device: " + _check())
        return float(loss.value)

    def net_augment(self) -> dict:
        """y2_net_augment: jitter and random of the closing [region] layer, [net] hue / saturation / exposure"""
        f = [C.c_float(0) for _ in range(4)]
        r = C.c_int(0)
        if lib().y2_net_augment(self.net, *[C.byref(v) for v in f], C.byref(r)) != 0:
            raise Y2Error("y2_net_augment: " + _check())
        return dict(jitter=f[0].value, hue=f[1].value, saturation=f[2].value, exposure=f[3].value, random=r.value)

    def train_load_detection(self, items, swap_rb: bool = False) -> None:
        """y2_train_load_detection: one batch of aug_items dicts -> the trainer's input and truth, built on the device"""
        arr, keep = aug_items(items)
        if lib().y2_train_load_detection(C.byref(self.net), arr, len(items), int(swap_rb)) != 0:
            raise Y2Error("y2_train_load_detection: " + _check())

    def net_augment_classifier(self) -> dict:
        """y2_net_augment_classifier: [net] min_crop / max_crop / angle / aspect / hue / saturation / exposure"""
        i = [C.c_int(0) for _ in range(2)]
        f = [C.c_float(0) for _ in range(5)]
        if lib().y2_net_augment_classifier(self.net, *[C.byref(v) for v in i + f]) != 0:
            raise Y2Error("y2_net_augment_classifier: " + _check())
        return dict(min_crop=i[0].value, max_crop=i[1].value, angle=f[0].value, aspect=f[1].value, hue=f[2].value,
                    saturation=f[3].value, exposure=f[4].value)

    def train_load_classification(self, items, truth, swap_rb: bool = False) -> None:
        """y2_train_load_classification: one batch of aug_cls_items dicts and its truth [batch][truth_floats()] -> the
        trainer's input and truth, built on the device"""
        arr, keep = aug_cls_items(items)
        if truth is not None:
            truth = np.ascontiguousarray(truth, dtype=np.float32).reshape(-1)
            if truth.size != self.net.batch * self.truth_floats():
                raise ValueError("train_load_classification: truth has %d floats" % truth.size)
        if lib().y2_train_load_classification(C.byref(self.net), arr, _ptr(truth) if truth is not None else None, len(items), int(swap_rb)) != 0:
            raise Y2Error("y2_train_load_classification: " + _check())

    def train_load_chars(self, text: bytes, offsets: np.ndarray) -> None:
        """y2_train_load_rnn_data: the next time_steps characters of each of the B = batch / time_steps streams -> the
        trainer's one-hot input and truth, written on the device; `offsets` (uint64 [B]) advances in place as get_rnn_data's"""
        if offsets.dtype != np.uint64 or not offsets.flags.c_contiguous or offsets.size != self.net.batch // max(self.net.time_steps, 1):
            raise ValueError("train_load_chars: offsets must be a contiguous uint64 array of batch / time_steps values")
        if lib().y2_train_load_rnn_data(C.byref(self.net), text, len(text), _ptr(offsets)) != 0:
            raise Y2Error("y2_train_load_rnn_data: " + _check())

    def train_step_loaded(self) -> float:
        loss = C.c_float(0)
        if lib().y2_train_step_loaded(C.byref(self.net), C.byref(loss)) != 0:
            raise Y2Error("y2_train_step_loaded: " + _check())
        return float(loss.value)

    def train_pull_input(self):
        """the loaded batch as the reference holds it: x [batch][3][h][w], truth [batch][150] (a classifier: [batch][truth_floats()])"""
        flat = not (self.net.h > 0 and self.net.w > 0 and self.net.c > 0)       # inputs= in front of an [rnn]: rows as given
        x = np.zeros((self.net.batch, self.net.inputs) if flat else (self.net.batch, self.net.c, self.net.h, self.net.w), np.float32)
        y = np.zeros((self.net.batch, 150 if LAYER_TYPES[self.net.layers[self.net.n - 1].type] == "REGION" else self.truth_floats()), np.float32)
        if lib().y2_train_pull_input(C.byref(self.net), _ptr(x), _ptr(y)) != 0:
            raise Y2Error("y2_train_pull_input: " + _check())
        return x, y

    def train_load_times(self) -> tuple:
        """host wall ms of the last load: (pack, enqueue, wait for the copy)"""
        ms = np.zeros(3, np.float32)
        if lib().y2_train_load_times(C.byref(self.net), _ptr(ms)) != 0:
            raise Y2Error("y2_train_load_times: " + _check())
        return tuple(float(v) for v in ms)

    def train_sync(self) -> None:
        if lib().y2_train_sync(C.byref(self.net)) != 0:
            raise Y2Error("y2_train_sync: " + _check())

    def train_pull(self, layer: int, what: str) -> np.ndarray:
        """one array of the trainer in the reference's order: activations [batch][c][h][w], weights [n][c][size][size] (a
        [connected] layer's [outputs][inputs]); "rand" is a [dropout] layer's draws of the last step, [batch][inputs]"""
        l = self.net.layers[layer]
        if what == "state" or "." in what:
            # an [rnn]: "state" is [time_steps + 1][B][hidden]; "input.weights", "self.delta", "output.x_norm" ... name an
            # array of a sub-layer: activations [time_steps * B][outputs] (rows step-major), mean / variance the last step's
            if LAYER_TYPES[l.type] != "RNN":
                raise Y2Error("train_pull: layer %d is no [rnn] layer: it has no %r" % (layer, what))
            if what == "state":
                code, n = len(self.TRAIN_ARRAYS), (l.steps + 1) * l.batch * l.hidden
            else:
                sub, name = what.split(".", 1)
                if sub not in self.RNN_SUBS or name not in self.TRAIN_ARRAYS[:-1]:
                    raise Y2Error("train_pull: unknown array %r (input. / self. / output. and one of %s)" % (what, ", ".join(self.TRAIN_ARRAYS[:-1])))
                k = self.RNN_SUBS.index(sub)
                ins, outs = ((l.inputs, l.hidden), (l.hidden, l.hidden), (l.hidden, l.outputs))[k]
                base = self.TRAIN_ARRAYS.index(name)
                code = ((k + 1) << 8) | base
                n = self.net.batch * outs if base < 4 else (ins * outs if name in ("weights", "weight_updates") else outs)
            out = np.zeros(max(n, 1), np.float32)
            if lib().y2_train_pull(C.byref(self.net), layer, code, _ptr(out), n) != 0:
                raise Y2Error("y2_train_pull: " + _check())
            return out[:n]
        code = self.TRAIN_ARRAYS.index(what)
        if code < 4 or what == "rand":
            n = self.net.batch * l.outputs
        elif what in ("weights", "weight_updates"):
            n = l.n * l.c * l.size * l.size
        else:
            n = l.n
        out = np.zeros(max(n, 1), np.float32)
        if lib().y2_train_pull(C.byref(self.net), layer, code, _ptr(out), n) != 0:
            raise Y2Error("y2_train_pull: " + _check())
        return out[:n]

    def truth_floats(self) -> int:
        """floats of truth per image of a training step: l.truths behind a [region] head (150) or a [detection] head
        (side*side*(1+coords+classes)), the inputs of a [cost]"""
        n = lib().y2_train_truth_floats(C.byref(self.net))
        if n < 0:
            raise Y2Error("y2_train_truth_floats: " + _check())       # a network the trainer refuses says so first
        return n

    def train_region_stats(self, layer: int = -1) -> dict:
        """what the reference prints per forward_region_layer call, of the last step (NaN averages when count == 0)"""
        st = RegionStats()
        if lib().y2_train_region_stats(C.byref(self.net), layer if layer >= 0 else self.net.n - 1, C.byref(st)) != 0:
            raise Y2Error("y2_train_region_stats: " + _check())
        return {k: getattr(st, k) for k, _ in RegionStats._fields_}

    def train_detection_stats(self, layer: int = -1) -> dict:
        """what the reference prints per forward_detection_layer call, of the last step (NaN averages when count == 0)"""
        st = DetectionStats()
        if lib().y2_train_detection_stats(C.byref(self.net), layer if layer >= 0 else self.net.n - 1, C.byref(st)) != 0:
            raise Y2Error("y2_train_detection_stats: " + _check())
        return {k: getattr(st, k) for k, _ in DetectionStats._fields_}

    def train_free(self) -> None:
        lib().y2_train_free(C.byref(self.net))

    # --- dreaming (nightmare.c) ---
    def dream_check(self, max_layer: int, c: int, h: int, w: int, scale: float = 1.0) -> None:
        """every refusal of a dream step, by name, without a device call"""
        if lib().y2_dream_check(C.byref(self.net), max_layer, c, h, w, scale) != 0:
            raise Y2Error("y2_dream_check: " + _check())

    def dream_open(self, picture: np.ndarray) -> "Dream":
        """a dream context on this batch-1 network: picture float32 [c][h][w], uploaded once and kept in HBM"""
        return Dream(self, picture)

    def optimize_picture(self, picture: np.ndarray, max_layer: int, scale: float, rate: float, thresh: float, norm: int) -> np.ndarray:
        """nightmare.c:34 with its own three rand() draws (libc's: seed with darknet.srand); returns the new picture"""
        p = np.array(picture, dtype=np.float32, order="C", copy=True)
        c, h, w = p.shape
        L = lib()
        L.optimize_picture(C.byref(self.net), Image(h, w, c, p.ctypes.data_as(C.POINTER(C.c_float))), max_layer, scale, rate, thresh, norm)
        if L.y2_failed_and_clear():
            raise Y2Error("optimize_picture: " + _check())
        return p

    def nightmare(self, picture: np.ndarray, max_layer: int, range_: int = 1, norm: int = 1, rounds: int = 1, iters: int = 10,
                  octaves: int = 4, zoom: float = 1.0, rate: float = .04, thresh: float = 1.0, rotate: float = 0.0, per_round=None) -> np.ndarray:
        """run_nightmare's loop (nightmare.c:258-306) with its defaults and libc's rand(); per_round(round, picture [c][h][w]) sees
        each round's picture, fetched once per round; returns the last round's"""
        p = np.array(picture, dtype=np.float32, order="C", copy=True)
        c, h, w = p.shape
        cb_t = C.CFUNCTYPE(None, C.c_int, Image, C.c_void_p)
        cb = cb_t(lambda r, im, user: per_round(r, np.ctypeslib.as_array(im.data, shape=(c, h, w)).copy())) if per_round else None
        rc = lib().y2_nightmare(C.byref(self.net), Image(h, w, c, p.ctypes.data_as(C.POINTER(C.c_float))), max_layer, range_, norm, rounds,
                                iters, octaves, zoom, rate, thresh, rotate, C.cast(cb, C.c_void_p) if cb else None, None)
        if rc != 0:
            raise Y2Error("y2_nightmare: " + _check())
        return p

    def get_current_rate(self) -> float:
        return float(lib().get_current_rate(self.net))

    def get_current_batch(self) -> int:
        return int(lib().get_current_batch(self.net))

    def get_network_cost(self) -> float:
        return float(lib().get_network_cost(self.net))

    # --- extensions ---
    def prepare(self) -> None:
        if lib().y2_prepare(C.byref(self.net)) != 0:
            raise Y2Error("y2_prepare: " + _check())

    def set_strict(self, on: bool) -> None:
        lib().y2_set_strict(C.byref(self.net), 1 if on else 0)

    def set_half(self, on: bool) -> None:
        """fp16 storage / fp32 accumulate (engine extension, include/sr_yolo2.h y2_set_half)."""
        lib().y2_set_half(C.byref(self.net), 1 if on else 0)

    def set_autotune(self, on: bool) -> None:
        """measure the conv tile shapes at plan time instead of modelling them (include/sr_yolo2.h y2_set_autotune)"""
        lib().y2_set_autotune(C.byref(self.net), 1 if on else 0)

    def set_fusion(self, on: bool) -> None:
        lib().y2_set_fusion(C.byref(self.net), 1 if on else 0)

    def set_detect_overlap(self, on: bool) -> None:
        """decode / NMS of batch i on their own stream beside the forward of batch i+1 (include/sr_yolo2.h y2_set_detect_overlap)"""
        lib().y2_set_detect_overlap(C.byref(self.net), 1 if on else 0)

    def set_graph(self, on: bool) -> None:
        """replay the forward pass from a hipGraph (include/sr_yolo2.h y2_set_graph)"""
        lib().y2_set_graph(C.byref(self.net), 1 if on else 0)

    def set_timing(self, on: bool) -> None:
        lib().y2_set_timing(C.byref(self.net), 1 if on else 0)

    def layer_times_ms(self) -> np.ndarray:
        ms = np.zeros(self.net.n, dtype=np.float32)
        n = lib().y2_layer_times_ms(self.net, _ptr(ms), self.net.n)
        return ms[:n]

    def layer_kernel(self, i: int) -> str:
        return lib().y2_layer_kernel(self.net, i).decode()

    def weights_arena(self):
        p = C.c_void_p()
        n = C.c_size_t()
        if lib().y2_weights_arena(C.byref(self.net), C.byref(p), C.byref(n)) != 0:
            raise Y2Error("y2_weights_arena: " + _check())
        return p.value, n.value

    def weights_layout(self):
        """(layout signature, bytes) of the weight arena: equal on every rank or the replication is refused"""
        sig, b = C.c_ulonglong(0), C.c_size_t(0)
        if lib().y2_weights_layout(C.byref(self.net), C.byref(sig), C.byref(b)) != 0:
            raise Y2Error("y2_weights_layout: " + _check())
        return int(sig.value), int(b.value)

    def weights_resident(self) -> None:
        lib().y2_weights_resident(C.byref(self.net))

    def broadcast_weights(self, comm: int, root: int = 0) -> None:
        """one in-place RCCL broadcast of the packed arena (include/sr_yolo2.h y2_broadcast_weights)"""
        if lib().y2_broadcast_weights(C.byref(self.net), C.c_void_p(comm), root) != 0:
            raise Y2Error("y2_broadcast_weights: " + _check())

    # --- pinned, multi-buffered host feed (include/sr_yolo2.h y2_feed_*) ---
    def feed_open(self, slots: int = 2, slot_bytes: int = 0) -> None:
        if lib().y2_feed_open(C.byref(self.net), slots, slot_bytes) != 0:
            raise Y2Error("y2_feed_open: " + _check())

    def feed_close(self) -> None:
        lib().y2_feed_close(C.byref(self.net))

    def feed_host(self, slot: int, dtype=np.float32) -> np.ndarray:
        """numpy view of the slot's PINNED host buffer (the producer writes frames here)"""
        p = lib().y2_feed_host(self.net, slot)
        if not p:
            raise Y2Error("y2_feed_host: " + _check())
        n = lib().y2_feed_slot_bytes(self.net)
        buf = (C.c_ubyte * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype)

    def feed_submit(self, slot: int, nbytes: int = 0) -> None:
        if lib().y2_feed_submit(self.net, slot, nbytes) != 0:
            raise Y2Error("y2_feed_submit: " + _check())

    def feed_wait_host(self, slot: int) -> None:
        if lib().y2_feed_wait_host(self.net, slot) != 0:
            raise Y2Error("y2_feed_wait_host: " + _check())

    def feed_forward(self, slot: int) -> None:
        if lib().y2_feed_forward(self.net, slot) != 0:
            raise Y2Error("y2_feed_forward: " + _check())

    def feed_forward_u8(self, slot: int, h: int, w: int, c: int, step: int = 0, swap_rb: bool = True, letterbox: bool = False) -> None:
        if lib().y2_feed_forward_u8(self.net, slot, h, w, c, step or w * c, 1 if swap_rb else 0, 1 if letterbox else 0) != 0:
            raise Y2Error("y2_feed_forward_u8: " + _check())

    def forward_device(self, d_input: int) -> None:
        if lib().y2_forward_device(self.net, C.c_void_p(d_input)) != 0:
            raise Y2Error("y2_forward_device: " + _check())

    def predict_device(self, d_input: int) -> np.ndarray:
        p = lib().y2_network_predict_device(self.net, C.c_void_p(d_input))
        if not p:
            raise Y2Error("y2_network_predict_device: " + _check())
        return np.ctypeslib.as_array(p, shape=(self.net.batch * self.output_size,)).copy()

    def detect_resident(self, thresh: float, nms: float, img_w: int = 1, img_h: int = 1, max_per_image: int | None = None):
        l = self.last
        cap = max_per_image or (l.w * l.h * l.n)
        dets = np.zeros((self.net.batch, cap), dtype=DET_DTYPE)
        counts = np.zeros(self.net.batch, dtype=np.int32)
        if lib().y2_detect_resident(self.net, thresh, nms, img_w, img_h, _ptr(dets), _ptr(counts), cap) != 0:
            raise Y2Error("y2_detect_resident: " + _check())
        return [dets[b, :min(int(counts[b]), cap)].copy() for b in range(self.net.batch)], counts

    def output_enqueue(self) -> None:
        L = lib()
        L.y2_output_enqueue.argtypes = [CNetwork]
        if L.y2_output_enqueue(self.net) != 0:
            raise Y2Error("y2_output_enqueue: " + _check())

    def output_fetch(self) -> np.ndarray:
        L = lib()
        L.y2_output_fetch.argtypes = [CNetwork]
        L.y2_output_fetch.restype = C.POINTER(C.c_float)
        p = L.y2_output_fetch(self.net)
        if not p:
            raise Y2Error("y2_output_fetch: " + _check())
        return np.ctypeslib.as_array(p, shape=(self.net.batch * self.output_size,)).copy()

    def detect_enqueue(self, thresh: float, nms: float, img_w: int = 1, img_h: int = 1) -> None:
        """first half of detect_resident: decode + NMS + compaction + D2H enqueued, no wait (y2_detect_enqueue)"""
        L = lib()
        L.y2_detect_enqueue.argtypes = [CNetwork, C.c_float, C.c_float, C.c_int, C.c_int]
        if L.y2_detect_enqueue(self.net, thresh, nms, img_w, img_h) != 0:
            raise Y2Error("y2_detect_enqueue: " + _check())

    def detect_fetch(self, max_per_image: int | None = None):
        """second half: wait for the enqueued detections only and unpack them (y2_detect_fetch)"""
        l = self.last
        cap = max_per_image or (l.w * l.h * l.n)
        dets = np.zeros((self.net.batch, cap), dtype=DET_DTYPE)
        counts = np.zeros(self.net.batch, dtype=np.int32)
        L = lib()
        L.y2_detect_fetch.argtypes = [CNetwork, C.c_void_p, C.c_void_p, C.c_int]
        if L.y2_detect_fetch(self.net, _ptr(dets), _ptr(counts), cap) != 0:
            raise Y2Error("y2_detect_fetch: " + _check())
        return [dets[b, :min(int(counts[b]), cap)].copy() for b in range(self.net.batch)], counts

    def detect_mean(self, thresh: float, nms: float, img_w: int = 1, img_h: int = 1):
        """decode + NMS of the average of the last three forwards (Detector use_mean, y2_detect_mean); batch 1"""
        l = self.last
        cap = l.w * l.h * l.n
        dets = np.zeros((1, cap), dtype=DET_DTYPE)
        counts = np.zeros(1, dtype=np.int32)
        L = lib()
        L.y2_detect_mean.argtypes = [CNetwork, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        if L.y2_detect_mean(self.net, thresh, nms, img_w, img_h, _ptr(dets), _ptr(counts), cap) != 0:
            raise Y2Error("y2_detect_mean: " + _check())
        return dets[0, :min(int(counts[0]), cap)].copy(), int(counts[0])

    def detect(self, x: np.ndarray, thresh: float, nms: float, img_w: int = 1, img_h: int = 1):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        l = self.last
        cap = l.w * l.h * l.n
        dets = np.zeros((self.net.batch, cap), dtype=DET_DTYPE)
        counts = np.zeros(self.net.batch, dtype=np.int32)
        if lib().y2_detect(self.net, _ptr(x), thresh, nms, img_w, img_h, _ptr(dets), _ptr(counts), cap) != 0:
            raise Y2Error("y2_detect: " + _check())
        return [dets[b, :min(int(counts[b]), cap)].copy() for b in range(self.net.batch)], counts

    def detect_u8(self, frames: np.ndarray, thresh: float, nms: float, swap_rb: bool = True, letterbox: bool = False,
                  img_w: int = 1, img_h: int = 1):
        """frames: [batch][h][w][c] uint8 camera frames of any size (y2_detect_u8)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        b, h, w, c = frames.shape
        if b != self.net.batch:
            raise Y2Error("detect_u8: %d frames for a batch-%d network" % (b, self.net.batch))
        l = self.last
        cap = l.w * l.h * l.n
        dets = np.zeros((self.net.batch, cap), dtype=DET_DTYPE)
        counts = np.zeros(self.net.batch, dtype=np.int32)
        if lib().y2_detect_u8(self.net, _ptr(frames), h, w, c, w * c, int(swap_rb), int(letterbox), thresh, nms,
                              img_w, img_h, _ptr(dets), _ptr(counts), cap) != 0:
            raise Y2Error("y2_detect_u8: " + _check())
        return [dets[i, :min(int(counts[i]), cap)].copy() for i in range(self.net.batch)], counts

    def ingest_u8(self, frames: np.ndarray, swap_rb: bool = True, letterbox: bool = False) -> None:
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        b, h, w, c = frames.shape
        if b != self.net.batch:
            raise Y2Error("ingest_u8: %d frames for a batch-%d network" % (b, self.net.batch))
        if lib().y2_ingest_u8(self.net, _ptr(frames), h, w, c, w * c, int(swap_rb), int(letterbox)) != 0:
            raise Y2Error("y2_ingest_u8: " + _check())

    def ingest_regions(self, items, swap_rb: bool = True, letterbox: bool = False) -> None:
        """y2_ingest_regions: items = [(frame uint8 [h][w][c], (x, y, rw, rh) | None)], one per batch slot from 0"""
        arr, keep = regions(items)
        if lib().y2_ingest_regions(self.net, arr, len(items), int(swap_rb), int(letterbox)) != 0:
            raise Y2Error(_check())

    def detect_regions(self, items, thresh: float, nms: float, swap_rb: bool = True, letterbox: bool = False,
                       max_per_item: int | None = None):
        """y2_detect_regions: one forward pass over the items; ([dets of item i], counts[n]) with boxes relative to
        each item's frame"""
        arr, keep = regions(items)
        n = len(items)
        l = self.last
        cap = max_per_item or l.w * l.h * l.n
        dets = np.zeros((max(n, 1), cap), dtype=DET_DTYPE)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        if lib().y2_detect_regions(self.net, arr, n, int(swap_rb), int(letterbox), thresh, nms, _ptr(dets), _ptr(counts),
                                   cap) != 0:
            raise Y2Error(_check())
        return [dets[i, :min(int(counts[i]), cap)].copy() for i in range(n)], counts[:n]

    # --- the KCF trackers of the Kinect loop (include/sr_yolo2.h y2_kcf_*) ---
    def kcf_init(self, frame, boxes) -> None:
        """y2_kcf_init: frame uint8 [h][w] / [h][w][3] BGR / [h][w][4] BGRA, boxes [n][4] = (cx, cy, w, h) in pixels"""
        f, h, w, c, step = _kcf_frame(frame)
        b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
        if lib().y2_kcf_init(self.net, f.ctypes.data_as(C.c_void_p), h, w, c, step, _ptr(b), len(b)) != 0:
            raise Y2Error(_check())
        self._kcf_geo = [kcf_plan(row) for row in b]

    def kcf_track(self, frame, update: bool = False):
        """y2_kcf_track -> (boxes float64 [n][4], peaks float32 [n]); update=False is the application's copy-and-drop call"""
        f, h, w, c, step = _kcf_frame(frame)
        n = lib().y2_kcf_count(self.net)
        boxes, peaks = np.zeros((max(n, 1), 4), np.float64), np.zeros(max(n, 1), np.float32)
        if lib().y2_kcf_track(self.net, f.ctypes.data_as(C.c_void_p), h, w, c, step, int(bool(update)), _ptr(boxes), _ptr(peaks)) != 0:
            raise Y2Error(_check())
        return boxes[:n], peaks[:n]

    def kcf_count(self) -> int:
        return int(lib().y2_kcf_count(self.net))

    def kcf_fetch(self, i: int, what: int) -> np.ndarray:
        """y2_kcf_fetch: PATCH [win_h][win_w], FEATURES [31][R][C], XF [31][2][R][C], ALPHAF [2][R][C], RESPONSE [R][C]"""
        geo = getattr(self, "_kcf_geo", [])
        if not 0 <= i < len(geo):
            raise Y2Error("kcf_fetch: tracker %d of %d (kcf_init first)" % (i, len(geo)))
        g = geo[i]
        R, Cc = g["cells_h"], g["cells_w"]
        shape = {KCF_PATCH: (g["win_h"], g["win_w"]), KCF_FEATURES: (KCF_CHANNELS, R, Cc), KCF_XF: (KCF_CHANNELS, 2, R, Cc),
                 KCF_ALPHAF: (2, R, Cc), KCF_RESPONSE: (R, Cc)}.get(what)
        if shape is None:
            raise Y2Error("kcf_fetch: unknown tensor %d" % what)
        out = np.zeros(shape, np.float32)
        if lib().y2_kcf_fetch(self.net, i, what, _ptr(out), out.size) != 0:
            raise Y2Error(_check())
        return out

    def kcf_dft(self, a, inverse: bool = False) -> np.ndarray:
        """y2_kcf_dft: forward float32 [R][C] -> [2][R][C]; inverse [2][R][C] -> the real part [R][C] / (R*C)"""
        a = np.ascontiguousarray(a, dtype=np.float32)
        R, Cc = a.shape[-2:]
        out = np.zeros((R, Cc) if inverse else (2, R, Cc), np.float32)
        if lib().y2_kcf_dft(self.net, _ptr(a), R, Cc, int(bool(inverse)), _ptr(out)) != 0:
            raise Y2Error(_check())
        return out

    def kcf_init_objects(self, frame, objs) -> None:
        """y2_kcf_init_objects: objs is a ctypes array of Object, boxes relative to the frame"""
        f, h, w, c, step = _kcf_frame(frame)
        lib().y2_kcf_init_objects(self.net, f.ctypes.data_as(C.c_void_p), h, w, c, step, objs, len(objs))
        if lib().y2_failed_and_clear():
            raise Y2Error(_check())
        self._kcf_geo = [kcf_plan((float(np.float32(o.x) * np.float32(w)), float(np.float32(o.y) * np.float32(h)),
                                   float(np.float32(o.w) * np.float32(w)), float(np.float32(o.h) * np.float32(h)))) for o in objs]

    def kcf_track_objects(self, frame, objs) -> int:
        """y2_kcf_track_objects: fills objs (a ctypes array of Object with room for every tracker) -> the tracker count"""
        f, h, w, c, step = _kcf_frame(frame)
        n = C.c_int(0)
        lib().y2_kcf_track_objects(self.net, f.ctypes.data_as(C.c_void_p), h, w, c, step, objs, C.byref(n))
        if lib().y2_failed_and_clear():
            raise Y2Error(_check())
        return n.value

    def kcf_free(self) -> None:
        lib().y2_kcf_free(self.net)
        self._kcf_geo = []

    # --- the depth stage of the Kinect loop (include/sr_yolo2.h y2_depth_*) ---
    def depth_upload(self, depth, body=None, map_=None, color_hw=None) -> None:
        """y2_depth_upload: depth uint16 [dh][dw], body uint8 [dh][dw] | None, map_ float32 [H][W][2] | None (then the
        depth frame is already registered and H x W = dh x dw)"""
        depth = np.ascontiguousarray(depth, dtype=np.uint16)
        dh, dw = depth.shape
        body = np.ascontiguousarray(body, dtype=np.uint8) if body is not None else None
        if body is not None and body.shape != depth.shape:
            raise ValueError("the body-index frame has the depth frame's size")
        map_ = np.ascontiguousarray(map_, dtype=np.float32) if map_ is not None else None
        H, W = map_.shape[:2] if map_ is not None else (color_hw or (dh, dw))
        f = DepthFrame(depth.ctypes.data, body.ctypes.data if body is not None else None,
                       map_.ctypes.data if map_ is not None else None, dh, dw, H, W)
        if lib().y2_depth_upload(self.net, C.byref(f)) != 0:
            raise Y2Error(_check())
        self._depth_hw = (H, W)

    def depth_set_camera_table(self, table) -> None:
        """y2_depth_set_camera_table: float32 [dh][dw][2] (GetDepthFrameToCameraSpaceTable), or None to drop it"""
        if table is None:
            rc = lib().y2_depth_set_camera_table(self.net, None, 0, 0)
        else:
            t = np.ascontiguousarray(table, dtype=np.float32)
            rc = lib().y2_depth_set_camera_table(self.net, _ptr(t), t.shape[0], t.shape[1])
        if rc != 0:
            raise Y2Error(_check())

    def depth_aligned(self):
        """y2_depth_aligned -> (depth16 [H][W] uint16, depth8 [H][W] uint8, person [H][W] uint8)"""
        H, W = getattr(self, "_depth_hw", (0, 0))
        if H * W == 0:
            raise Y2Error("depth_aligned: no depth frame has been uploaded")
        d16, d8, per = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        if lib().y2_depth_aligned(self.net, _ptr(d16), _ptr(d8), _ptr(per)) != 0:
            raise Y2Error(_check())
        return d16, d8, per

    # --- the Grasp branch: the table plane removed behind depth_upload (include/sr_yolo2.h y2_plane_*) ---
    def depth_set_plane_removal(self, far_m: float = 1.0, dist_m: float = 0.02, iters: int = 50, seed: int = 1,
                                samples=None) -> None:
        """y2_depth_set_plane_removal; iters <= 0 turns it off.  samples: int32 [iters][3] depth-pixel indices, or None"""
        smp = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3) if samples is not None else None
        if smp is not None and len(smp) != iters:
            raise ValueError("samples needs one triple per hypothesis")
        o = PlaneOpts(far_m, dist_m, iters, seed & 0xFFFFFFFF, smp.ctypes.data if smp is not None else None)
        if lib().y2_depth_set_plane_removal(self.net, C.byref(o) if iters > 0 else None) != 0:
            raise Y2Error(_check())

    def depth_plane(self) -> dict:
        """y2_depth_plane -> dict of the fields of y2_plane"""
        p = Plane()
        if lib().y2_depth_plane(self.net, C.byref(p)) != 0:
            raise Y2Error(_check())
        return {k: getattr(p, k) for k, _ in Plane._fields_}

    def depth_grasp_aligned(self, dhw):
        """y2_depth_grasp_aligned -> (grasp_depth [dh][dw] uint16, grasp16 [H][W] uint16); dhw = the depth frame's shape"""
        H, W = getattr(self, "_depth_hw", (0, 0))
        if H * W == 0:
            raise Y2Error("depth_grasp_aligned: no depth frame has been uploaded")
        gd, g16 = np.zeros(tuple(dhw), np.uint16), np.zeros((H, W), np.uint16)
        if lib().y2_depth_grasp_aligned(self.net, _ptr(gd), _ptr(g16)) != 0:
            raise Y2Error(_check())
        return gd, g16

    def depth_set_event(self, event: int) -> None:
        """y2_depth_set_event: EVENT_DEMO_WHAT or EVENT_GRASP"""
        if lib().y2_depth_set_event(self.net, event) != 0:
            raise Y2Error(_check())

    def depth_set_grasp_filter(self, on: bool) -> None:
        if lib().y2_depth_set_grasp_filter(self.net, int(on)) != 0:
            raise Y2Error(_check())

    def depth_boxes(self, boxes) -> np.ndarray:
        """y2_depth_boxes: frame-relative (x, y, w, h) boxes [n][4] -> DET3D_DTYPE [n]"""
        b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        out = np.zeros(max(len(b), 1), dtype=DET3D_DTYPE)
        if lib().y2_depth_boxes(self.net, _ptr(b), len(b), _ptr(out)) != 0:
            raise Y2Error(_check())
        return out[:len(b)]

    def ingest_regions_depth(self, items, far_m, swap_rb: bool = True, letterbox: bool = False) -> None:
        """y2_ingest_regions_depth: ingest_regions with the hand-crop distance filter on the items whose far_m is > 0"""
        arr, keep = regions(items)
        far = np.ascontiguousarray(far_m, dtype=np.float32)
        if len(far) != len(items):
            raise ValueError("far_m needs one value per item")
        if lib().y2_ingest_regions_depth(self.net, arr, len(items), _ptr(far), int(swap_rb), int(letterbox)) != 0:
            raise Y2Error(_check())

    def detect_regions_depth(self, items, far_m, thresh: float, nms: float, swap_rb: bool = True, letterbox: bool = False,
                             max_per_item: int | None = None):
        """y2_detect_regions_depth -> ([dets of item i], [DET3D_DTYPE of item i], counts[n]); far_m None: no filter"""
        arr, keep = regions(items)
        n = len(items)
        far = np.ascontiguousarray(far_m, dtype=np.float32) if far_m is not None else None
        if far is not None and len(far) != n:
            raise ValueError("far_m needs one value per item")
        l = self.last
        cap = max_per_item or l.w * l.h * l.n
        dets = np.zeros((max(n, 1), cap), dtype=DET_DTYPE)
        d3 = np.zeros((max(n, 1), cap), dtype=DET3D_DTYPE)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        if lib().y2_detect_regions_depth(self.net, arr, n, _ptr(far) if far is not None else None, int(swap_rb), int(letterbox),
                                         thresh, nms, _ptr(dets), _ptr(d3), _ptr(counts), cap) != 0:
            raise Y2Error(_check())
        keep_n = [min(int(counts[i]), cap) for i in range(n)]
        return [dets[i, :keep_n[i]].copy() for i in range(n)], [d3[i, :keep_n[i]].copy() for i in range(n)], counts[:n]

    def validate_detector_frames(self, frames: np.ndarray, paths, orig_w, orig_h, prefix: str, eval: str = "voc",
                                 names=None, map_: np.ndarray | None = None) -> None:
        """validate_detector (detector.c:245) over in-memory network-sized frames [n][c][h][w]."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n = frames.shape[0]
        ow = np.ascontiguousarray(orig_w, dtype=np.int32)
        oh = np.ascontiguousarray(orig_h, dtype=np.int32)
        cpaths = (C.c_char_p * n)(*[p.encode() for p in paths])
        cnames = (C.c_char_p * len(names))(*[s.encode() for s in names]) if names else None
        mp = np.ascontiguousarray(map_, dtype=np.int32) if map_ is not None else None
        if lib().y2_validate_detector_frames(self.net, _ptr(frames), n, cpaths, _ptr(ow), _ptr(oh), eval.encode(),
                                             prefix.encode(), cnames, _ptr(mp) if mp is not None else None) != 0:
            raise Y2Error("y2_validate_detector_frames: " + _check())

    def validate_recall_frames(self, frames: np.ndarray, truth_per_frame) -> dict:
        """validate_detector_recall (detector.c:371): truth_per_frame = list of [k][4] relative centre-form boxes."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n = frames.shape[0]
        first = np.zeros(n + 1, np.int32)
        first[1:] = np.cumsum([len(t) for t in truth_per_frame])
        truth = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32).reshape(-1, 4) for t in truth_per_frame] or
                                                    [np.zeros((0, 4), np.float32)]), dtype=np.float32)
        if truth.size == 0:
            truth = np.zeros((1, 4), np.float32)
        res = Recall()
        if lib().y2_validate_recall_frames(self.net, _ptr(frames), n, _ptr(truth), _ptr(first), C.byref(res)) != 0:
            raise Y2Error("y2_validate_recall_frames: " + _check())
        return dict(total=res.total, correct=res.correct, proposals=res.proposals, avg_iou=res.avg_iou)

    def validate_classifier_frames(self, frames: np.ndarray, truth, classes: int, topk: int):
        """validate_classifier_single (classifier.c:469) over in-memory frames -> (top-1 accuracy, top-k accuracy)."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        truth = np.ascontiguousarray(truth, dtype=np.int32)
        a, b = C.c_float(), C.c_float()
        L = lib()
        L.y2_validate_classifier_frames.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                    C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if L.y2_validate_classifier_frames(self.net, _ptr(frames), frames.shape[0], _ptr(truth), classes, topk,
                                           C.byref(a), C.byref(b)) != 0:
            raise Y2Error("y2_validate_classifier_frames: " + _check())
        return a.value, b.value

    def classify(self, frames: np.ndarray, top: int):
        """predict_classifier's core (classifier.c:716-718) over network-sized frames [n][c][h][w]: forward, with a
        hierarchy hierarchy_predictions(.., 0) on the device, top_k over all outputs -> (indexes [n][top], probs [n][top])."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n = frames.shape[0]
        idx = np.zeros((n, top), dtype=np.int32)
        probs = np.zeros((n, top), dtype=np.float32)
        if lib().y2_classify_frames(self.net, _ptr(frames), n, top, _ptr(idx), _ptr(probs)) != 0:
            raise Y2Error(_check())
        return idx, probs

    def hierarchy_enqueue(self, only_leaves: bool = False) -> None:
        """hierarchy_predictions (tree.c:37) on the output rows of the last forward, in HBM, before output_enqueue /
        output_fetch; the leaf flags are read from net.hierarchy at the call.  In place: once per forward"""
        if lib().y2_hierarchy_enqueue(self.net, 1 if only_leaves else 0) != 0:
            raise Y2Error(_check())

    @property
    def hierarchy(self):
        """net.hierarchy (a POINTER(Tree); false when the network has none)"""
        return self.net.hierarchy

    # --- the reference's multi-view classifier evaluations (classifier.c:336-593; include/sr_yolo2.h Y2_VIEWS_*) ---
    def classifier_view_sums(self, mode: int, frames, scales=None) -> np.ndarray:
        """summed predictions [n][outputs] of every frame's views: VIEWS_CROP10 (valid10: ten crops of the frame at
        net size + 32), VIEWS_MULTI (validmulti: whole image and mirror image at each scale, the network resized) or
        VIEWS_FULL (validfull); frames: float32 [c][h][w] arrays of any size."""
        arr, keep = images(frames)
        sc = np.ascontiguousarray(scales, dtype=np.int32) if scales is not None else None
        sums = np.zeros((len(keep), self.output_size), dtype=np.float32)
        if lib().y2_classifier_view_sums(C.byref(self.net), mode, arr, len(keep), _ptr(sc) if sc is not None else None,
                                         sc.size if sc is not None else 0, _ptr(sums)) != 0:
            raise Y2Error(_check())
        return sums

    def _validate_views(self, fn, net_arg, frames, truth, classes: int, topk: int, scales=None, with_scales=False):
        arr, keep = images(frames)
        truth = np.ascontiguousarray(truth, dtype=np.int32)
        a, b = C.c_float(), C.c_float()
        args = [net_arg, arr, len(keep)]
        if with_scales:
            sc = np.ascontiguousarray(scales, dtype=np.int32) if scales is not None else None
            args += [_ptr(sc) if sc is not None else None, sc.size if sc is not None else 0]
        if fn(*args, _ptr(truth), classes, topk, C.byref(a), C.byref(b)) != 0:
            raise Y2Error(_check())
        return a.value, b.value

    def validate_classifier_10(self, frames, truth, classes: int, topk: int):
        """validate_classifier_10 (classifier.c:336) over in-memory frames -> (top-1 accuracy, top-k accuracy)"""
        return self._validate_views(lib().y2_validate_classifier_10_frames, self.net, frames, truth, classes, topk)

    def validate_classifier_multi(self, frames, truth, classes: int, topk: int, scales=None):
        """validate_classifier_multi (classifier.c:531); scales=None: 224, 288, 320, 352, 384"""
        return self._validate_views(lib().y2_validate_classifier_multi_frames, C.byref(self.net), frames, truth, classes, topk,
                                    scales, True)

    def validate_classifier_full(self, frames, truth, classes: int, topk: int):
        """validate_classifier_full (classifier.c:408)"""
        return self._validate_views(lib().y2_validate_classifier_full_frames, C.byref(self.net), frames, truth, classes, topk)

    def pull_layer_output(self, i: int) -> np.ndarray:
        l = self.net.layers[i]
        out = np.zeros(self.net.batch * l.outputs, dtype=np.float32)
        if lib().y2_pull_layer_output(self.net, i, _ptr(out)) != 0:
            raise Y2Error("y2_pull_layer_output: " + _check())
        return out

    # --- text generation and scoring (rnn.c; include/sr_yolo2.h y2_rnn_*) ---
    @property
    def sequences(self) -> int:
        """B: sequences per forward of a recurrent network (net.batch / time_steps)"""
        return self.net.batch // max(self.net.time_steps, 1)

    @staticmethod
    def rnn_uniforms(rseed: int, n: int) -> np.ndarray:
        """srand(rseed), then n values of rand_uniform(0, 1) (utils.c:603): the reference's stream on libc rand"""
        u = np.zeros(n, dtype=np.float32)
        if lib().y2_rnn_uniforms(int(rseed), int(n), _ptr(u)) != 0:
            raise Y2Error("y2_rnn_uniforms: " + _check())
        return u

    def rnn_generate(self, seed, num: int, uniforms, probs: bool = False):
        """num characters per sequence, sampled on the device (test_char_rnn's loop, rnn.c:257-278): seed is [len][B] (or
        [len] for one sequence; empty: token 0), uniforms [num][B].  Returns tokens [num][B], and with probs=True also the
        rows each draw sampled from, [num][B][outputs].  Goes on from the network's current state and temperature."""
        B = self.sequences
        seed = np.ascontiguousarray(seed, dtype=np.int32).reshape(-1, B)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if u.size != num * B:
            raise ValueError("uniforms has %d values, %d draws x %d sequences need %d" % (u.size, num, B, num * B))
        tokens = np.zeros((num, B), dtype=np.int32)
        rows = np.zeros((num, B, self.output_size), dtype=np.float32) if probs else None
        L = lib()
        L.y2_rnn_generate.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if L.y2_rnn_generate(self.net, _ptr(seed), seed.shape[0], num, _ptr(u), _ptr(tokens), _ptr(rows) if probs else None) != 0:
            raise Y2Error("y2_rnn_generate: " + _check())
        return (tokens, rows) if probs else tokens

    def rnn_score(self, tokens, probs: bool = False):
        """teacher-forced scoring of tokens [n][B] (or [n]): p_next [n-1][B], the probability given to the character that
        followed; with probs=True also the rows, [n-1][B][outputs].  n-1 must be a multiple of time_steps."""
        B = self.sequences
        tokens = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1, B)
        n = tokens.shape[0]
        p = np.zeros((max(n - 1, 0), B), dtype=np.float32)
        rows = np.zeros((max(n - 1, 0), B, self.output_size), dtype=np.float32) if probs else None
        L = lib()
        L.y2_rnn_score.argtypes = [CNetwork, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if L.y2_rnn_score(self.net, _ptr(tokens), n, _ptr(p), _ptr(rows) if probs else None) != 0:
            raise Y2Error("y2_rnn_score: " + _check())
        return (p, rows) if probs else p

    @staticmethod
    def rnn_perplexity(p_next, text: bytes):
        """valid_char_rnn's books (rnn.c:402-416) -> (perplexity, word perplexity) of a text and its len-1 scores"""
        p = np.ascontiguousarray(p_next, dtype=np.float32).reshape(-1)
        if p.size != len(text) - 1:
            raise ValueError("%d scores for a text of %d characters" % (p.size, len(text)))
        a, b = C.c_float(), C.c_float()
        L = lib()
        L.y2_rnn_perplexity.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if L.y2_rnn_perplexity(_ptr(p), bytes(text), len(text), C.byref(a), C.byref(b)) != 0:
            raise Y2Error("y2_rnn_perplexity: " + _check())
        return a.value, b.value

    # --- Go (go.c; include/sr_yolo2.h y2_go_*) ---
    def predict_move(self, board, multi: bool = False) -> np.ndarray:
        """go.c:262 on one board [361] as the mover sees it -> move [361]"""
        b = _go_boards(board, 1).copy()
        move = np.zeros(GO_POINTS, np.float32)
        lib().predict_move(self.net, _ptr(b), _ptr(move), int(multi))
        if lib().y2_failed_and_clear():
            raise Y2Error("predict_move: " + _check())
        return move

    def generate_move(self, player: int, board, multi: bool, thresh: float, temp: float, ko: bytes) -> int:
        """go.c:351: one libc rand() draw, then the point or -1"""
        b = _go_boards(board, 1).copy()
        k = np.frombuffer(_go_ko(ko, 1), np.uint8).copy()
        r = lib().generate_move(self.net, int(player), _ptr(b), int(multi), thresh, temp, _ptr(k), 0)
        if r < 0 and lib().y2_failed_and_clear():
            raise Y2Error("generate_move: " + _check())
        return int(r)

    def go_predict(self, boards, players, multi: bool = False) -> np.ndarray:
        """y2_go_predict: boards [n][361] (absolute), players [n] -> moves [n][361]"""
        p = np.ascontiguousarray(players, dtype=np.int32).reshape(-1)
        b = _go_boards(boards, p.size)
        out = np.zeros((p.size, GO_POINTS), np.float32)
        if lib().y2_go_predict(self.net, _ptr(b), _ptr(p), p.size, int(multi), _ptr(out)) != 0:
            raise Y2Error("y2_go_predict: " + _check())
        return out

    def go_rules(self, boards, ko, players):
        """y2_go_rules -> (liberties int32 [n][361], legal uint8 [n][361], suicide uint8 [n][361])"""
        p = np.ascontiguousarray(players, dtype=np.int32).reshape(-1)
        n = p.size
        b = _go_boards(boards, n)
        k = np.frombuffer(_go_ko(ko, n), np.uint8)
        lib_, legal, sui = np.zeros((n, GO_POINTS), np.int32), np.zeros((n, GO_POINTS), np.uint8), np.zeros((n, GO_POINTS), np.uint8)
        if lib().y2_go_rules(self.net, _ptr(b), _ptr(k), _ptr(p), n, _ptr(lib_), _ptr(legal), _ptr(sui)) != 0:
            raise Y2Error("y2_go_rules: " + _check())
        return lib_, legal, sui

    def go_generate(self, boards, ko, players, multi: bool, thresh: float, temp: float, uniforms, kept: bool = False):
        """y2_go_generate: one chain and one sync for n positions -> index int32 [n] (and the thresholded arrays)"""
        p = np.ascontiguousarray(players, dtype=np.int32).reshape(-1)
        n = p.size
        b = _go_boards(boards, n)
        k = np.frombuffer(_go_ko(ko, n), np.uint8)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if u.size != n:
            raise ValueError("go_generate: %d uniforms for %d positions" % (u.size, n))
        index = np.zeros(n, np.int32)
        rows = np.zeros((n, GO_POINTS), np.float32) if kept else None
        if lib().y2_go_generate(self.net, _ptr(b), _ptr(k), _ptr(p), n, int(multi), thresh, temp, _ptr(u), _ptr(index),
                                _ptr(rows) if kept else None) != 0:
            raise Y2Error("y2_go_generate: " + _check())
        return (index, rows) if kept else index

    def go_valid(self, records, multi: bool = False) -> np.ndarray:
        """y2_go_valid: records uint8 [n][93] -> predicted point per record"""
        r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, GO_RECORD)
        out = np.zeros(r.shape[0], np.int32)
        if lib().y2_go_valid(self.net, _ptr(r), r.shape[0], int(multi), _ptr(out)) != 0:
            raise Y2Error("y2_go_valid: " + _check())
        return out

    def go_selfplay(self, games: int, max_moves: int, uniforms, multi: bool = False, thresh: float = .1, temp: float = .7,
                    other: "Network | None" = None, first: int = 0):
        """y2_go_selfplay -> (records uint8 [games][max_moves][93], counts int32 [games], final boards [games][361])"""
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if u.size != max(games, 0) * max(max_moves, 0):
            raise ValueError("go_selfplay: %d uniforms for %d games x %d moves" % (u.size, games, max_moves))
        rec = np.zeros((max(games, 1), max(max_moves, 1), GO_RECORD), np.uint8)
        counts = np.zeros(max(games, 1), np.int32)
        boards = np.zeros((max(games, 1), GO_POINTS), np.float32)
        if lib().y2_go_selfplay(self.net, (other or self).net, games, first, max_moves, int(multi), thresh, temp, _ptr(u), _ptr(rec),
                                _ptr(counts), _ptr(boards)) != 0:
            raise Y2Error("y2_go_selfplay: " + _check())
        return rec, counts, boards

    def go_set_poll(self, every: int) -> None:
        if lib().y2_go_set_poll(self.net, int(every)) != 0:
            raise Y2Error("y2_go_set_poll: " + _check())

    def train_load_go(self, records, pick, flip, rot) -> None:
        """y2_train_load_go: records uint8 [n][93] and the draws of go_draw_moves -> the trainer's input and truth"""
        r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, GO_RECORD)
        d = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (pick, flip, rot)]
        if any(a.size != self.net.batch for a in d):
            raise ValueError("train_load_go: pick, flip and rot need net.batch = %d values each" % self.net.batch)
        if lib().y2_train_load_go(C.byref(self.net), _ptr(r), r.shape[0], _ptr(d[0]), _ptr(d[1]), _ptr(d[2])) != 0:
            raise Y2Error("y2_train_load_go: " + _check())

    def sync(self) -> None:
        lib().y2_sync(self.net)

    def stream(self) -> int:
        return lib().y2_stream(self.net) or 0

    def free(self) -> None:
        if not self._freed:
            lib().free_network(self.net)
            self._freed = True

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Dream:
    """A dream context (include/sr_yolo2.h y2_dream): the picture in HBM, the packed weights, the buffers per input size.
    Close it before the network is freed."""
    ARRAYS = ("output", "delta", "input", "gradient", "update")

    def __init__(self, net: Network, picture: np.ndarray):
        p = np.ascontiguousarray(picture, dtype=np.float32)
        if p.ndim != 3:
            raise ValueError("picture must be [c][h][w]")
        self.net, self.shape = net, p.shape
        self.h = lib().y2_dream_open(C.byref(net.net), _ptr(p), p.shape[0], p.shape[1], p.shape[2])
        if not self.h:
            raise Y2Error("y2_dream_open: " + _check())

    def step(self, max_layer: int, scale: float = 1.0, rate: float = .04, thresh: float = 1.0, norm: int = 1, dx: int = 0, dy: int = 0,
             flip: int = 0) -> None:
        if lib().y2_dream_step(self.h, max_layer, scale, rate, thresh, norm, dx, dy, flip) != 0:
            raise Y2Error("y2_dream_step: " + _check())

    def round_end(self, rotate: float = 0.0, zoom: float = 1.0) -> None:
        if lib().y2_dream_round_end(self.h, rotate, zoom) != 0:
            raise Y2Error("y2_dream_round_end: " + _check())

    def fetch(self) -> np.ndarray:
        out = np.zeros(self.shape, np.float32)
        if lib().y2_dream_fetch(self.h, _ptr(out)) != 0:
            raise Y2Error("y2_dream_fetch: " + _check())
        return out

    def stats(self) -> dict:
        st = DreamCounters()
        if lib().y2_dream_stats(self.h, C.byref(st)) != 0:
            raise Y2Error("y2_dream_stats: " + _check())
        return {k: int(getattr(st, k)) for k, _ in DreamCounters._fields_}

    def pull(self, what: str, layer: int = 0, shape=None) -> np.ndarray:
        """of the last step: "output" / "delta" of a layer, the "input" it built and the image "gradient" ([c][h][w] at the
        step's size), the picture-sized "update" before normalisation; shape = (c, h, w) of the array"""
        shape = tuple(shape) if shape is not None else self.shape
        out = np.zeros(shape, np.float32)
        if lib().y2_dream_pull(self.h, layer, self.ARRAYS.index(what), _ptr(out), out.size) != 0:
            raise Y2Error("y2_dream_pull: " + _check())
        return out

    def close(self) -> None:
        if self.h:
            lib().y2_dream_close(self.h)
            self.h = None

    def __del__(self):
        try:
            if not self.net._freed:
                self.close()
        except Exception:
            pass


def srand(seed: int) -> None:
    """libc's srand: the generator y2_dream_draw, optimize_picture and y2_nightmare draw from"""
    C.CDLL(None).srand(C.c_uint(seed))


# --- Go: the device-free half of go.c ---
GO_POINTS, GO_KO, GO_RECORD, GO_LINE = 361, 91, 93, 94


class GoMoves(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_void_p)), ("n", C.c_int)]


def _go_boards(boards, n: int) -> np.ndarray:
    b = np.ascontiguousarray(boards, dtype=np.float32).reshape(-1)
    if b.size != n * GO_POINTS:
        raise ValueError("%d board values for %d positions" % (b.size, n))
    return b


def _go_ko(ko, n: int) -> bytes:
    k = bytes(n * GO_KO) if ko is None else (ko if isinstance(ko, (bytes, bytearray)) else np.ascontiguousarray(ko, dtype=np.uint8).tobytes())
    if len(k) != n * GO_KO:
        raise ValueError("%d ko bytes for %d positions" % (len(k), n))
    return bytes(k)


def string_to_board(s) -> np.ndarray:
    k = np.frombuffer(_go_ko(s, 1), np.uint8).copy()
    board = np.zeros(GO_POINTS, np.float32)
    lib().string_to_board(_ptr(k), _ptr(board))
    return board


def board_to_string(board) -> bytes:
    b = _go_boards(board, 1)
    s = np.zeros(GO_KO, np.uint8)
    lib().board_to_string(_ptr(s), _ptr(b))
    return s.tobytes()


def calculate_liberties(board) -> np.ndarray:
    b = _go_boards(board, 1)
    L = lib()
    p = L.calculate_liberties(_ptr(b))
    out = np.ctypeslib.as_array(p, shape=(GO_POINTS,)).astype(np.int32)
    C.CDLL(None).free(C.cast(p, C.c_void_p))
    return out


def move_go(board, player: int, row: int, col: int) -> np.ndarray:
    """the board after the move (the argument is not changed)"""
    b = _go_boards(board, 1).copy()
    lib().move_go(_ptr(b), int(player), int(row), int(col))
    return b


def suicide_go(board, player: int, row: int, col: int) -> int:
    b = _go_boards(board, 1).copy()
    return int(lib().suicide_go(_ptr(b), int(player), int(row), int(col)))


def legal_go(board, ko, player: int, row: int, col: int) -> int:
    b = _go_boards(board, 1).copy()
    k = np.frombuffer(_go_ko(ko, 1), np.uint8).copy()
    return int(lib().legal_go(_ptr(b), _ptr(k), int(player), int(row), int(col)))


def load_go_moves(path: str) -> np.ndarray:
    """go.c:34 -> records uint8 [n][93] (the lines without their newline)"""
    L = lib()
    m = L.load_go_moves(path.encode())
    if L.y2_failed_and_clear():
        raise Y2Error("load_go_moves: " + _check())
    out = np.zeros((m.n, GO_RECORD), np.uint8)
    for i in range(m.n):
        out[i] = np.frombuffer(C.string_at(m.data[i], GO_RECORD), np.uint8)
    L.y2_go_free_moves(m)
    return out


def go_draw_moves(n_records: int, batch: int):
    """random_go_moves' draws for one batch, on libc rand: (pick, flip, rot), int32 [batch] each"""
    d = [np.zeros(max(batch, 1), np.int32) for _ in range(3)]
    if lib().y2_go_draw_moves(n_records, batch, _ptr(d[0]), _ptr(d[1]), _ptr(d[2])) != 0:
        raise Y2Error("y2_go_draw_moves: " + _check())
    return tuple(a[:batch] for a in d)


def dream_draw(range_: int = 1, octaves: int = 4) -> dict:
    """the five rand() calls of one run_nightmare iteration in its order"""
    d = DreamDraws()
    lib().y2_dream_draw(range_, octaves, C.byref(d))
    return {k: int(getattr(d, k)) for k, _ in DreamDraws._fields_}


def dream_scale(octave: int) -> float:
    return float(lib().y2_dream_scale(octave))


def dream_size(w: int, h: int, scale: float) -> tuple:
    ow, oh = C.c_int(), C.c_int()
    lib().y2_dream_size(w, h, scale, C.byref(ow), C.byref(oh))
    return ow.value, oh.value


def do_nms_sort(boxes: np.ndarray, probs: np.ndarray, thresh: float, classes: int | None = None) -> np.ndarray:
    """box.c:249 on host arrays (staged through the GPU kernel).  Returns the updated probs."""
    L = lib()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    probs = np.array(probs, dtype=np.float32, order="C", copy=True)
    L.do_nms_sort(_ptr(boxes), _rows(probs), probs.shape[0], classes or probs.shape[1], thresh)
    if L.y2_failed_and_clear():
        raise Y2Error("do_nms_sort: " + _check())
    return probs


def do_nms(boxes: np.ndarray, probs: np.ndarray, thresh: float) -> np.ndarray:
    L = lib()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    probs = np.array(probs, dtype=np.float32, order="C", copy=True)
    L.do_nms(_ptr(boxes), _rows(probs), probs.shape[0], probs.shape[1], thresh)
    if L.y2_failed_and_clear():
        raise Y2Error("do_nms: " + _check())
    return probs


def read_tree(path: str):
    """tree.c:53 -> POINTER(Tree)"""
    t = lib().read_tree(path.encode())
    if not t:
        raise Y2Error("read_tree: " + _check())
    return t


def hierarchy_predictions(predictions: np.ndarray, hier, only_leaves: bool = False) -> np.ndarray:
    """tree.c:37 on a host row (hier: POINTER(Tree), e.g. Network.hierarchy or read_tree's); returns the new row"""
    p = np.array(predictions, dtype=np.float32, order="C", copy=True)
    lib().hierarchy_predictions(_ptr(p), p.size, hier, 1 if only_leaves else 0)
    return p


def get_hierarchy_probability(x: np.ndarray, hier, c: int) -> float:
    """tree.c:27: x[c] times x of every ancestor of c"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return float(lib().get_hierarchy_probability(_ptr(x), hier, int(c)))


def change_leaves(hier, leaf_list: str) -> None:
    """tree.c:7: the tree's leaves become the names listed in the file, one per line"""
    L = lib()
    L.change_leaves(hier, leaf_list.encode())
    if L.y2_failed_and_clear():
        raise Y2Error("change_leaves: " + _check())


def box_iou(a, b) -> float:
    return float(lib().box_iou(Box(*[float(v) for v in a]), Box(*[float(v) for v in b])))


def resize_image(im: np.ndarray, w: int, h: int) -> np.ndarray:
    """image.c:1950 on the GPU: [c][ih][iw] -> [c][h][w]."""
    L = lib()
    im = np.ascontiguousarray(im, dtype=np.float32)
    c, ih, iw = im.shape
    out = L.resize_image(Image(ih, iw, c, im.ctypes.data_as(C.POINTER(C.c_float))), w, h)
    if L.y2_failed_and_clear():
        raise Y2Error("resize_image: " + _check())
    arr = np.ctypeslib.as_array(out.data, shape=(c, h, w)).copy()
    L.free_image(out)
    return arr


class _CFile:
    """FILE* from the C library, for the writers that take one (the reference's own signatures)."""
    _libc = None

    def __init__(self, path: str, mode: str = "w"):
        if _CFile._libc is None:
            _CFile._libc = C.CDLL(None)
            _CFile._libc.fopen.restype = C.c_void_p
            _CFile._libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
            _CFile._libc.fclose.argtypes = [C.c_void_p]
        self.fp = _CFile._libc.fopen(path.encode(), mode.encode())
        if not self.fp:
            raise OSError("cannot open " + path)

    def close(self):
        if self.fp:
            _CFile._libc.fclose(self.fp)
            self.fp = None


def write_detections(kind: str, paths, ident, boxes: np.ndarray, probs: np.ndarray, w: int, h: int) -> None:
    """The reference's evaluation writers (detector.c:175-243) through this library: kind 'voc'
    (print_detector_detections, one path per class), 'imagenet' (print_imagenet_detections), 'coco' (print_cocos)."""
    L = lib()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    total, classes = probs.shape
    rows = _rows(probs)
    files = [_CFile(p, "a") for p in paths]
    try:
        if kind == "voc":
            fps = (C.c_void_p * classes)(*[f.fp for f in files])
            L.print_detector_detections(fps, str(ident).encode(), _ptr(boxes), rows, total, classes, w, h)
        elif kind == "imagenet":
            L.print_imagenet_detections(files[0].fp, int(ident), _ptr(boxes), rows, total, classes, w, h)
        elif kind == "coco":
            L.print_cocos(files[0].fp, str(ident).encode(), _ptr(boxes), rows, total, classes, w, h)
        else:
            raise ValueError(kind)
    finally:
        for f in files:
            f.close()


def letterbox_image(im: np.ndarray, w: int, h: int, into: np.ndarray | None = None) -> np.ndarray:
    """image.c:1624 letterbox_image (into=None) / :1607 letterbox_image_into, on the GPU."""
    L = lib()
    im = np.ascontiguousarray(im, dtype=np.float32)
    c, ih, iw = im.shape
    src = Image(ih, iw, c, im.ctypes.data_as(C.POINTER(C.c_float)))
    if into is None:
        out = L.letterbox_image(src, w, h)
        failed = L.y2_failed_and_clear()
        arr = np.ctypeslib.as_array(out.data, shape=(c, h, w)).copy()
        L.free_image(out)
    else:
        arr = np.ascontiguousarray(into, dtype=np.float32).copy()
        L.letterbox_image_into(src, w, h, Image(h, w, c, arr.ctypes.data_as(C.POINTER(C.c_float))))
        failed = L.y2_failed_and_clear()
    if failed:
        raise Y2Error("letterbox_image: " + _check())
    return arr


BBOX_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("prob", "<f4"), ("obj_id", "<u4"), ("track_id", "<u4")])


class Detector:
    """The C++ Detector class (include/yolo_v2_class.hpp; reference yolo_v2_class.hpp:42-57) through its C face."""

    def __init__(self, cfg: str, weights: str = "", gpu: int = 0):
        lib().y2_set_error_mode(1)
        self.h = lib().y2_detector_create(cfg.encode(), weights.encode(), gpu)
        if not self.h:
            raise Y2Error("Detector: " + _check())
        self._out = np.zeros(4096, dtype=BBOX_DTYPE)

    def net_size(self):
        w, h = C.c_int(0), C.c_int(0)
        lib().y2_detector_net_size(C.c_void_p(self.h), C.byref(w), C.byref(h))
        return w.value, h.value

    def detect(self, chw: np.ndarray, thresh: float = 0.2, use_mean: bool = False, nms: float = -1.0, track: bool = False) -> np.ndarray:
        """Detector::detect(image_t) (+ tracking): structured array of bbox_t"""
        chw = np.ascontiguousarray(chw, dtype=np.float32)
        c, h, w = chw.shape
        n = lib().y2_detector_detect(C.c_void_p(self.h), _ptr(chw), c, h, w, thresh, int(use_mean), nms, int(track),
                                     _ptr(self._out), self._out.size)
        if n < 0:
            raise Y2Error("Detector.detect: " + _check())
        return self._out[:min(n, self._out.size)].copy()

    def free(self) -> None:
        if self.h:
            lib().y2_detector_destroy(C.c_void_p(self.h))
            self.h = None


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (rank 0 creates it and hands it to the other ranks)"""
    buf = C.create_string_buffer(128)
    if lib().y2_comm_unique_id(buf) != 0:
        raise Y2Error("y2_comm_unique_id: " + _check())
    return buf.raw


def comm_init_rank(nranks: int, uid: bytes, rank: int, device: int) -> int:
    comm = C.c_void_p()
    if len(uid) != 128:
        raise Y2Error("comm_init_rank: the unique id must be 128 bytes")
    if lib().y2_comm_init_rank(C.byref(comm), nranks, C.create_string_buffer(uid, 128), rank, device) != 0:
        raise Y2Error("y2_comm_init_rank: " + _check())
    return comm.value


def comm_count(comm: int):
    """(ranks, this rank) of an RCCL communicator, as ncclCommCount / ncclCommUserRank report them"""
    n, r = C.c_int(0), C.c_int(-1)
    if lib().y2_comm_count(C.c_void_p(comm), C.byref(n), C.byref(r)) != 0:
        raise Y2Error("y2_comm_count: " + _check())
    return n.value, r.value


def comm_destroy(comm: int) -> None:
    if lib().y2_comm_destroy(C.c_void_p(comm)) != 0:
        raise Y2Error("y2_comm_destroy: " + _check())


def comm_library() -> str:
    p = lib().y2_comm_library()
    if not p:
        raise Y2Error("y2_comm_library: " + _check())
    return p.decode()


def device_count() -> int:
    return int(lib().y2h_device_count())


def device_name() -> str:
    return lib().y2h_device_name().decode()


def clock_probe(iters: int = 8000) -> float:
    """GHz the current device holds under a full-chip fp32 matrix load (y2h_clock_probe)"""
    g = C.c_float(0)
    if lib().y2h_clock_probe(iters, C.byref(g), None) != 0:
        raise Y2Error("y2h_clock_probe: " + lib().y2h_last_error().decode())
    return float(g.value)


def device_pci_bus_id(dev: int = -1) -> str:
    """PCI address of a device ("0000:c1:00.0"; dev < 0: the current one); "" if the runtime will not say"""
    return lib().y2h_device_pci_bus_id(dev).decode()


def numa_cpus_of_device(dev: int = -1):
    """(NUMA node, cpu list) of the GPU's PCI function as /sys exposes them, or (None, None).  The host feed of rank r
    (142 MB per 608x608 fp32 batch) should run on the cores next to GPU r's root port."""
    bdf = device_pci_bus_id(dev).lower()
    if not bdf:
        return None, None
    try:
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read().strip())
        if node < 0:
            return None, None
        cpus = []
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus += list(range(int(lo), int(hi or lo) + 1))
        return node, cpus
    except (OSError, ValueError):
        return None, None
