"""Synthetic frames the tracker tests share (tests/test_kcf_host.py, tests/test_gpu_kcf.py): a 96 x 128 BGR scene of a
high-contrast blocky object on low-contrast noise, and a blocky texture that is rolled as a whole."""
import numpy as np

H, W = 96, 128
BOX = (60.0, 50.0, 24.0, 28.0)                  # the object of scene(60, 50): cx, cy, w, h


def scene(cx, cy, seed=11, ow=24, oh=28):
    rng = np.random.default_rng(seed)
    f = rng.integers(90, 140, (H, W, 3)).astype(np.int64)
    orng = np.random.default_rng(seed + 1)
    obj = np.kron(orng.integers(0, 2, (oh // 4, ow // 4, 1)) * 200 + 20, np.ones((4, 4, 1), np.int64)) + orng.integers(0, 30, (oh, ow, 3))
    ys, xs = np.arange(cy - oh // 2, cy - oh // 2 + oh), np.arange(cx - ow // 2, cx - ow // 2 + ow)
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    f[np.ix_(ys[oky], xs[okx])] = obj[np.ix_(oky, okx)]
    return f.astype(np.uint8)


def texture(seed=5):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 256, (H // 4, W // 4, 1)), np.ones((4, 4, 3), np.int64)).astype(np.uint8)


def peak_margin(resp64):
    """the response maximum minus the runner-up"""
    r = np.sort(np.asarray(resp64).ravel())
    return float(r[-1] - r[-2])
