"""GPU unit tests of the two kernels behind the multi-view classifier evaluations, driven through the C-ABI:
y2h_views_to_input against the numpy rule of tests/tta_rule.py (crop_image with clamped taps, flip_image) and
y2h_accumulate_rows against the sequential fp32 sum.  Both are data movement / one addition per value, so every check
is exact equality."""
import ctypes as C
import itertools

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth
from tests import tta_rule as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
SOURCES = ((9, 11), (5, 8), (3, 2), (1, 1), (7, 10))          # (sh, sw): odd and even widths, equal to / smaller than a view


class Dev:
    def __init__(self):
        self.L = darknet.lib()
        self.L.y2h_set_device(0)
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.L.y2h_malloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.L.y2h_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
        self.bufs.append(p)
        return p

    def get(self, p, shape, dtype=np.float32):
        out = np.zeros(shape, dtype=dtype)
        assert self.L.y2h_device_sync() == 0
        assert self.L.y2h_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, None) == 0
        assert self.L.y2h_device_sync() == 0
        return out

    def close(self):
        for p in self.bufs:
            self.L.y2h_free(p)


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.close()


def _pack_sources(planes, seed, pad):
    """the sources back to back in one buffer (`pad` floats in front of each, so that some start off a 16-byte
    boundary) -> (buffer, [(offset, image [planes][sh][sw])])"""
    parts, items, off = [], [], 0
    for k, (sh, sw) in enumerate(SOURCES):
        im = synth.uniform(seed + k, planes * sh * sw, -1, 1).reshape(planes, sh, sw)
        parts.append(np.full(pad, np.nan, np.float32))
        off += pad
        items.append((off, im))
        parts.append(im.reshape(-1))
        off += im.size
    return np.concatenate(parts), items


def _run_views(dev, descs, src, batch, planes, h, w, guard):
    """launch once over NaN-filled dst with `guard` sentinel floats in front of and behind it -> dst [batch][planes][h][w]"""
    n = len(descs)
    table = (darknet.View * max(n, 1))(*[darknet.View(*d, 0) for d in descs])
    d_desc = dev.put(np.frombuffer(bytes(table), dtype=np.uint8))
    d_src = dev.put(src)
    total = batch * planes * h * w
    host = np.concatenate([np.full(guard, SENTINEL), np.full(total, np.nan, np.float32), np.full(guard, SENTINEL)]).astype(np.float32)
    d_dst = dev.put(host)
    rc = dev.L.y2h_views_to_input(d_desc, n, d_src, batch, planes, h, w, C.c_void_p(d_dst.value + 4 * guard), None)
    assert rc == 0, darknet.lib().y2h_last_error()
    got = dev.get(d_dst, host.shape)
    assert (got[:guard] == SENTINEL).all() and (got[guard + total:] == SENTINEL).all(), "wrote outside dst"
    return got[guard:guard + total].reshape(batch, planes, h, w)


@pytest.mark.parametrize("planes", [3, 1])
@pytest.mark.parametrize("h,w,guard_extra", [(5, 8, 0), (6, 7, 0), (4, 12, 0), (5, 8, 1)])
def test_views_equal_the_rule(dev, planes, h, w, guard_extra):
    # (5, 8) and (4, 12): 16-byte stores; (6, 7): the scalar path; guard_extra = 1: rows of 8 at a misaligned dst
    src, items = _pack_sources(planes, 40 + planes, pad=1 if guard_extra else 0)
    descs, want = [], []
    for off, im in items:
        sh, sw = im.shape[1:]
        xs = sorted({-32, -3, 0, 2, sw - w + 3})
        ys = sorted({-32, -3, 0, 2, sh - h + 3})
        for dx, dy, flip in itertools.product(xs, ys, (0, 1)):
            descs.append((off, sw, sh, dx, dy, flip))
            want.append(R.view(im, dx, dy, w, h, flip))
    n = len(descs)                                        # sources of five sizes mixed in one launch
    got = _run_views(dev, descs, src, n + 2, planes, h, w, guard=w + guard_extra)
    for b in range(n):
        assert got[b].tobytes() == want[b].tobytes(), (descs[b], got[b], want[b])
    assert not got[n:].any() and not np.isnan(got[n:]).any(), "slots n .. batch-1 must be zero"


def test_views_pad_slots_are_zeroed_and_empty_launches_work(dev):
    src, items = _pack_sources(3, 77, pad=0)
    off, im = items[0]
    descs = [(off, 11, 9, 0, 0, 0), (off, 11, 9, 1, -2, 1), (items[4][0], 10, 7, -1, 1, 1)]
    want = [R.view(im, 0, 0, 8, 5, 0), R.view(im, 1, -2, 8, 5, 1), R.view(items[4][1], -1, 1, 8, 5, 1)]
    got = _run_views(dev, descs, src, 5, 3, 5, 8, guard=8)             # batch 5 with n = 3
    for b in range(3):
        assert got[b].tobytes() == want[b].tobytes()
    assert got[3:].tobytes() == np.zeros((2, 3, 5, 8), np.float32).tobytes()
    got = _run_views(dev, [], src, 2, 3, 6, 7, guard=7)                # n = 0: everything is zeroed
    assert got.tobytes() == np.zeros((2, 3, 6, 7), np.float32).tobytes()
    # arguments outside what the kernel supports are refused, not launched
    L = dev.L
    p = dev.put(np.zeros(64, np.float32))
    assert L.y2h_views_to_input(p, 3, p, 2, 3, 2, 2, p, None) == darknet.Y2H_EINVAL      # n > batch
    assert L.y2h_views_to_input(p, 1, p, 1, 3, 0, 2, p, None) == darknet.Y2H_EINVAL
    assert L.y2h_views_to_input(None, 1, p, 1, 3, 2, 2, p, None) == darknet.Y2H_EINVAL


def _spread(seed, shape):
    """values whose magnitudes are spread over 2^20: their fp32 sum depends on the order of the additions"""
    n = int(np.prod(shape))
    mant = synth.uniform(seed, n, -1, 1)
    exp = (synth.splitmix64(seed + 1, n) % np.uint64(21)).astype(np.int32)
    return np.ldexp(mant, exp).astype(np.float32).reshape(shape)


def _accumulate_rule(acc, rows, owner, n):
    acc = acc.copy()
    for s, o in enumerate(owner):
        if o >= 0:
            acc[o] = (acc[o] + rows[s, :n]).astype(np.float32)
    return acc


OWNERS = {1: [1], 4: [0, 1, 0, -1], 10: [0, 1, 0, 0, -1, 1, 1, 0, -1, 1]}


@pytest.mark.parametrize("n", [1, 10, 1000, 1030])
@pytest.mark.parametrize("nslots", [1, 4, 10])
def test_accumulate_rows_adds_in_slot_order(dev, n, nslots):
    ld = n + 3                                              # ld > n: the pad columns hold NaN and are never read
    owner = np.array(OWNERS[nslots], np.int32)
    images = 3                                              # image 2 is owned by no slot and must not change
    acc0 = np.concatenate([np.full((1, n), SENTINEL), np.zeros((images, n), np.float32), np.full((1, n), SENTINEL)]).astype(np.float32)
    acc0[3] = _spread(5, (n,))
    d_acc = dev.put(acc0)
    inner = C.c_void_p(d_acc.value + 4 * n)                 # a guard row in front of and behind acc
    want = acc0[1:1 + images].copy()
    for launch in range(2):                                 # an image whose views straddle two forwards
        rows = np.full((nslots, ld), np.nan, np.float32)
        rows[:, :n] = _spread(100 * launch + n + nslots, (nslots, n))
        rows[owner < 0] = np.nan                            # an unused slot's row must not reach any sum
        rc = dev.L.y2h_accumulate_rows(inner, dev.put(rows), ld, dev.put(owner), nslots, n, None)
        assert rc == 0, darknet.lib().y2h_last_error()
        want = _accumulate_rule(want, rows, owner, n)
    got = dev.get(d_acc, acc0.shape)
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "wrote outside acc"
    assert got[1:1 + images].tobytes() == want.tobytes()
    assert not np.isnan(got).any()
    if nslots == 10 and n >= 10:
        # the order matters for these values: adding the same rows in reverse gives other bits somewhere
        rev = _accumulate_rule(acc0[1:1 + images], rows[::-1], owner[::-1], n)
        fwd = _accumulate_rule(acc0[1:1 + images], rows, owner, n)
        assert rev.tobytes() != fwd.tobytes()


def test_accumulate_rows_refuses_bad_arguments(dev):
    p = dev.put(np.zeros(64, np.float32))
    L = dev.L
    assert L.y2h_accumulate_rows(p, p, 4, p, 2, 8, None) == darknet.Y2H_EINVAL          # ld < n
    assert L.y2h_accumulate_rows(p, p, 8, p, 0, 8, None) == darknet.Y2H_EINVAL
    assert L.y2h_accumulate_rows(None, p, 8, p, 1, 8, None) == darknet.Y2H_EINVAL
