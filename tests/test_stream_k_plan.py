"""Host arithmetic of the stream-K plan (y2h_p8_stream_k_plan, y2_conv_f16.hip) and of the stream-K share rule
(include/y2_streamk_rule.h) -- no GPU needed.

Every kernel that cuts K loops and every launch that adds the pieces up derives them from share boundaries floor(w * I / G)
through one header; the y2h_sk_* wrappers run that very code on the host.  This test restates the rule in Python as the
independent check and compares the two: for the plans the host really makes and for the fp32 form (every tile cut) and
the one unfinished piece per workgroup, that the pieces partition the cut tiles' K loops exactly once, that no share
exceeds one tile (at most two pieces per workgroup: the slot scheme 2*wg + piece relies on it), that the first share of a
tile and the walk from it are what a brute-force search finds, and that the BASELINE fp16 shapes (darknet19_448 b128: 392 /
784 / 1568 tiles on 256 workgroups) are split as DESIGN.md says."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet


def _plan(ntiles, nk, grid):
    t, w = C.c_int(0), C.c_int(0)
    r = darknet.lib().y2h_p8_stream_k_plan(ntiles, nk, grid, C.byref(t), C.byref(w))
    return r, t.value, w.value


def _pieces_restated(sk_tiles, sk_wgs, nk):
    """(wg, piece, tile, kb, ke): the rule restated"""
    total = sk_tiles * nk
    out = []
    for w in range(sk_wgs):
        lo, hi = w * total // sk_wgs, (w + 1) * total // sk_wgs
        if hi <= lo:
            continue
        t0, k0, ln = lo // nk, lo % nk, hi - lo
        assert ln <= nk
        out.append((w, 0, t0, k0, min(nk, k0 + ln)))
        if k0 + ln > nk:
            out.append((w, 1, t0 + 1, 0, k0 + ln - nk))
    return out


def _shares(sk_tiles, sk_wgs, nk):
    """[n, tile, kb0, ke0, ke1] per workgroup from the compiled rule"""
    buf = (C.c_int * (5 * sk_wgs))()
    assert darknet.lib().y2h_sk_shares(sk_tiles, nk, sk_wgs, buf) == 0
    return np.frombuffer(buf, dtype=np.intc).reshape(sk_wgs, 5)


def _first(sk_tiles, sk_wgs, nk):
    buf = (C.c_int * sk_tiles)()
    assert darknet.lib().y2h_sk_first(sk_tiles, nk, sk_wgs, buf) == 0
    return np.frombuffer(buf, dtype=np.intc)


def _walk(sk_tiles, sk_wgs, nk):
    """(tile, wg, piece) in the order the reduce / fix-up kernels visit them"""
    buf = (C.c_int * (3 * (sk_tiles + sk_wgs)))()
    n = darknet.lib().y2h_sk_walk(sk_tiles, nk, sk_wgs, buf, sk_tiles + sk_wgs)
    assert n >= 0
    return np.frombuffer(buf, dtype=np.intc)[:3 * n].reshape(n, 3)


def _pieces(sk_tiles, sk_wgs, nk):
    """(wg, piece, tile, kb, ke) from the compiled rule (y2_sk_share_of: what conv_mfma_kernel's stream-K forms run), held
    against the restatement (which is also what conv_p8_f16_kernel still writes out for itself)"""
    out = []
    for w, (n, tile, kb0, ke0, ke1) in enumerate(_shares(sk_tiles, sk_wgs, nk).tolist()):
        if n >= 1:
            out.append((w, 0, tile, kb0, ke0))
        if n == 2:
            out.append((w, 1, tile + 1, 0, ke1))
    assert out == _pieces_restated(sk_tiles, sk_wgs, nk)
    return out


@pytest.mark.parametrize("ntiles,nk,grid", [(392, 72, 256), (784, 36, 256), (1568, 18, 256), (392, 8, 256), (136, 72, 256),
                                            (12, 18, 7), (300, 9, 256), (257, 144, 256), (511, 4, 256), (1000, 1, 256)])
def test_plan_pieces_partition_the_tail(monkeypatch, ntiles, nk, grid):
    for k in ("Y2_SK", "Y2_SK_TILES", "Y2_SK_WGS", "Y2_SK_MARGIN", "Y2_SK_MINK"):
        monkeypatch.delenv(k, raising=False)
    r, t, w = _plan(ntiles, nk, grid)
    if not r:
        assert t == 0 and w == 0
        return
    assert 0 < t <= w <= grid and t <= ntiles
    assert t == ntiles % grid                       # the plan splits exactly the last, partial round
    cover = [[0] * nk for _ in range(t)]
    slots = set()
    for (wg, piece, tile, kb, ke) in _pieces(t, w, nk):
        assert 0 <= tile < t and 0 <= kb < ke <= nk
        assert (wg, piece) not in slots
        slots.add((wg, piece))
        for k in range(kb, ke):
            cover[tile][k] += 1
    assert all(c == 1 for row in cover for c in row)


def test_baseline_fp16_shapes_are_split(monkeypatch):
    for k in ("Y2_SK", "Y2_SK_TILES", "Y2_SK_WGS", "Y2_SK_MARGIN", "Y2_SK_MINK"):
        monkeypatch.delenv(k, raising=False)
    # darknet19_448 b128, 3x3 layers on the 256x256 tile: 28x28 256->512 (784 tiles, 36 K-tiles), 14x14 512->1024 (392, 72)
    assert _plan(784, 36, 256)[0] == 1
    assert _plan(392, 72, 256)[0] == 1
    # a full last round is left alone, and so is everything when switched off
    assert _plan(512, 36, 256) == (0, 0, 0)
    monkeypatch.setenv("Y2_SK", "0")
    assert _plan(784, 36, 256) == (0, 0, 0)


def test_forced_plan_keeps_a_share_within_one_tile(monkeypatch):
    monkeypatch.setenv("Y2_SK_TILES", "9")
    monkeypatch.setenv("Y2_SK_WGS", "4")            # fewer workgroups than tiles: raised to the tile count
    assert _plan(12, 18, 16) == (1, 9, 9)
    monkeypatch.setenv("Y2_SK_WGS", "40")           # more than the grid: clamped
    assert _plan(12, 18, 16) == (1, 9, 16)
    monkeypatch.setenv("Y2_SK_TILES", "30")         # more than there are tiles
    assert _plan(12, 18, 16) == (1, 12, 16)


def _check_rule(tiles, G, nk):
    """every property of the rule for one (tiles, G, nk), the compiled code against brute force"""
    I = tiles * nk
    w = np.arange(G + 1, dtype=np.int64)
    bounds = w * I // G
    lo, hi = bounds[:-1], bounds[1:]
    sh = _shares(tiles, G, nk)
    n = sh[:, 0]
    assert ((n == 0) == (hi == lo)).all() and n.max() <= 2            # empty exactly when hi == lo; at most two pieces
    pieces = _pieces(tiles, G, nk)                                    # (also: equal to the restatement)
    # every (tile, K-step) exactly once; the pieces of a share are its K-steps in order
    cover = np.zeros(I, dtype=np.int32)
    for (wg, piece, tile, kb, ke) in pieces:
        assert 0 <= tile < tiles and 0 <= kb < ke <= nk
        cover[tile * nk + kb:tile * nk + ke] += 1
        assert tile * nk + kb == (lo[wg] if piece == 0 else (lo[wg] // nk + 1) * nk)
    assert (cover == 1).all()
    assert all(ke == nk for (wg, piece, tile, kb, ke) in pieces if piece == 0 and sh[wg, 0] == 2)
    # first share of a tile = the lowest non-empty share that intersects it (brute force over all shares)
    tb = np.arange(tiles, dtype=np.int64)[:, None] * nk
    hits = (hi > lo)[None, :] & (lo[None, :] < tb + nk) & (hi[None, :] > tb)          # [tile][share]
    assert hits.any(axis=1).all()
    assert (_first(tiles, G, nk) == hits.argmax(axis=1)).all()
    # the walk visits exactly the intersecting shares, tile by tile, in ascending K = ascending workgroup
    want = [(t, wg, int(lo[wg] < t * nk)) for t in range(tiles) for wg in np.flatnonzero(hits[t]).tolist()]
    assert [tuple(v) for v in _walk(tiles, G, nk).tolist()] == want
    return pieces, hits


def test_rule_exhaustive():
    for nk in (1, 2, 4, 9, 18, 27):
        for G in range(1, 49):
            for tiles in range(1, G + 1):
                _check_rule(tiles, G, nk)


@pytest.mark.parametrize("tiles,G,nk", [(113, 256, 18), (6, 256, 144), (1, 2, 16), (200, 512, 9), (255, 256, 27), (256, 256, 36)])
def test_fp32_stream_k_all_tiles_cut(tiles, G, nk):
    """conv_mfma_kernel<..., 1>: ALL output tiles are cut (sk_tiles = ntiles), slot 2 * wg + piece, and sk_reduce_kernel reads
    slot 2 * w + piece of every share its walk visits: each slot written is read exactly once, by its own tile"""
    pieces, _ = _check_rule(tiles, G, nk)
    written = {2 * wg + piece: tile for (wg, piece, tile, kb, ke) in pieces}
    assert len(written) == len(pieces)
    read = [(2 * wg + piece, t) for (t, wg, piece) in _walk(tiles, G, nk).tolist()]
    assert sorted(read) == sorted(written.items())


@pytest.mark.parametrize("ntiles,sk_tiles,G,nk", [(1444, 164, 256, 36), (300, 44, 256, 72), (9, 2, 7, 18), (40, 8, 8, 4), (513, 1, 512, 27)])
def test_share_rule_one_unfinished_piece_per_workgroup(ntiles, sk_tiles, G, nk):
    """A property of the share rule that conv_p8_f16_kernel relies on (the last sk_tiles of ntiles tiles cut over G workgroups):
    at most one piece per workgroup does not end its tile's K loop ("producer"), and the earlier pieces of a tile belong to
    the workgroups below the one that ends it ("finisher"): the shares its tile's walk visits below that workgroup are exactly
    the tile's producers, ascending K"""
    pieces, _ = _check_rule(sk_tiles, G, nk)
    producers = [(wg, tile) for (wg, piece, tile, kb, ke) in pieces if ke < nk]
    assert len({wg for wg, _ in producers}) == len(producers)           # slot = workgroup is unique
    walk = _walk(sk_tiles, G, nk).tolist()
    for (wg, piece, tile, kb, ke) in pieces:
        if ke == nk and kb > 0:                                         # a finisher with earlier pieces
            gathered = [w for (t, w, pc) in walk if t == tile and w < wg]
            assert gathered == [w for (w, t) in producers if t == tile]
        assert ntiles - sk_tiles + tile < ntiles                        # cut tiles follow the ndp = ntiles - sk_tiles whole ones
    # every producer is gathered by exactly one finisher: the workgroup that ends the producer's tile
    for (w, t) in producers:
        enders = [wg for (wg, piece, tile, kb, ke) in pieces if tile == t and ke == nk]
        assert len(enders) == 1 and enders[0] > w
