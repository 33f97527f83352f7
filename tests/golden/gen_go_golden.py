#!/usr/bin/env python3
"""Reference-run fixture of the Go path: tests/golden/go.npz.

The reference's go.c is compiled where it lies into a temporary directory, together with tests/native/go_ref.c (the
driver, which also states the three image.c functions go.c calls -- image.c has no compiled form here), and linked
against oracle/_ref/libdarknet_ref.so.  Everything stored is data the reference's own functions returned: liberties,
legal and suicide maps, boards after move_go, packed strings, load_go_moves' records, random_go_moves' batch, and --
on the two zoo.GO networks with synthetic weights -- predict_move rows, generate_move returns with the uniform each
call drew, a 12-ply game and valid_go's predictions.

The generator ASSERTS, and exits non-zero otherwise, that
  * the driver's image functions equal numpy.rot90(a, 1) / fliplr on an asymmetric array (permutations: nothing rounds),
  * every hand-built position has the property its name claims,
  * each branch of generate_move's decision asked for occurs in a pick case,
  * tests/go_rule.py reproduces every recorded value bit for bit.

    python tests/golden/gen_go_golden.py
    python tests/golden/gen_go_golden.py --driver-only     # only leave the driver as oracle/_ref/go_ref (tools/go_latency.py)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import synth, zoo  # noqa: E402
from tests import go_rule as G  # noqa: E402
from tests.golden.gen_hier_golden import REF_DIR, reference_sources, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "go.npz")
P, KO, REC = G.P, G.KO, G.REC
F = np.float32
WSEED = {"go-mini": 31, "go": 32}
ZERO_KO = bytes(KO)


def build_go_ref(tmp, rpath=REF_DIR):
    """the link line of oracle/build_ref.sh:36-38, plus go.c itself"""
    exe = os.path.join(tmp, "go_ref")
    src = reference_sources()
    subprocess.check_call(["gcc", "-O2", "-w", "-fopenmp", "-ffp-contract=off", "-rdynamic", "-iquote", src,
                           os.path.join(ROOT, "tests", "native", "go_ref.c"), os.path.join(src, "go.c"), "-o", exe,
                           "-L" + REF_DIR, "-ldarknet_ref", "-Wl,-rpath," + rpath, "-Wl,--unresolved-symbols=ignore-in-shared-libs",
                           "-lm", "-lpthread", "-ldl"])
    return exe


def run(exe, *args):
    subprocess.check_call([exe] + [str(a) for a in args], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def pt(r, c):
    return r * 19 + c


def board_of(black=(), white=()):
    b = np.zeros(P, F)
    for r, c in black:
        b[pt(r, c)] = 1
    for r, c in white:
        b[pt(r, c)] = -1
    return b


def spiral():
    """one colour along a square spiral with one empty lane between the turns: a single chain"""
    b = np.zeros((19, 19), F)
    r, c, dr, dc = 0, 0, 0, 1
    b[r, c] = 1
    while True:
        nr, nc = r + dr, c + dc
        ahead = (nr + dr, nc + dc)
        ok = 0 <= nr < 19 and 0 <= nc < 19 and b[nr, nc] == 0 and not (0 <= ahead[0] < 19 and 0 <= ahead[1] < 19 and b[ahead] == 1)
        if not ok:
            dr, dc = dc, -dr
            nr, nc = r + dr, c + dc
            ahead = (nr + dr, nc + dc)
            if not (0 <= nr < 19 and 0 <= nc < 19 and b[nr, nc] == 0) or (0 <= ahead[0] < 19 and 0 <= ahead[1] < 19 and b[ahead] == 1):
                break
        r, c = nr, nc
        b[r, c] = 1
    return b.reshape(P)


def random_play(seed, plies):
    """seeded random non-suicidal play from the empty board by the rule: (board, ko of that ply, player to move)"""
    rng = np.random.RandomState(seed)
    b, player = np.zeros(P, F), 1
    strings = [ZERO_KO, ZERO_KO]
    for t in range(plies):
        ko = strings[t & 1]
        legal, sui = G.legal_map(b, ko, player), G.suicide_map(b, player)
        cand = np.flatnonzero((legal == 1) & (sui == 0))
        if not len(cand):
            break
        at = int(cand[rng.randint(len(cand))])
        b = G.move(b, player, at // 19, at % 19)
        strings[t & 1] = G.pack(b)
        player = -player
    return b, strings[plies & 1], player


def positions():
    """(name, board, ko, player) with the property each name claims asserted"""
    out = []
    out.append(("empty", np.zeros(P, F), ZERO_KO, 1))
    b = board_of(black=[(0, 0)])
    assert G.liberties(b)[0] == 2
    out.append(("corner_stone", b, ZERO_KO, -1))
    b = board_of(white=[(0, 9)])
    assert G.liberties(b)[9] == 3
    out.append(("edge_stone", b, ZERO_KO, 1))
    # the empty point (6, 5) touches the group above it and to its right: it counts once
    b = board_of(black=[(5, 5), (5, 6), (6, 6)])
    g = G.group(b, pt(5, 5))
    assert len(g) == 3 and sum(q in g for q in G.neighbours(pt(6, 5))) == 2 and G.liberties(b)[pt(5, 5)] == 7
    out.append(("two_sides", b, ZERO_KO, -1))
    # black at (1, 1) captures the white stones at (0, 1) and (1, 0), two groups
    b = board_of(black=[(0, 0), (0, 2), (2, 0)], white=[(0, 1), (1, 0)])
    lib = G.liberties(b)
    after = G.move(b, 1, 1, 1)
    assert lib[pt(0, 1)] == 1 and lib[pt(1, 0)] == 1 and G.group(b, pt(0, 1)) != G.group(b, pt(1, 0))
    assert after[pt(0, 1)] == 0 and after[pt(1, 0)] == 0 and after[pt(1, 1)] == 1
    out.append(("double_capture", b, ZERO_KO, 1))
    # ko: white takes at (4, 4); black's recapture at (4, 5) would give the position back
    p0 = board_of(black=[(3, 4), (4, 3), (5, 4), (4, 5)], white=[(3, 5), (4, 6), (5, 5)])
    p1 = G.move(p0, -1, 4, 4)
    assert p1[pt(4, 5)] == 0 and np.array_equal(G.move(p1, 1, 4, 5), p0)
    assert G.legal_map(p1, G.pack(p0), 1)[pt(4, 5)] == 0 and G.legal_map(p1, ZERO_KO, 1)[pt(4, 5)] == 1
    out.append(("ko_forbidden", p1, G.pack(p0), 1))
    out.append(("ko_zero_string", p1, ZERO_KO, 1))
    bad = bytearray(G.pack(p0))
    bad[90] |= 0x40                                 # bits no board packs to: the string never matches
    out.append(("ko_stray_bits", p1, bytes(bad), 1))
    both = bytearray(G.pack(p0))
    both[0] |= 3                                    # `me` and `you` on one point: no board packs to that either
    out.append(("ko_both_bits", p1, bytes(both), 1))
    # (0, 0) is suicide for black; legal_go does not say so
    b = board_of(white=[(0, 1), (1, 0), (1, 1)])
    assert G.suicide_map(b, 1)[0] == 1 and G.legal_map(b, ZERO_KO, 1)[0] == 1
    out.append(("suicide_corner", b, ZERO_KO, 1))
    # (0, 0) has no empty neighbour for black, but the stone captures both neighbours
    b = board_of(black=[(0, 2), (1, 1), (2, 0)], white=[(0, 1), (1, 0)])
    after = G.move(b, 1, 0, 0)
    assert G.suicide_map(b, 1)[0] == 0 and all(b[q] != 0 for q in G.neighbours(0)) and after[1] == 0 and after[19] == 0
    out.append(("capture_not_suicide", b, ZERO_KO, 1))
    b = spiral()
    assert len(G.group(b, 0)) == int((b != 0).sum()) > 150
    out.append(("spiral", b, ZERO_KO, -1))
    out.append(("spiral_white", np.where(b != 0, F(-1), F(0)), ZERO_KO, -1))
    # white everywhere but two eyes: black has two legal points and both are suicide
    b = -np.ones(P, F)
    b[pt(3, 3)] = 0
    b[pt(15, 15)] = 0
    assert G.legal_map(b, ZERO_KO, 1).sum() == 2 and G.suicide_map(b, 1)[pt(3, 3)] == 1 and G.suicide_map(b, 1)[pt(15, 15)] == 1
    out.append(("two_eyes", b, ZERO_KO, 1))
    b = np.ones(P, F)
    b[::3] = -1
    assert G.legal_map(b, ZERO_KO, 1).sum() == 0
    out.append(("no_legal_point", b, ZERO_KO, 1))
    b, ko, player = random_play(901, 330)
    assert (b == 0).sum() < 120
    out.append(("nearly_full", b, ko, player))
    for seed, plies in ((902, 7), (903, 40), (904, 41), (905, 120), (906, 121), (907, 216), (908, 217)):
        b, ko, player = random_play(seed, plies)
        out.append(("play_%d_%d" % (seed, plies), b, ko, player))
    assert {p for _, _, _, p in out} == {1, -1}
    return out


def pack_positions(path, pos):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(pos)))
        for _, b, ko, player in pos:
            f.write(np.asarray(b, F).tobytes() + bytes(ko) + struct.pack("<i", player))


def reference_rules(exe, tmp, pos):
    pack_positions(os.path.join(tmp, "rules.in"), pos)
    run(exe, "rules", os.path.join(tmp, "rules.in"), os.path.join(tmp, "rules.out"))
    raw = np.fromfile(os.path.join(tmp, "rules.out"), np.uint8).reshape(len(pos), P * 4 + 2 * P)
    lib = raw[:, :P * 4].copy().view(np.int32).reshape(len(pos), P)
    return lib, raw[:, P * 4:P * 5].copy(), raw[:, P * 5:].copy()


def reference_moves(exe, tmp, cases):
    with open(os.path.join(tmp, "moves.in"), "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for b, player, at in cases:
            f.write(np.asarray(b, F).tobytes() + struct.pack("<iii", player, at // 19, at % 19))
    run(exe, "moves", os.path.join(tmp, "moves.in"), os.path.join(tmp, "moves.out"))
    raw = np.fromfile(os.path.join(tmp, "moves.out"), np.uint8).reshape(len(cases), P * 4 + KO)
    return raw[:, :P * 4].copy().view(F).reshape(len(cases), P), raw[:, P * 4:].copy()


def generate_job(seed, player, board, multi, thresh, temp, ko):
    return (struct.pack("<ii", seed, player) + np.asarray(board, F).tobytes() + struct.pack("<iff", int(multi), thresh, temp) + bytes(ko))


def read_generate(buf, at):
    index, u = struct.unpack_from("<if", buf, at)
    kept = np.frombuffer(buf, F, P, at + 8).copy()
    return index, F(u), kept, at + 8 + P * 4


def pick_rows(pos):
    """(position index, row, thresh, seed): crafted network outputs that drive generate_move into each branch"""
    names = [p[0] for p in pos]
    rng = np.random.RandomState(77)
    cases = []

    def soft(peak_at=None, peak=0.0):
        r = rng.rand(P).astype(F) + F(.05)
        r = (r / r.sum() * F(1 - peak)).astype(F)
        if peak_at is not None:
            r[peak_at] = F(peak)
        return r
    mid, mid2 = names.index("play_905_120"), names.index("play_906_121")
    empties = np.flatnonzero(pos[mid][1] == 0)
    cases.append(("thresh_below_best", mid, soft(int(empties[5]), .5), .1, 11))
    cases.append(("thresh_above_best", mid2, soft(), .1, 12))
    r = np.full(P, 1e-4, F)                         # ties among the five best, and equal values an entry is displaced past
    e2 = np.flatnonzero(pos[mid2][1] == 0)
    r[e2[[3, 9, 20]]] = F(.04)
    r[e2[[1, 30, 31]]] = F(.05)
    r[e2[40]] = F(.06)
    cases.append(("ties_thresh_above", mid2, r, .1, 13))
    r = r.copy()
    r[e2[40]] = F(.3)
    cases.append(("ties_thresh_below", mid2, r, .1, 14))
    sc = names.index("suicide_corner")
    cases.append(("argmax_suicide", sc, soft(0, .6), .1, 15))
    r = np.full(P, 1e-5, F)
    r[0], r[pt(9, 9)] = F(.45), F(.5)
    for seed in range(100, 200):                    # a draw that lands on the suicide corner: found by search, asserted below
        cases.append(("sample_suicide_%d" % seed, sc, r, .1, seed))
    cases.append(("no_legal_point", names.index("no_legal_point"), soft(), .1, 16))
    cases.append(("empty_white", names.index("empty"), soft(), .3, 17))
    cases.append(("ko_forbidden", names.index("ko_forbidden"), soft(pt(4, 5), .7), .1, 18))
    cases.append(("white_midgame", names.index("play_904_41"), soft(), .05, 19))
    return cases


def reference_pick(exe, tmp, pos, cases):
    with open(os.path.join(tmp, "pick.in"), "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for name, k, row, thresh, seed in cases:
            _, b, ko, player = pos[k]
            player = -1 if name == "empty_white" else player
            f.write(np.asarray(row, F).tobytes() + generate_job(seed, player, b, 0, thresh, 1.0, ko))
    run(exe, "pick", os.path.join(tmp, "pick.in"), os.path.join(tmp, "pick.out"))
    buf, at, got = open(os.path.join(tmp, "pick.out"), "rb").read(), 0, []
    for _ in cases:
        index, u, kept, at = read_generate(buf, at)
        got.append((index, u, kept))
    return got


def materialize(tmp, name):
    cfg, wts = os.path.join(tmp, name + ".cfg"), os.path.join(tmp, name + ".weights")
    with open(cfg, "w") as f:
        f.write(zoo.go_cfg_text(name, 1))
    synth.write_go_weights(wts, name, WSEED[name])
    return cfg, wts


def reference_net(exe, tmp, name, jobs):
    """jobs: ("predict", board, multi) | ("generate", seed, player, board, multi, thresh, temp, ko) | ("game", seed, plies,
    multi, thresh, temp) | ("valid", record, multi) -> their results in order"""
    cfg, wts = materialize(tmp, name)
    layers = len(zoo.GO[name])
    with open(os.path.join(tmp, "net.in"), "wb") as f:
        for j in jobs:
            if j[0] == "predict":
                f.write(struct.pack("<i", 1) + np.asarray(j[1], F).tobytes() + struct.pack("<i", int(j[2])))
            elif j[0] == "generate":
                f.write(struct.pack("<i", 2) + generate_job(*j[1:]))
            elif j[0] == "game":
                f.write(struct.pack("<iiiiff", 3, j[1], j[2], int(j[3]), j[4], j[5]))
            else:
                f.write(struct.pack("<i", 4) + bytes(j[1]) + struct.pack("<i", int(j[2])))
    run(exe, "net", cfg, wts, os.path.join(tmp, "net.in"), os.path.join(tmp, "net.out"))
    buf, at, out = open(os.path.join(tmp, "net.out"), "rb").read(), 0, []
    for j in jobs:
        if j[0] == "predict":
            out.append(np.frombuffer(buf, F, P, at).copy())
            at += P * 4
        elif j[0] == "generate":
            index, u, kept, at = read_generate(buf, at)
            temps = np.frombuffer(buf, F, layers, at).copy()
            at += layers * 4
            out.append((index, u, kept, temps))
        elif j[0] == "game":
            (plies,) = struct.unpack_from("<i", buf, at)
            at += 4
            idx, us, recs = [], [], []
            while True:
                (index,) = struct.unpack_from("<i", buf, at)
                at += 4
                if index == -2:
                    break
                us.append(struct.unpack_from("<f", buf, at)[0])
                at += 4
                idx.append(index)
                if index >= 0:
                    recs.append(np.frombuffer(buf, np.uint8, REC, at).copy())
                    at += REC
            (count,) = struct.unpack_from("<i", buf, at)
            board = np.frombuffer(buf, F, P, at + 4).copy()
            at += 4 + P * 4
            assert count == len(recs) <= plies
            out.append((np.array(idx, np.int32), np.array(us, F), np.array(recs, np.uint8).reshape(-1, REC), board))
        else:
            out.append(struct.unpack_from("<i", buf, at)[0])
            at += 4
    assert at == len(buf)
    return out


def main():
    if not os.path.exists(os.path.join(REF_DIR, "libdarknet_ref.so")):
        sys.exit("oracle/_ref/libdarknet_ref.so missing: run oracle/build_ref.sh where the reference checkout exists")
    if "--driver-only" in sys.argv:
        build_go_ref(REF_DIR, "$ORIGIN")
        print("wrote", os.path.join(REF_DIR, "go_ref"))
        return
    A = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_go_ref(tmp)
        # the driver's image functions are the permutations the rule states
        run(exe, "image", os.path.join(tmp, "image.out"))
        img = np.fromfile(os.path.join(tmp, "image.out"), F).reshape(16, 19, 19)
        a = np.arange(P, dtype=F).reshape(19, 19)
        for k, t in enumerate(range(-7, 8)):
            assert np.array_equal(img[k], np.rot90(a, t % 4)), "rotate_image_cw(%d)" % t
        assert np.array_equal(img[15], np.fliplr(a)) and not np.array_equal(img[8], a.T)

        # ---- positions: liberties, legal, suicide ----
        pos = positions()
        lib, legal, sui = reference_rules(exe, tmp, pos)
        for k, (name, b, ko, player) in enumerate(pos):
            assert np.array_equal(G.liberties(b), lib[k]), name
            assert np.array_equal(G.legal_map(b, ko, player), legal[k]), name
            assert np.array_equal(G.suicide_map(b, player), sui[k]), name
        names = [p[0] for p in pos]
        assert legal[names.index("ko_forbidden")][pt(4, 5)] == 0 and legal[names.index("ko_zero_string")][pt(4, 5)] == 1
        assert legal[names.index("ko_stray_bits")][pt(4, 5)] == 1 and legal[names.index("ko_both_bits")][pt(4, 5)] == 1
        assert legal[names.index("no_legal_point")].sum() == 0
        A["pos_names"] = np.array(names)
        A["pos_boards"] = np.array([p[1] for p in pos]).astype(np.int8)
        A["pos_ko"] = np.array([np.frombuffer(bytes(p[2]), np.uint8) for p in pos])
        A["pos_players"] = np.array([p[3] for p in pos], np.int32)
        A["pos_liberties"], A["pos_legal"], A["pos_suicide"] = lib.astype(np.int16), legal, sui

        # ---- moves: a few legal points of every position, the captures among them ----
        rng = np.random.RandomState(5)
        mv = []
        for k, (name, b, ko, player) in enumerate(pos):
            cand = np.flatnonzero(legal[k])
            take = set(int(c) for c in cand[rng.permutation(len(cand))[:2]])
            take |= {"double_capture": {pt(1, 1)}, "capture_not_suicide": {0}, "ko_zero_string": {pt(4, 5)}}.get(name, set())
            mv += [(k, at) for at in sorted(take)]
        after, strings = reference_moves(exe, tmp, [(pos[k][1], pos[k][3], at) for k, at in mv])
        for (k, at), b2, s in zip(mv, after, strings):
            assert np.array_equal(G.move(pos[k][1], pos[k][3], at // 19, at % 19), b2) and G.pack(b2) == s.tobytes()
            assert np.array_equal(G.unpack(s.tobytes()), b2)
        A["move_pos"], A["move_at"] = np.array([k for k, _ in mv], np.int32), np.array([at for _, at in mv], np.int32)
        A["move_after"], A["move_string"] = after.astype(np.int8), strings

        # ---- pick: generate_move on preset rows ----
        cases = pick_rows(pos)
        got = reference_pick(exe, tmp, pos, cases)
        keep, hit = [], None
        for c, g in zip(cases, got):
            if c[0].startswith("sample_suicide"):
                if hit is None and g[0] == pt(9, 9) and g[1] < F(.45):    # the draw fell into the corner's share: the arg-max came back
                    hit = True
                    keep.append((("sample_suicide",) + c[1:], g))
                continue
            keep.append((c, g))
        assert hit, "no seed made the sample land on the suicide point"
        pk = {"names": [], "pos": [], "players": [], "move": [], "thresh": [], "u": [], "index": [], "kept": []}
        for (name, k, row, thresh, seed), (index, u, kept) in keep:
            _, b, ko, player = pos[k]
            player = -1 if name == "empty_white" else player
            move = np.where(b != 0, F(0), row).astype(F)            # what predict_move hands back
            lg, su = (G.legal_map(b, ko, player), G.suicide_map(b, player))
            r_index, r_kept = G.pick(move, lg, su, thresh, u)
            assert r_index == index and np.array_equal(r_kept, kept), name
            for key, v in zip(("names", "pos", "players", "move", "thresh", "u", "index", "kept"), (name, k, player, move, thresh, u, index, kept)):
                pk[key].append(v)
        by = dict(zip(pk["names"], zip(pk["index"], pk["kept"], pk["move"], pk["thresh"])))
        assert by["thresh_below_best"][3] < by["thresh_below_best"][2].max() and (by["thresh_below_best"][1] > 0).sum() < 5
        assert by["thresh_above_best"][3] > by["thresh_above_best"][2].max() and (by["thresh_above_best"][1] > 0).sum() >= 5
        assert by["argmax_suicide"][0] == -1 and by["sample_suicide"][0] == pt(9, 9)
        assert by["no_legal_point"][0] in (-1, 360, 0) and not by["no_legal_point"][1].any()
        A["pick_names"] = np.array(pk["names"])
        A["pick_pos"], A["pick_players"], A["pick_index"] = (np.array(pk[k], np.int32) for k in ("pos", "players", "index"))
        A["pick_move"], A["pick_kept"] = np.array(pk["move"], F), np.array(pk["kept"], F)
        A["pick_thresh"], A["pick_u"] = np.array(pk["thresh"], F), np.array(pk["u"], F)

        # ---- the networks ----
        ib = [names.index(n) for n in ("play_903_40", "play_904_41", "play_905_120")]
        seen = lambda k: pos[k][1] * pos[k][3]                     # the board as its mover sees it
        jobs = [("predict", seen(k), m) for m in (0, 1) for k in ib]
        gen = [(k, m, th, te) for k, m, th, te in ((ib[0], 0, .1, .7), (ib[1], 1, .1, .7), (ib[2], 1, .0, 1.),
                                                   (names.index("ko_forbidden"), 0, .1, .7), (names.index("two_eyes"), 0, .1, .7),
                                                   (names.index("empty"), 1, .3, .5), (names.index("nearly_full"), 0, .1, 1.))]
        jobs += [("generate", 40 + i, pos[k][3], pos[k][1], m, th, te, pos[k][2]) for i, (k, m, th, te) in enumerate(gen)]
        jobs += [("game", 7, 12, 1, .1, .7)]
        res = reference_net(exe, tmp, "go-mini", jobs)
        A["mini_predict_pos"] = np.array(ib * 2, np.int32)
        A["mini_predict_multi"] = np.array([0] * 3 + [1] * 3, np.int32)
        A["mini_predict_rows"] = np.array(res[:6], F)
        g = res[6:6 + len(gen)]
        A["mini_gen_pos"] = np.array([k for k, _, _, _ in gen], np.int32)
        A["mini_gen_multi"] = np.array([m for _, m, _, _ in gen], np.int32)
        A["mini_gen_thresh"], A["mini_gen_temp"] = np.array([t for _, _, t, _ in gen], F), np.array([t for _, _, _, t in gen], F)
        A["mini_gen_seed"] = np.array([40 + i for i in range(len(gen))], np.int32)
        A["mini_gen_index"], A["mini_gen_u"] = np.array([x[0] for x in g], np.int32), np.array([x[1] for x in g], F)
        for x, (_, _, _, te) in zip(g, gen):
            assert np.all(x[3] == F(te)), "generate_move leaves temp on every layer"
        assert A["mini_gen_index"][4] == -1 and A["mini_gen_index"][3] != pt(4, 5)
        assert {pos[k][3] for k, _, _, _ in gen} == {1, -1}
        idx, us, recs, final = res[-1]
        assert len(idx) == 12 and (idx >= 0).all()
        A["game_index"], A["game_u"], A["game_records"], A["game_final"] = idx, us, recs, final.astype(np.int8)
        # valid_go on the game's first five records, and the loader on a file of all twelve
        vres = reference_net(exe, tmp, "go-mini", [("valid", recs[i], m) for m in (0, 1) for i in range(5)])
        A["valid_records"], A["valid_predicted"] = recs[:5], np.array(vres, np.int32).reshape(2, 5)
        moves_file = os.path.join(tmp, "game.moves")
        with open(moves_file, "wb") as f:
            for r in recs:
                f.write(r.tobytes() + b"\n")
        run(exe, "batch", moves_file, 123, 4, os.path.join(tmp, "batch.out"))
        buf = open(os.path.join(tmp, "batch.out"), "rb").read()
        (nraw,) = struct.unpack_from("<i", buf, 0)
        raw = np.frombuffer(buf, np.int32, nraw, 4)
        xy = np.frombuffer(buf, F, 2 * 4 * P, 4 + 4 * nraw).reshape(2, 4, P)
        assert nraw == 12
        pick_, flip_, rot = raw[0::3] % len(recs), raw[1::3] % 2, raw[2::3] % 4
        rx, ry = G.loader(recs, pick_, flip_, rot)
        assert np.array_equal(rx, xy[0]) and np.array_equal(ry, xy[1])
        A["batch_seed"] = np.array(123, np.int32)
        A["batch_pick"], A["batch_flip"], A["batch_rot"] = pick_.astype(np.int32), flip_.astype(np.int32), rot.astype(np.int32)
        A["batch_x"], A["batch_y"] = xy[0].astype(np.int8), xy[1].astype(np.int8)
        three = os.path.join(tmp, "three.moves")
        with open(three, "wb") as f:
            for r in recs[:3]:
                f.write(r.tobytes() + b"\n")
            f.write(b"short tail")
        run(exe, "load", three, os.path.join(tmp, "load.out"))
        buf = open(os.path.join(tmp, "load.out"), "rb").read()
        assert struct.unpack_from("<i", buf, 0)[0] == 3 and buf[4:] == recs[:3].tobytes()
        A["load_records"] = recs[:3]

        # ---- go.test.cfg's topology ----
        k = ib[2]
        res = reference_net(exe, tmp, "go", [("predict", seen(k), 1), ("predict", seen(ib[1]), 0),
                                             ("generate", 60, pos[k][3], pos[k][1], 1, .1, .7, pos[k][2])])
        A["go_predict_pos"], A["go_predict_multi"] = np.array([k, ib[1]], np.int32), np.array([1, 0], np.int32)
        A["go_predict_rows"] = np.array(res[:2], F)
        A["go_gen_pos"], A["go_gen_seed"] = np.array(k, np.int32), np.array(60, np.int32)
        A["go_gen_index"], A["go_gen_u"] = np.array(res[2][0], np.int32), np.array(res[2][1], F)
        A["wseed_mini"], A["wseed_go"] = np.array(WSEED["go-mini"], np.int32), np.array(WSEED["go"], np.int32)
    write_npz(OUT, A)
    print("wrote %s (%d bytes, %d positions, %d moves, %d pick cases)" % (OUT, os.path.getsize(OUT), len(pos), len(mv), len(keep)))


if __name__ == "__main__":
    main()
