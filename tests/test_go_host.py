"""Go without a GPU: the go.c entry points are exported; every device-free host function is the compiled reference's
fixture (tests/golden/go.npz) bit for bit; y2_go_draw_moves is the reference's draws; the numpy statement tests/go_rule.py
equals the same fixtures, so the GPU tests may lean on it; every refusal happens before the device is touched."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth, zoo
from tests import go_rule as G
from tests.helpers import load_golden

P = G.P
EXPORTS = ("string_to_board board_to_string flip_board calculate_liberties move_go suicide_go legal_go print_board "
           "load_go_moves predict_move generate_move y2_go_predict y2_go_rules y2_go_generate y2_go_selfplay y2_go_valid "
           "y2_go_draw_moves y2_train_load_go y2h_go_views y2h_go_merge y2h_go_rules y2h_go_apply y2h_go_pick").split()


@pytest.fixture(scope="module")
def g():
    return load_golden("go")


def positions(g):
    return [(str(n), g["pos_boards"][k].astype(np.float32), g["pos_ko"][k].tobytes(), int(g["pos_players"][k]))
            for k, n in enumerate(g["pos_names"])]


def go_net(tmp, name="go-mini", batch=1, wseed=None, text=None):
    """a zoo.GO network with synthetic weights (wseed None: as parsed)"""
    cfg = os.path.join(str(tmp), "%s_b%d.cfg" % (name, batch))
    with open(cfg, "w") as f:
        f.write(zoo.go_cfg_text(name, batch) if text is None else text)
    net = darknet.Network.parse_network_cfg(cfg)
    if wseed is not None:
        wts = os.path.join(str(tmp), "%s_%d.weights" % (name, wseed))
        if not os.path.exists(wts):
            synth.write_go_weights(wts, name, wseed)
        net.load_weights(wts)
    return net


def test_exports_are_present():
    L = darknet.lib()
    for name in EXPORTS:
        assert hasattr(L, name), name


def test_zoo_go_is_the_topology_of_go_test_cfg(tmp_path):
    ref = darknet.Network.parse_network_cfg(os.path.join(os.path.dirname(__file__), "golden", "ref_cfg", "go.test.cfg"))
    own = go_net(tmp_path, "go")
    table = lambda net: [(l.type, l.n, l.size, l.stride, l.pad, l.batch_normalize, l.activation, l.h, l.w, l.c, l.outputs)
                         for l in (net.net.layers[i] for i in range(net.net.n))]
    assert table(ref) == table(own) and ref.net.n == 16 and (ref.net.h, ref.net.w, ref.net.c) == (19, 19, 1)
    ref.free()
    own.free()


def test_the_fixture_holds_what_the_issue_lists(g):
    names = set(str(n) for n in g["pos_names"])
    assert {"empty", "corner_stone", "edge_stone", "two_sides", "double_capture", "ko_forbidden", "ko_zero_string", "suicide_corner",
            "capture_not_suicide", "spiral", "nearly_full", "no_legal_point"} <= names
    assert set(g["pos_players"].tolist()) == {1, -1} and len(names) >= 20
    assert {"thresh_below_best", "thresh_above_best", "ties_thresh_above", "argmax_suicide", "sample_suicide",
            "no_legal_point"} <= set(str(n) for n in g["pick_names"])
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "go.npz")) < 100 * 1024


def test_packed_strings_round_trip(g):
    for b, s in zip(g["move_after"].astype(np.float32), g["move_string"]):
        assert darknet.board_to_string(b) == s.tobytes()
        assert np.array_equal(darknet.string_to_board(s.tobytes()), b)
        assert G.pack(b) == s.tobytes() and np.array_equal(G.unpack(s.tobytes()), b)


def test_liberties_are_the_reference(g):
    for k, (name, b, _, _) in enumerate(positions(g)):
        assert np.array_equal(darknet.calculate_liberties(b), g["pos_liberties"][k]), name
        assert np.array_equal(G.liberties(b), g["pos_liberties"][k]), name


def test_legal_and_suicide_maps_are_the_reference(g):
    for k, (name, b, ko, player) in enumerate(positions(g)):
        # the host functions on every point of the small cases, on a sample of the large ones (each call is a flood fill)
        pts = range(P) if (b != 0).sum() < 12 or k % 4 == 0 else range(k % 5, P, 5)
        for p in pts:
            assert darknet.legal_go(b, ko, player, p // 19, p % 19) == g["pos_legal"][k][p], (name, p)
            assert darknet.suicide_go(b, player, p // 19, p % 19) == g["pos_suicide"][k][p], (name, p)


def test_the_rule_gives_the_reference_maps(g):
    for k, (name, b, ko, player) in enumerate(positions(g)):
        if k % 3 and (b != 0).sum() > 100:
            continue                            # the rule is a Python flood fill per point: a third of the large boards
        assert np.array_equal(G.legal_map(b, ko, player), g["pos_legal"][k]), name
        assert np.array_equal(G.suicide_map(b, player), g["pos_suicide"][k]), name


def test_move_go_is_the_reference(g):
    pos = positions(g)
    for k, at, after in zip(g["move_pos"], g["move_at"], g["move_after"]):
        _, b, _, player = pos[k]
        assert np.array_equal(darknet.move_go(b, player, at // 19, at % 19), after), (pos[k][0], at)
        assert np.array_equal(G.move(b, player, at // 19, at % 19), after), (pos[k][0], at)


def test_flip_board():
    b = synth.go_boards(3, 1)[0]
    c = b.copy()
    darknet.lib().flip_board(c.ctypes.data_as(C.c_void_p))
    assert np.array_equal(c, -b)


def test_load_go_moves_reads_94_byte_lines(g, tmp_path):
    path = os.path.join(str(tmp_path), "three.moves")
    with open(path, "wb") as f:
        for r in g["load_records"]:
            f.write(r.tobytes() + b"\n")
        f.write(b"short tail")
    assert np.array_equal(darknet.load_go_moves(path), g["load_records"])
    with pytest.raises(darknet.Y2Error, match="Couldn't open"):
        darknet.load_go_moves(os.path.join(str(tmp_path), "absent"))


def test_draw_moves_are_the_reference_draws(g):
    darknet.srand(int(g["batch_seed"]))
    pick, flip, rot = darknet.go_draw_moves(len(g["game_records"]), 4)
    assert np.array_equal(pick, g["batch_pick"]) and np.array_equal(flip, g["batch_flip"]) and np.array_equal(rot, g["batch_rot"])
    with pytest.raises(darknet.Y2Error, match="n_records"):
        darknet.go_draw_moves(0, 4)


def test_the_rule_gives_the_reference_batch(g):
    x, y = G.loader(g["game_records"], g["batch_pick"], g["batch_flip"], g["batch_rot"])
    assert np.array_equal(x, g["batch_x"]) and np.array_equal(y, g["batch_y"])
    assert g["batch_flip"].any() and (g["batch_rot"] % 2).any(), "the batch draws no flip or no odd turn"


def test_the_rule_picks_what_the_reference_picked(g):
    pos = positions(g)
    for i, name in enumerate(g["pick_names"]):
        _, b, ko, _ = pos[g["pick_pos"][i]]
        player = int(g["pick_players"][i])
        index, kept = G.pick(g["pick_move"][i], G.legal_map(b, ko, player), G.suicide_map(b, player), g["pick_thresh"][i], g["pick_u"][i])
        assert index == g["pick_index"][i] and np.array_equal(kept, g["pick_kept"][i]), name


def test_views_and_merge_of_the_rule_invert_each_other():
    a = np.arange(P, dtype=np.float32)
    for i in range(8):
        assert np.array_equal(G.unview(G.view(a, i), i), a)
        assert not np.array_equal(G.view(a, i), a) or i == 0
    # rotate_image_cw read from its assignments: one turn is new[r][c] = old[c][18-r]
    assert G.view(a, 1).reshape(19, 19)[2, 5] == a.reshape(19, 19)[5, 16]


# what is asked -> a word of the message; all of it is refused on the arguments alone
REFUSALS = {
    "input is not 19 x 19 x 1": "reads 19 x 19 x 1",
    "output is not 361 values": "gives 361",
    "board value 2": "boards: board 1 holds 2",
    "board value nan": "boards: board 0 holds nan",
    "player 0": "players: player 0",
    "n = 0": "n = 0",
    "fp16 mode": "fp16 mode",
    "games = 0": "games = 0",
    "rules with player 2": "players: player 2",
    "generate_move with a bad board": "generate_move: boards",
    "loader pick outside": "pick: item 1",
    "loader rot 4": "rot: item 0",
    "loader row 19": "records: record 0",
}


def refusal(tmp, what):
    """(network, call) -- the call must raise darknet.Y2Error with REFUSALS[what]"""
    boards = np.zeros((2, P), np.float32)
    players = np.array([1, -1], np.int32)
    u = np.zeros(2, np.float32)
    if what == "input is not 19 x 19 x 1":
        net = go_net(tmp, text=zoo.cfg_text("mini", 32, 32, 1))
        return net, lambda: net.go_predict(boards, players)
    if what == "output is not 361 values":
        spec = [("conv", 8, 3, 1, "relu"), ("avg",), ("softmax",)]
        net = go_net(tmp, text=zoo.cfg_text("go-8", 19, 19, 1, spec=spec).replace("channels=3", "channels=1"))
        return net, lambda: net.go_generate(boards, None, players, False, .1, .7, u)
    if what.startswith("loader"):
        net = go_net(tmp, batch=2)
        rec = np.zeros((3, 93), np.uint8)
        if what == "loader row 19":
            rec[0, 0] = 19
        pick = [0, 3] if what == "loader pick outside" else [0, 1]
        rot = [4, 0] if what == "loader rot 4" else [0, 1]
        return net, lambda: net.train_load_go(rec, pick, [0, 1], rot)
    net = go_net(tmp)
    if what == "board value 2":
        boards[1, 200] = 2
        return net, lambda: net.go_predict(boards, players)
    if what == "board value nan":
        boards[0, 0] = np.nan
        return net, lambda: net.go_generate(boards, None, players, True, .1, .7, u)
    if what == "player 0":
        return net, lambda: net.go_predict(boards, [1, 0])
    if what == "n = 0":
        return net, lambda: _raw_predict(net, 0)
    if what == "fp16 mode":
        net.set_half(True)
        return net, lambda: net.go_predict(boards, players)
    if what == "games = 0":
        return net, lambda: net.go_selfplay(0, 12, np.zeros(0, np.float32))
    if what == "rules with player 2":
        return net, lambda: net.go_rules(boards, None, [1, 2])
    boards[0, 5] = .5
    return net, lambda: net.generate_move(1, boards[0], False, .1, .7, bytes(91))


def _raw_predict(net, n):
    b, p, out = np.zeros(P, np.float32), np.ones(1, np.int32), np.zeros(P, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if darknet.lib().y2_go_predict(net.net, vp(b), vp(p), n, 0, vp(out)) != 0:
        raise darknet.Y2Error("y2_go_predict: " + darknet._check())


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_argument(tmp_path, what):
    net, call = refusal(tmp_path, what)
    syncs = darknet.stream_syncs()
    with pytest.raises(darknet.Y2Error, match=REFUSALS[what]):
        call()
    assert darknet.stream_syncs() == syncs, "a refused call waited on the device"
    net.free()


def test_a_refused_generate_move_draws_nothing(tmp_path):
    net = go_net(tmp_path)
    libc = C.CDLL(None)
    darknet.srand(5)
    want = libc.rand()
    darknet.srand(5)
    bad = np.zeros(P, np.float32)
    bad[7] = 3
    with pytest.raises(darknet.Y2Error):
        net.generate_move(1, bad, False, .1, .7, bytes(91))
    assert libc.rand() == want
    net.free()
