"""Go on the device against the compiled reference's fixture (tests/golden/go.npz) and the numpy statement the host test
holds to it (tests/go_rule.py): the kernels one by one through the C-ABI, then predict_move / generate_move and the
batched entries.  Strict mode reproduces the reference's rows and decisions bit for bit; default mode keeps each row
within the bound the project holds softmax rows to, 1e-4 x the row's maximum per value (tests/chargen_rule.py margin_bar)."""
import ctypes as C

import numpy as np
import pytest

from sr_object_detection_amd import darknet, synth
from tests import go_rule as G
from tests.helpers import load_golden
from tests.test_go_host import REFUSALS, go_net, positions, refusal

pytestmark = pytest.mark.gpu

P, KO, REC = G.P, G.KO, G.REC


@pytest.fixture(scope="module")
def g():
    return load_golden("go")


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

    def new(self, shape, dtype, fill=0x5a):
        return self.put(np.full(shape, fill, np.uint8).repeat(np.dtype(dtype).itemsize, axis=-1))

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


# ---- 1. views and merge ----
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("multi", [0, 1])
def test_views_and_merge_are_the_rule(dev, n, multi):
    V = 8 if multi else 1
    boards = synth.uniform(400 + n, n * P, -1, 1).reshape(n, P)          # asymmetric: no view equals another
    boards[:, 1::2] = 0
    players = np.array([1, -1, -1][:n], np.int32)
    x = dev.new((n * V, P), np.float32)
    assert dev.L.y2h_go_views(dev.put(boards), dev.put(players), n, multi, x, None) == 0
    assert np.array_equal(dev.get(x, (n * V, P)), G.views(boards, players, multi))
    # rows of very different sizes: a wrong summation order rounds differently, a wrong inverse moves values
    scale = np.repeat(10. ** (np.arange(n * V) % 8), P).astype(np.float32)
    rows = (synth.uniform(500 + n, n * V * P, 0, 1) * scale).astype(np.float32).reshape(n * V, P)
    move = dev.new((n, P), np.float32)
    assert dev.L.y2h_go_merge(dev.put(rows), P, dev.put(boards), n, multi, move, None) == 0
    want = G.merge(rows, boards, multi)
    assert np.array_equal(dev.get(move, (n, P)), want) and (want[boards != 0] == 0).all() and (want[boards == 0] != 0).all()


# ---- 2. the rules ----
def _rules(dev, boards, ko, players):
    n = len(players)
    lib, legal, sui = dev.new((n, P), np.int32), dev.new((n, P), np.uint8), dev.new((n, P), np.uint8)
    assert dev.L.y2h_go_rules(dev.put(boards.astype(np.float32)), dev.put(ko), dev.put(players.astype(np.int32)), n, lib, legal, sui, None) == 0
    return dev.get(lib, (n, P), np.int32), dev.get(legal, (n, P), np.uint8), dev.get(sui, (n, P), np.uint8)


def test_rules_are_the_reference_in_any_grouping(dev, g):
    boards, ko, players = g["pos_boards"], g["pos_ko"], g["pos_players"]
    n = len(players)
    for order in (np.arange(n), np.arange(n)[::-1]):
        lib, legal, sui = _rules(dev, boards[order], ko[order], players[order])
        assert np.array_equal(lib, g["pos_liberties"][order]), "liberties"
        assert np.array_equal(legal, g["pos_legal"][order]), "legal: %s" % g["pos_names"][order][np.flatnonzero((legal != g["pos_legal"][order]).any(1))]
        assert np.array_equal(sui, g["pos_suicide"][order]), "suicide"
    for k in range(n):
        lib, legal, sui = _rules(dev, boards[k:k + 1], ko[k:k + 1], players[k:k + 1])
        assert np.array_equal(lib[0], g["pos_liberties"][k]) and np.array_equal(legal[0], g["pos_legal"][k]) and \
            np.array_equal(sui[0], g["pos_suicide"][k]), g["pos_names"][k]


def test_rules_outputs_may_be_null_and_ko_too(dev, g):
    k = list(g["pos_names"]).index("ko_zero_string")
    b, p = dev.put(g["pos_boards"][k:k + 1].astype(np.float32)), dev.put(g["pos_players"][k:k + 1])
    legal = dev.new((1, P), np.uint8)
    assert dev.L.y2h_go_rules(b, None, p, 1, None, legal, None, None) == 0
    assert np.array_equal(dev.get(legal, (1, P), np.uint8)[0], g["pos_legal"][k])


def test_apply_is_move_go_and_board_to_string(dev, g):
    k, at = g["move_pos"], g["move_at"]
    boards = dev.put(g["pos_boards"][k].astype(np.float32))
    strings = dev.new((len(k), KO), np.uint8)
    assert dev.L.y2h_go_apply(boards, dev.put(g["pos_players"][k]), dev.put(at), len(k), strings, None) == 0
    assert np.array_equal(dev.get(boards, (len(k), P)), g["move_after"])
    assert np.array_equal(dev.get(strings, (len(k), KO), np.uint8), g["move_string"])
    # a move of -1 leaves the board and packs it
    assert dev.L.y2h_go_apply(boards, dev.put(g["pos_players"][k]), dev.put(np.full(len(k), -1, np.int32)), len(k), strings, None) == 0
    assert np.array_equal(dev.get(boards, (len(k), P)), g["move_after"])
    assert np.array_equal(dev.get(strings, (len(k), KO), np.uint8), g["move_string"])


# ---- 3. the decision ----
def test_pick_decides_as_generate_move(dev, g):
    pos = positions(g)
    n = len(g["pick_names"])
    legal, sui = np.zeros((n, P), np.uint8), np.zeros((n, P), np.uint8)
    for i in range(n):
        _, b, ko, _ = pos[g["pick_pos"][i]]
        legal[i], sui[i] = G.legal_map(b, ko, int(g["pick_players"][i])), G.suicide_map(b, int(g["pick_players"][i]))
    for thresh in sorted(set(g["pick_thresh"].tolist())):
        sel = np.flatnonzero(g["pick_thresh"] == np.float32(thresh))
        index, kept = dev.new((len(sel),), np.int32), dev.new((len(sel), P), np.float32)
        assert dev.L.y2h_go_pick(dev.put(g["pick_move"][sel]), P, dev.put(legal[sel]), dev.put(sui[sel]), len(sel), thresh,
                                 dev.put(g["pick_u"][sel]), index, kept, None) == 0
        assert np.array_equal(dev.get(index, (len(sel),), np.int32), g["pick_index"][sel]), g["pick_names"][sel]
        assert np.array_equal(dev.get(kept, (len(sel), P)), g["pick_kept"][sel]), g["pick_names"][sel]


def test_decode_and_argmax(dev, g):
    rec = g["game_records"]
    boards, index = dev.new((len(rec), P), np.float32), dev.new((len(rec),), np.int32)
    assert dev.L.y2h_go_decode(dev.put(rec), None, None, None, len(rec), boards, None, None) == 0
    got = dev.get(boards, (len(rec), P))
    assert np.array_equal(got, np.array([G.unpack(r[2:].tobytes()) for r in rec]))
    rows = synth.uniform(9, 5 * P, 0, 1).reshape(5, P)
    rows[1, [40, 300]] = 2                       # the first maximum
    assert dev.L.y2h_go_argmax(dev.put(rows), P, 5, index, None) == 0
    assert np.array_equal(dev.get(index, (5,), np.int32), rows.argmax(1)) and rows.argmax(1)[1] == 40


# ---- 4 / 5. predict ----
def _predict_case(g, key):
    pos = positions(g)
    ks = g[key + "_predict_pos"]
    return (np.array([pos[k][1] for k in ks]), np.array([pos[k][3] for k in ks], np.int32), g[key + "_predict_multi"], g[key + "_predict_rows"])


@pytest.mark.parametrize("batch", [1, 8])
def test_predict_strict_is_the_reference_mini(tmp_path, g, batch):
    boards, players, multi, rows = _predict_case(g, "mini")
    net = go_net(tmp_path, "go-mini", batch, int(g["wseed_mini"]))
    net.set_strict(True)
    for m in (0, 1):
        sel = np.flatnonzero(multi == m)
        assert np.array_equal(net.go_predict(boards[sel], players[sel], m), rows[sel]), "n = 3, multi = %d" % m
        for i in sel:
            assert np.array_equal(net.go_predict(boards[i], players[i:i + 1], m)[0], rows[i]), "n = 1, multi = %d" % m
            assert np.array_equal(net.predict_move(boards[i] * players[i], m), rows[i]), "predict_move, multi = %d" % m
    net.free()


def test_predict_strict_is_the_reference_go(tmp_path, g):
    boards, players, multi, rows = _predict_case(g, "go")
    net = go_net(tmp_path, "go", 8, int(g["wseed_go"]))
    net.set_strict(True)
    for i in range(len(multi)):
        assert np.array_equal(net.go_predict(boards[i], players[i:i + 1], int(multi[i]))[0], rows[i]), "multi = %d" % multi[i]
    net.free()


@pytest.mark.parametrize("name,batch", [("go-mini", 1), ("go-mini", 8), ("go", 8)])
def test_predict_default_mode_keeps_the_softmax_bound(tmp_path, g, name, batch):
    key = "mini" if name == "go-mini" else "go"
    boards, players, multi, rows = _predict_case(g, key)
    net = go_net(tmp_path, name, batch, int(g["wseed_" + key]))
    for i in range(len(multi)):
        got = net.go_predict(boards[i], players[i:i + 1], int(multi[i]))[0]
        err, bar = float(np.abs(got - rows[i]).max()), 1e-4 * float(rows[i].max())
        print("%s batch %d multi %d: max |got - ref| = %.3g, bound %.3g" % (name, batch, multi[i], err, bar))
        assert err <= bar and np.array_equal(got == 0, rows[i] == 0)
    net.free()


# ---- 6. generate ----
def test_generate_move_is_the_reference(tmp_path, g):
    pos = positions(g)
    net = go_net(tmp_path, "go-mini", 8, int(g["wseed_mini"]))
    net.set_strict(True)
    net.go_predict(np.zeros(P, np.float32), [1])             # the runtime is up: nothing but generate_move draws from rand() now
    ks = g["mini_gen_pos"]
    assert -1 in g["mini_gen_index"] and {pos[k][3] for k in ks} == {1, -1} and "ko_forbidden" in [pos[k][0] for k in ks]
    for i, k in enumerate(ks):
        _, b, ko, player = pos[k]
        multi, thresh, temp = int(g["mini_gen_multi"][i]), float(g["mini_gen_thresh"][i]), float(g["mini_gen_temp"][i])
        darknet.srand(int(g["mini_gen_seed"][i]))
        assert net.generate_move(player, b, multi, thresh, temp, ko) == g["mini_gen_index"][i], pos[k][0]
        assert all(net.net.layers[j].temperature == np.float32(temp) for j in range(net.net.n)), "temp must be on every layer"
        got = net.go_generate(b, ko, [player], multi, thresh, temp, g["mini_gen_u"][i:i + 1])
        assert got[0] == g["mini_gen_index"][i], pos[k][0]
    # the cases that share their settings, as one batch
    same = [i for i in range(len(ks)) if (g["mini_gen_multi"][i], g["mini_gen_thresh"][i], g["mini_gen_temp"][i]) == (0, np.float32(.1), np.float32(.7))]
    assert len(same) >= 3
    got = net.go_generate(np.array([pos[ks[i]][1] for i in same]), b"".join(pos[ks[i]][2] for i in same), [pos[ks[i]][3] for i in same],
                          0, .1, .7, g["mini_gen_u"][same])
    assert np.array_equal(got, g["mini_gen_index"][same])
    net.free()


def test_generate_move_on_go_test_cfg(tmp_path, g):
    pos = positions(g)
    net = go_net(tmp_path, "go", 8, int(g["wseed_go"]))
    net.set_strict(True)
    _, b, ko, player = pos[int(g["go_gen_pos"])]
    assert net.go_generate(b, ko, [player], 1, .1, .7, [float(g["go_gen_u"])])[0] == g["go_gen_index"]
    net.free()


# ---- 7. self-play ----
def _alone(net, seed, plies, multi, thresh, temp):
    """one game through the exported generate_move + move_go, driven as go.c:775-823 drives it"""
    board, player, one, two, recs = np.zeros(P, np.float32), 1, bytes(KO), bytes(KO), []
    darknet.srand(seed)
    while len(recs) < plies:
        index = net.generate_move(player, board, multi, thresh, temp, two)
        if index < 0:
            break
        one, two = two, one
        recs.append(bytes([index // 19, index % 19]) + darknet.board_to_string(board * player + 0))
        board = darknet.move_go(board, player, index // 19, index % 19)
        one = darknet.board_to_string(board)
        player = -player
    return np.frombuffer(b"".join(recs), np.uint8).reshape(-1, REC), board


def test_selfplay_is_the_reference_game_and_each_game_alone(tmp_path, g):
    G_, M = 3, 12
    net = go_net(tmp_path, "go-mini", 8, int(g["wseed_mini"]))
    net.set_strict(True)
    net.go_predict(np.zeros(P, np.float32), [1])
    seeds = [7, 1001, 1002]
    u = np.array([darknet.Network.rnn_uniforms(s, M) for s in seeds])
    assert np.array_equal(u[0], g["game_u"]), "the fixture game's draws are srand(7)'s"
    rec, counts, final = net.go_selfplay(G_, M, u, multi=True, thresh=.1, temp=.7)
    assert counts[0] == len(g["game_records"]) and np.array_equal(rec[0, :counts[0]], g["game_records"])
    assert np.array_equal(final[0], g["game_final"])
    for i, s in enumerate(seeds):
        r, b = _alone(net, s, M, True, .1, .7)
        assert counts[i] == len(r) and np.array_equal(rec[i, :counts[i]], r) and np.array_equal(final[i], b), "game %d" % i
    net.go_set_poll(4)                                       # asking whether all games are over changes nothing
    rec2, counts2, final2 = net.go_selfplay(G_, M, u, multi=True, thresh=.1, temp=.7)
    assert np.array_equal(rec2, rec) and np.array_equal(counts2, counts) and np.array_equal(final2, final)
    net.free()


def test_two_networks_alternate(tmp_path, g):
    a = go_net(tmp_path, "go-mini", 8, int(g["wseed_mini"]))
    b = go_net(tmp_path, "go-mini", 8, 77)
    for n in (a, b):
        n.set_strict(True)
    u = darknet.Network.rnn_uniforms(5, 2 * 6).reshape(2, 6)
    rec, counts, final = a.go_selfplay(2, 6, u, other=b, first=1)
    # by hand: b moves first
    for i in range(2):
        board, player, ko = np.zeros(P, np.float32), 1, [bytes(KO), bytes(KO)]
        for t in range(6):
            net = b if t % 2 == 0 else a
            index = int(net.go_generate(board, ko[t & 1], [player], False, .1, .7, u[i, t:t + 1])[0])
            assert index >= 0 and int(rec[i, t, 0]) * 19 + int(rec[i, t, 1]) == index
            board = darknet.move_go(board, player, index // 19, index % 19)
            ko[t & 1] = darknet.board_to_string(board)
            player = -player
        assert counts[i] == 6 and np.array_equal(final[i], board)
    a.free()
    b.free()


def test_a_game_that_ends_keeps_its_records(dev, g):
    """y2h_go_play, the kernel self-play advances with: a -1 ends a game for good"""
    pos = positions(g)
    k = [list(g["pos_names"]).index(n) for n in ("play_903_40", "double_capture", "ko_zero_string")]
    start = np.array([pos[i][1] for i in k])
    free = [np.flatnonzero(g["pos_legal"][i]) for i in k]
    M = 4
    boards, ko = dev.put(start), dev.put(np.zeros((2, 3, KO), np.uint8))
    alive, counts = dev.put(np.ones(3, np.int32)), dev.put(np.zeros(3, np.int32))
    records = dev.put(np.zeros((3, M, REC), np.uint8))
    first = np.array([free[0][0], -1, free[2][0]], np.int32)
    assert dev.L.y2h_go_play(boards, ko, 1, dev.put(first), alive, records, counts, M, 3, None) == 0
    after1 = dev.get(boards, (3, P))
    assert np.array_equal(dev.get(alive, (3,), np.int32) != 0, [True, False, True])
    assert np.array_equal(after1[1], start[1]) and np.array_equal(after1[0], G.move(start[0], 1, first[0] // 19, first[0] % 19))
    second = np.array([-1, free[1][0], np.flatnonzero(after1[2] == 0)[3]], np.int32)       # game 1 is over: its move must be ignored
    assert dev.L.y2h_go_play(boards, ko, -1, dev.put(second), alive, records, counts, M, 3, None) == 0
    after2, rec = dev.get(boards, (3, P)), dev.get(records, (3, M, REC), np.uint8)
    assert np.array_equal(dev.get(counts, (3,), np.int32), [1, 0, 2])
    assert np.array_equal(after2[0], after1[0]) and np.array_equal(after2[1], start[1])
    assert np.array_equal(after2[2], G.move(after1[2], -1, second[2] // 19, second[2] % 19))
    assert not rec[1].any() and not rec[0, 1:].any()
    assert rec[0, 0].tobytes() == bytes([first[0] // 19, first[0] % 19]) + G.pack(start[0])
    assert rec[2, 1].tobytes() == bytes([second[2] // 19, second[2] % 19]) + G.pack(-after1[2])   # the mover's side
    assert dev.get(ko, (2, 3, KO), np.uint8)[0, 2].tobytes() == G.pack(after2[2])


# ---- 8. valid ----
@pytest.mark.parametrize("batch", [1, 8])
def test_valid_is_the_reference(tmp_path, g, batch):
    net = go_net(tmp_path, "go-mini", batch, int(g["wseed_mini"]))
    net.set_strict(True)
    for multi in (0, 1):
        assert np.array_equal(net.go_valid(g["valid_records"], multi), g["valid_predicted"][multi]), "multi = %d" % multi
    net.free()


# ---- 9. the training loader ----
def test_train_load_go_builds_the_reference_batch_and_steps(tmp_path, g):
    net = go_net(tmp_path, "go-mini", 4, int(g["wseed_mini"]))
    net.train_load_go(g["game_records"], g["batch_pick"], g["batch_flip"], g["batch_rot"])
    x, y = net.train_pull_input()
    assert np.array_equal(x.reshape(4, P), g["batch_x"]) and np.array_equal(y.reshape(4, P), g["batch_y"])
    assert (y.reshape(4, P).sum(1) == 1).all()
    loss = net.train_step_loaded()
    assert np.isfinite(loss) and loss > 0
    net.free()


# ---- 10. refusals ----
@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_leave_the_network_usable(tmp_path, what):
    net, call = refusal(tmp_path, what)
    with pytest.raises(darknet.Y2Error, match=REFUSALS[what]):
        call()
    net.set_half(False)
    if net.net.w == 19 and net.output_size == P:
        out = net.go_predict(np.zeros(P, np.float32), [1])
    else:
        out = net.network_predict(synth.image_batch(net.net.batch, net.net.c, net.net.h, net.net.w))
    assert np.isfinite(out).all() and out.any()
    net.free()
