#!/usr/bin/env python3
"""What a generated Go move costs on the device, on go.test.cfg's topology (zoo "go") with synthetic weights, multi = 1.

    python tools/go_latency.py [--iters 200] [--out profiles/go_stage.txt] [--no-selfplay]

One generated move at n = 1, network at batch 8 (one forward for the eight views), default mode:
  * the wall time of y2_go_generate (host clock around a call that ends in its one device sync), p50 / p95;
  * device time (HIP events around 100 back-to-back repetitions on the engine's stream) of the forward alone, and of the
    part that is not the forward -- views, merge, rules, pick through their kernel-level entries -- on the same position;
  * beside them what a caller could assemble without the Go entries: network_predict at batch 8 (wall) plus the rules on
    the host, timed by the compiled reference's own 361 legal_go + 2 suicide_go per move through oracle/_ref/go_ref
    (tests/golden/gen_go_golden.py --driver-only builds it where the reference checkout exists; absent: "not measured").
Positions: a mid-game position of at least 216 stones reached by seeded random non-suicidal play, and the empty board.
Self-play: plies per second of y2_go_selfplay at 1, 8 and 64 games, max_moves 300, with and without polling for
"all games over" every 16 plies."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet, synth, zoo  # noqa: E402

P, KO = 361, 91
GO_REF = os.path.join(ROOT, "oracle", "_ref", "go_ref")


def go_net(tmp, batch):
    cfg, wts = os.path.join(tmp, "go_b%d.cfg" % batch), os.path.join(tmp, "go.weights")
    with open(cfg, "w") as f:
        f.write(zoo.go_cfg_text("go", batch))
    if not os.path.exists(wts):
        synth.write_go_weights(wts, "go", 32)
    net = darknet.Network.parse_network_cfg(cfg)
    net.load_weights(wts)
    return net


def midgame(net, stones, seed=216):
    """seeded random non-suicidal play until the board holds `stones` stones; the maps come from y2_go_rules"""
    rng = np.random.RandomState(seed)
    board, player, ko = np.zeros(P, np.float32), 1, [bytes(KO), bytes(KO)]
    for t in range(2000):
        if int((board != 0).sum()) >= stones:
            break
        _, legal, sui = net.go_rules(board, ko[t & 1], [player])
        cand = np.flatnonzero((legal[0] == 1) & (sui[0] == 0))
        if not len(cand):
            break
        at = int(cand[rng.randint(len(cand))])
        board = darknet.move_go(board, player, at // 19, at % 19)
        ko[t & 1] = darknet.board_to_string(board)
        player = -player
    return board, ko[t & 1], player


class Events:
    def __init__(self, net):
        self.L, self.s = darknet.lib(), C.c_void_p(net.stream())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        self.L.y2h_event_create(C.byref(self.e0))
        self.L.y2h_event_create(C.byref(self.e1))
        self.net = net

    def us_per(self, fn, reps=100):
        fn()
        self.net.sync()
        self.L.y2h_event_record(self.e0, self.s)
        for _ in range(reps):
            fn()
        self.L.y2h_event_record(self.e1, self.s)
        self.net.sync()
        ms = C.c_float()
        self.L.y2h_event_elapsed_ms(self.e0, self.e1, C.byref(ms))
        return ms.value * 1e3 / reps


def put(L, a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert L.y2h_malloc(C.byref(p), max(a.nbytes, 16)) == 0
    assert L.y2h_memcpy_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
    return p


def reference_rules_ms(tmp, positions):
    if not os.path.exists(GO_REF):
        return None
    path = os.path.join(tmp, "time.in")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(positions)))
        for b, ko, player in positions:
            f.write(np.asarray(b, np.float32).tobytes() + bytes(ko) + struct.pack("<i", player))
    r = subprocess.run([GO_REF, "time", path], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return None
    return [float(line.split(":")[1].split("ms")[0]) for line in r.stdout.strip().splitlines() if line.startswith("position")]


def one_move(tmp, iters, lines):
    L = darknet.lib()
    net = go_net(tmp, 8)
    net.go_predict(np.zeros(P, np.float32), [1], True)
    mid = midgame(net, 216)
    cases = [("midgame_%d_stones" % int((mid[0] != 0).sum()), mid), ("empty_board", (np.zeros(P, np.float32), bytes(KO), 1))]
    ref = reference_rules_ms(tmp, [c for _, c in cases])
    ev = Events(net)
    s = ev.s
    x = synth.go_boards(3, 8)
    ts = []
    for i in range(iters + 20):                     # the composition's forward: network_predict at batch 8, wall
        t0 = time.perf_counter()
        net.network_predict(x.reshape(8, 1, 19, 19))
        if i >= 20:
            ts.append(time.perf_counter() - t0)
    predict_us = float(np.percentile(np.array(ts) * 1e6, 50))
    d_x = put(L, x)
    forward_us = ev.us_per(lambda: net.forward_device(d_x.value))
    for k, (name, (board, ko, player)) in enumerate(cases):
        u = np.array([.37], np.float32)
        ts = []
        for i in range(iters + 20):
            t0 = time.perf_counter()
            net.go_generate(board, ko, [player], True, .1, .7, u)
            if i >= 20:
                ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e6
        d_b, d_k, d_p, d_u = put(L, board), put(L, np.frombuffer(ko, np.uint8)), put(L, np.array([player], np.int32)), put(L, u)
        d_rows, d_views = put(L, np.full((8, P), 1 / P, np.float32)), put(L, np.zeros((8, P), np.float32))
        d_move, d_legal, d_sui, d_idx = (put(L, np.zeros(P, t)) for t in (np.float32, np.uint8, np.uint8, np.int32))

        def rest():
            L.y2h_go_views(d_b, d_p, 1, 1, d_views, s)
            L.y2h_go_merge(d_rows, P, d_b, 1, 1, d_move, s)
            L.y2h_go_rules(d_b, d_k, d_p, 1, None, d_legal, d_sui, s)
            L.y2h_go_pick(d_move, P, d_legal, d_sui, 1, .1, d_u, d_idx, None, s)
        rest_us = ev.us_per(rest)
        rules_us = ev.us_per(lambda: L.y2h_go_rules(d_b, d_k, d_p, 1, None, d_legal, d_sui, s))
        pick_us = ev.us_per(lambda: L.y2h_go_pick(d_move, P, d_legal, d_sui, 1, .1, d_u, d_idx, None, s))
        for p in (d_b, d_k, d_p, d_u, d_rows, d_views, d_move, d_legal, d_sui, d_idx):
            L.y2h_free(p)
        host_ms = ref[k] if ref else None
        out = dict(case=name, generate_wall_p50_us=round(float(np.percentile(ts, 50)), 1), generate_wall_p95_us=round(float(np.percentile(ts, 95)), 1),
                   forward_b8_device_us=round(forward_us, 1), views_merge_rules_pick_device_us=round(rest_us, 1),
                   rules_device_us=round(rules_us, 1), pick_device_us=round(pick_us, 1), network_predict_b8_wall_p50_us=round(predict_us, 1),
                   reference_host_rules_us=round(host_ms * 1e3, 1) if host_ms else "not measured")
        if host_ms:
            out["non_forward_share_below_host_rules"] = bool(rest_us < host_ms * 1e3)
            out["chain_below_predict_plus_host_rules"] = bool(out["generate_wall_p50_us"] < predict_us + host_ms * 1e3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    L.y2h_free(d_x)
    net.free()


def selfplay(tmp, lines, max_moves=300):
    for games in (1, 8, 64):
        net = go_net(tmp, games * 8)
        u = darknet.Network.rnn_uniforms(games, games * max_moves)
        net.go_selfplay(games, 8, u[:games * 8], multi=True)           # warm-up: the plan, every kernel
        out = dict(selfplay_games=games, max_moves=max_moves)
        for poll in (0, 16):
            net.go_set_poll(poll)
            t0 = time.perf_counter()
            _, counts, _ = net.go_selfplay(games, max_moves, u, multi=True)
            dt = time.perf_counter() - t0
            out["plies_per_s_poll_%d" % poll] = round(float(counts.sum()) / dt, 1)
            out["plies_poll_%d" % poll] = int(counts.sum())
            out["seconds_poll_%d" % poll] = round(dt, 3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        net.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-selfplay", action="store_true")
    a = ap.parse_args()
    if darknet.device_count() < 1:
        sys.exit("go_latency: no HIP device visible (a timing needs the GPU)")
    lines = ["# tools/go_latency.py on %s: zoo 'go' (go.test.cfg's topology), synthetic weights, multi = 1, default mode" % darknet.device_name()]
    with tempfile.TemporaryDirectory() as tmp:
        one_move(tmp, a.iters, lines)
        if not a.no_selfplay:
            selfplay(tmp, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
