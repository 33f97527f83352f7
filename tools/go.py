#!/usr/bin/env python3
"""go.c's verbs valid, self and train (src_yolo2/go.c:402, :748, :118) as thin loops over the batched entries.

valid  y2_go_valid over a file of records, --chunk records per call; prints the running accuracy as valid_go does.
self   y2_go_selfplay: --games games in lockstep per round, at most --max-moves plies each (the reference's cap is 300),
       thresh .1 and temp .7 as self_go passes them.  The reference scores a finished game by piping it to gnugo and
       prints the winner's records; that stays out: every game's records are written, 94 bytes each (the record and a
       newline), the file format load_go_moves reads.  Rounds alternate which network moves first, as self_go's `total`
       does.  The uniforms come from libc rand(), srand(time) unless --seed.
train  random_go_moves' draws (y2_go_draw_moves) -> y2_train_load_go -> y2_train_step_loaded, the loss divided by the
       batch with train_go's .95 / .05 running average; weights saved as train_go saves them, into --backup DIR.

usage: go.py valid CFG WEIGHTS MOVES [--multi] [--chunk 256]
       go.py self CFG [WEIGHTS [CFG2 [WEIGHTS2]]] [--multi] [--games 8] [--rounds 1] [--max-moves 300] [--out FILE] [--seed N] [--poll N]
       go.py train CFG MOVES --backup DIR [--weights FILE] [--seed N] [--max-steps N]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sr_object_detection_amd import darknet  # noqa: E402


def open_net(cfg, weights, batch=None):
    net = darknet.Network.parse_network_cfg(cfg)
    if weights:
        net.load_weights(weights)
    if batch:
        net.set_batch_network(batch)
    return net


def valid(a):
    rec = darknet.load_go_moves(a.moves)
    net = open_net(a.cfg, a.weights, 8 if a.multi else 1)      # one forward per record with --multi, as valid_go's batch 1 otherwise
    correct = 0
    for at in range(0, len(rec), a.chunk):
        part = rec[at:at + a.chunk]
        got = net.go_valid(part, a.multi)
        for i, (r, p) in enumerate(zip(part, got)):
            correct += int(p) == int(r[0]) * 19 + int(r[1])
            print("%d Accuracy %f" % (at + i, correct / (at + i + 1)))


def self_play(a):
    libc = ctypes.CDLL(None)
    net = open_net(a.cfg, a.weights, a.games * (8 if a.multi else 1))
    net2 = open_net(a.cfg2, a.weights2, a.games * (8 if a.multi else 1)) if a.cfg2 else None
    net.go_predict(np.zeros(361, np.float32), [1])             # the runtime draws from rand() while it starts: seed behind it
    libc.srand(ctypes.c_uint(int(time.time()) if a.seed is None else a.seed))
    if a.poll:
        net.go_set_poll(a.poll)
    out = open(a.out, "ab") if a.out else None
    plies, t0 = 0, time.time()
    for rnd in range(a.rounds):
        u = np.array([libc.rand() for _ in range(a.games * a.max_moves)], np.float32) / np.float32(2147483647)
        rec, counts, boards = net.go_selfplay(a.games, a.max_moves, u, a.multi, .1, .7, other=net2, first=rnd % 2 if net2 else 0)
        plies += int(counts.sum())
        for g in range(a.games):
            stones = int((boards[g] == 1).sum()), int((boards[g] == -1).sum())
            print("round %d game %d: %d moves, %d black and %d white stones left" % (rnd, g, counts[g], stones[0], stones[1]), file=sys.stderr)
            for r in rec[g, :counts[g]]:
                if out:
                    out.write(r.tobytes() + b"\n")
    dt = time.time() - t0
    print("%d plies in %.2f s: %.0f plies/s" % (plies, dt, plies / dt), file=sys.stderr)


def train(a):
    libc = ctypes.CDLL(None)
    rec = darknet.load_go_moves(a.moves)
    if not len(rec):
        sys.exit("%s holds no record" % a.moves)
    os.makedirs(a.backup, exist_ok=True)
    base = os.path.splitext(os.path.basename(a.cfg))[0]
    net = open_net(a.cfg, a.weights)
    n = net.net
    print("Learning Rate: %g, Momentum: %g, Decay: %g" % (n.learning_rate, n.momentum, n.decay), file=sys.stderr)
    net.train_prepare()
    libc.srand(ctypes.c_uint(int(time.time()) if a.seed is None else a.seed))
    avg, ran, epoch = -1., 0, n.seen[0] // len(rec)
    while (net.get_current_batch() < n.max_batches or n.max_batches == 0) and (a.max_steps is None or ran < a.max_steps):
        ran += 1
        t0 = time.time()
        net.train_load_go(rec, *darknet.go_draw_moves(len(rec), n.batch))
        loss = net.train_step_loaded() / n.batch
        avg = loss if avg < 0 else avg
        avg = avg * .95 + loss * .05
        i, seen = net.get_current_batch(), net.get_current_batch() * n.batch
        print("%d, %.3f: %f, %f avg, %f rate, %f seconds, %d images" % (i, seen / len(rec), loss, avg, net.get_current_rate(), time.time() - t0, seen),
              file=sys.stderr)
        if seen // len(rec) > epoch:
            epoch = seen // len(rec)
            net.save_weights(os.path.join(a.backup, "%s_%d.weights" % (base, epoch)))
        if i % 100 == 0:
            net.save_weights(os.path.join(a.backup, "%s.backup" % base))
    final = os.path.join(a.backup, "%s.weights" % base)
    net.save_weights(final)
    print(final)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="verb", required=True)
    v = sub.add_parser("valid")
    v.add_argument("cfg"), v.add_argument("weights"), v.add_argument("moves")
    v.add_argument("--multi", action="store_true"), v.add_argument("--chunk", type=int, default=256)
    s = sub.add_parser("self")
    s.add_argument("cfg")
    for name in ("weights", "cfg2", "weights2"):
        s.add_argument(name, nargs="?", default=None)
    s.add_argument("--multi", action="store_true")
    s.add_argument("--games", type=int, default=8), s.add_argument("--rounds", type=int, default=1)
    s.add_argument("--max-moves", type=int, default=300), s.add_argument("--out", default=None)
    s.add_argument("--seed", type=int, default=None), s.add_argument("--poll", type=int, default=0)
    t = sub.add_parser("train")
    t.add_argument("cfg"), t.add_argument("moves"), t.add_argument("--backup", required=True)
    t.add_argument("--weights", default=None), t.add_argument("--seed", type=int, default=None)
    t.add_argument("--max-steps", type=int, default=None)
    a = ap.parse_args()
    {"valid": valid, "self": self_play, "train": train}[a.verb](a)


if __name__ == "__main__":
    main()
