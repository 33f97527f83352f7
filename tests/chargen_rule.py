"""The sampling rule of test_char_rnn (rnn.c:273-276) and sample_array (utils.c:520-531) in numpy fp32, in the reference's
own order.  tests/golden/gen_chargen_golden.py pins it on the reference's compiled sample_array; the tests apply it to
the engine's rows."""
from __future__ import annotations

import math

import numpy as np


def sample_rule(row, u, n):
    """(token, margin): the index the reference draws from the first n values of `row` with the uniform `u`, and how far
    the running subtraction was from deciding otherwise: min(r just before the deciding subtraction, -r after it)"""
    a = np.array(np.asarray(row).reshape(-1)[:n], dtype=np.float32)
    a[a.astype(np.float64) < .0001] = 0                       # rnn.c:274, compared in double
    s = np.float32(0)
    for v in a:                                               # sum_array (utils.c:407): fp32, ascending, from 0
        s = np.float32(s + v)
    with np.errstate(all="ignore"):
        a = (a * np.float32(1. / np.float64(s))).astype(np.float32)   # scale_array(a, n, 1. / sum): the divide in double
        r = np.float32(u)
        for i in range(n):
            before = r
            r = np.float32(r - a[i])
            if r <= 0:
                return i, float(min(before, -r))
    return n - 1, 0.0


def margin_bar(row, n):
    """what a draw's margin must exceed for a row that is only within 1e-4 * max(row) per value of the reference's to
    give the same index: 2 * (K * delta + F * 1e-4), K values left after thresholding, F values within delta of .0001"""
    a = np.asarray(row, dtype=np.float64).reshape(-1)[:n]
    delta = 1e-4 * float(np.asarray(row).max())
    K = int((a >= .0001).sum())
    F = int((np.abs(a - .0001) <= delta).sum())
    return 2 * (K * delta + F * 1e-4)


def perplexity(p_next, text):
    """valid_char_rnn's bookkeeping (rnn.c:402-416) over the whole text: p_next[i] is the probability given to text[i+1].
    Returns (perplexity, word perplexity) as the reference's printf arguments, in double"""
    log2 = np.float32(math.log(2.))
    s = np.float32(0)
    words = 1
    for i, p in enumerate(np.asarray(p_next, np.float32).reshape(-1)):
        if text[i + 1] in (ord(" "), ord("\n"), ord("\t")):
            words += 1
        s = np.float32(float(s) + (math.log(float(p)) if p > 0 else -math.inf) / float(log2))     # libm's log, as the C side
    count = len(p_next)
    return float(2. ** np.float64(np.float32(-s) / np.float32(count))), float(2. ** np.float64(np.float32(-s) / np.float32(words)))
