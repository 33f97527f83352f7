"""The Go path in numpy, stated from the reference's go.c: the eight views and their merge (predict_move, go.c:262-289),
liberties (calculate_liberties :188), move_go :304, legal_go :338, suicide_go :326, generate_move's decision from :362 on
and random_go_moves' pixel chain (:92-115).  tests/test_go_host.py holds every function here to the fixtures recorded from
the compiled reference (tests/golden/go.npz), so the GPU tests may use it for inputs the fixtures do not carry.

rotate_image_cw (image.c:1035-1054), read from its assignments: one turn is new[r][c] = old[c][18-r], which is
numpy.rot90(a, 1); flip_image (image.c:1056-1070) mirrors columns."""
import numpy as np

N, P, KO, REC = 19, 361, 91, 93
F = np.float32


def rotate_cw(a, times):
    return np.rot90(a.reshape(N, N), (times + 400) % 4)


def flip(a):
    return np.fliplr(a.reshape(N, N))


def view(board, i):
    """view i of predict_move's loop: rotate by i, then flip when i >= 4"""
    a = rotate_cw(board, i)
    return (flip(a) if i >= 4 else a).reshape(P)


def unview(row, i):
    """an output row back: un-flip when i >= 4, then rotate by -i"""
    a = row.reshape(N, N)
    if i >= 4:
        a = flip(a)
    return rotate_cw(a, -i).reshape(P)


def views(boards, players, multi):
    """[n][361], [n] -> the network input, [n * (8 if multi else 1)][361]"""
    out = []
    for b, p in zip(np.asarray(boards, F).reshape(-1, P), players):
        b = -b if p < 0 else b
        out += [view(b, i) for i in range(8 if multi else 1)]
    return np.ascontiguousarray(np.stack(out), dtype=F)


def merge(rows, boards, multi):
    """the softmax rows of views() -> move [n][361]: row 0, += rows 1..7 in order in fp32, x 1/8, occupied points zeroed"""
    boards = np.asarray(boards, F).reshape(-1, P)
    V = 8 if multi else 1
    rows = np.asarray(rows, F).reshape(boards.shape[0], V, P)
    out = np.zeros((boards.shape[0], P), F)
    for n in range(boards.shape[0]):
        acc = rows[n, 0].copy()
        if multi:
            for i in range(1, 8):
                acc = (acc + unview(rows[n, i], i)).astype(F)
            acc = (acc * F(0.125)).astype(F)
        acc[boards[n] != 0] = 0
        out[n] = acc
    return out


def neighbours(p):
    r, c = divmod(p, N)
    return [q for q, ok in ((p + N, r < N - 1), (p - N, r > 0), (p + 1, c < N - 1), (p - 1, c > 0)) if ok]


def group(board, start):
    side, seen, todo = board[start], {start}, [start]
    while todo:
        for q in neighbours(todo.pop()):
            if q not in seen and board[q] == side:
                seen.add(q)
                todo.append(q)
    return seen


def liberties(board):
    """every stone carries its group's count; an empty point adds one to each distinct adjacent group"""
    board = np.asarray(board, F).reshape(P)
    lib, done = np.zeros(P, np.int32), set()
    for p in range(P):
        if board[p] == 0 or p in done:
            continue
        g = group(board, p)
        empty = {q for s in g for q in neighbours(s) if board[q] == 0}
        for s in g:
            lib[s] = len(empty)
        done |= g
    return lib


def move(board, player, r, c):
    """move_go: the counts are those of the board before the stone is placed"""
    b = np.array(board, F).reshape(P)
    lib = liberties(b)
    at = r * N + c
    b[at] = player
    for q in neighbours(at):
        if b[q] == -player and lib[q] == 1:
            for s in group(b, q):
                b[s] = 0
    return b


def pack(board):
    board = np.asarray(board, F).reshape(P)
    s = bytearray(KO)
    for p in range(P):
        if board[p] == 1:
            s[p >> 2] |= 1 << (2 * (p & 3))
        if board[p] == -1:
            s[p >> 2] |= 2 << (2 * (p & 3))
    return bytes(s)


def unpack(s):
    s = bytes(s)
    b = np.zeros(P, F)
    for p in range(P):
        two = (s[p >> 2] >> (2 * (p & 3))) & 3
        b[p] = 1 if two & 1 else -1 if two & 2 else 0
    return b


def legal_map(board, ko, player):
    """legal_go at every point: occupied is illegal, a result equal to ko is illegal, suicide is NOT"""
    board = np.asarray(board, F).reshape(P)
    ko = bytes(ko)
    out = np.zeros(P, np.uint8)
    for p in range(P):
        if board[p] == 0:
            out[p] = pack(move(board, player, p // N, p % N)) != ko
    return out


def suicide_map(board, player):
    board = np.asarray(board, F).reshape(P)
    lib = liberties(board)
    out = np.zeros(P, np.uint8)
    for p in range(P):
        safe = False
        for q in neighbours(p):
            if board[q] == -player:
                safe |= lib[q] <= 1
            elif board[q] == 0:
                safe = True
            else:
                safe |= lib[q] > 1
        out[p] = not safe
    return out


def top_k(a, k):
    """utils.c:179-193: strict >, a displaced entry moves on down the list"""
    index = [-1] * k
    for i in range(len(a)):
        curr = i
        for j in range(k):
            if index[j] < 0 or a[curr] > a[index[j]]:
                curr, index[j] = index[j], curr
    return index


def pick(move_row, legal, suicide, thresh, u):
    """generate_move from go.c:362 on -> (index, the thresholded array before sample_array scales it)"""
    a = np.array(move_row, F).reshape(P)
    a[np.asarray(legal).reshape(P) == 0] = 0
    idx = top_k(a, 5)
    thresh = F(thresh)
    if thresh > a[idx[0]]:
        thresh = a[idx[4]]
    a[a < thresh] = 0
    kept = a.copy()
    mx = 0
    for i in range(1, P):                       # max_index: the first maximum
        if a[i] > a[mx]:
            mx = i
    with np.errstate(all="ignore"):
        s = F(0)
        for v in a:                             # sum_array: ascending from 0 in fp32
            s = F(s + v)
        scale = F(1. / float(s)) if s != 0 else F(np.inf)
        r, c = F(u), P - 1
        for i in range(P):
            r = F(r - F(a[i] * scale))
            if r <= 0:
                c = i
                break
    suicide = np.asarray(suicide).reshape(P)
    return (-1 if suicide[mx] else mx if suicide[c] else c), kept


def loader(records, pick_, flip_, rot):
    """random_go_moves' pixel chain per item: decode, label, clear the move's point, flip if drawn, then rotate"""
    records = np.asarray(records, np.uint8).reshape(-1, REC)
    x, y = np.zeros((len(pick_), P), F), np.zeros((len(pick_), P), F)
    for i, (k, f, t) in enumerate(zip(pick_, flip_, rot)):
        rec = records[k]
        at = int(rec[0]) * N + int(rec[1])
        b = unpack(rec[2:])
        lab = np.zeros(P, F)
        lab[at] = 1
        b[at] = 0
        b, lab = b.reshape(N, N), lab.reshape(N, N)
        if f:
            b, lab = flip(b), flip(lab)
        x[i], y[i] = rotate_cw(b, t).reshape(P), rotate_cw(lab, t).reshape(P)
    return x, y
