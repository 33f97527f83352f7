"""The fused stationary Winograd kernel's arithmetic (y2_winos.hip) against the direct fp32 convolution, restated in numpy (no
GPU): tests/test_wino_numerics_cpu.py with the new kernel's association order.

Differences from the three-pass path restated there: an accumulator M[i][j] takes its channels two at a time in the order of
the kernel's MFMAs (channels 8 g + s and 8 g + 4 + s per step), the output transform first forms S = M A row by row in the
wave that owns row i -- S[i][0] = (M[i][0] + M[i][1]) + M[i][2], S[i][1] = (M[i][1] - M[i][2]) - M[i][3] -- and then A^T S across
the four waves: Y[0][b] = (S[0][b] + S[1][b]) + S[2][b], Y[1][b] = (S[1][b] - S[2][b]) - S[3][b].  The bounds are that test's:
distance from the truth at most twice the direct kernel's, distance from the reference at most 1.25 times the direct kernel's."""
import numpy as np
import pytest

from tests.test_wino_numerics_cpu import AT, BT, F, G, _chain2, _patches


def _case(C, H, W, N, seed):
    rng = np.random.RandomState(seed)
    x = rng.normal(0, 1, (C, H, W))
    x = np.where(x > 0, x, 0.1 * x).astype(F)
    w = rng.normal(0, np.sqrt(2.0 / (9 * C)), (N, C, 3, 3)).astype(F)
    cols = _patches(x, 3, 1).reshape(C * 9, H * W)                      # k = (c, kh, kw): the reference's im2col order
    wk = w.reshape(N, C * 9).T                                          # [K, N]
    truth = cols.astype(np.float64).T @ wk.astype(np.float64)
    ref = np.zeros((H * W, N), F)
    for k in range(C * 9):
        ref = ref + cols[k][:, None] * wk[k][None, :]                   # fp32 product, fp32 sum
    order = np.array([(c0 + c) * 9 + t for c0 in range(0, C, 32) for t in range(9) for c in range(32)])
    direct = _chain2(cols[order], wk[order])
    # stationary Winograd
    d = _patches(x, 4, 2)                                               # [C, 4, 4, th, tw]
    th, tw = d.shape[3], d.shape[4]
    r = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]], axis=1)            # B^T d, fp32
    V = np.stack([r[:, :, 0] - r[:, :, 2], r[:, :, 1] + r[:, :, 2], r[:, :, 2] - r[:, :, 1], r[:, :, 1] - r[:, :, 3]], axis=2)
    assert V.dtype == F
    U = np.einsum("ik,nckl,jl->ncij", G, w.astype(np.float64), G).astype(F)                                      # rounded once
    korder = np.array([8 * g + 4 * h + s for g in range(C // 8) for s in range(4) for h in range(2)])            # MFMA k pairs
    M = np.empty((4, 4, th * tw, N), F)
    for i in range(4):
        for j in range(4):
            M[i, j] = _chain2(V[:, i, j].reshape(C, th * tw)[korder], U[:, :, i, j].T[korder])
    S = np.stack([(M[:, 0] + M[:, 1]) + M[:, 2], (M[:, 1] - M[:, 2]) - M[:, 3]], axis=1)                          # [i, b]: M A
    y = np.stack([(S[0] + S[1]) + S[2], (S[1] - S[2]) - S[3]])                                                  # [a, b]: A^T S
    assert y.dtype == F and y.shape == (2, 2, th * tw, N)
    winos = y.reshape(2, 2, th, tw, N).transpose(2, 0, 3, 1, 4).reshape(H * W, N)
    # the restatement itself: exact arithmetic gives the truth
    Vd, Ud = np.einsum("ik,cklyx,jl->cijyx", BT, d.astype(np.float64), BT), np.einsum("ik,nckl,jl->ncij", G, w.astype(np.float64), G)
    exact = np.einsum("ai,bj,ijyxn->yaxbn", AT, AT, np.einsum("cijyx,ncij->ijyxn", Vd, Ud)).reshape(H * W, N)
    assert np.abs(exact - truth).max() < 1e-12 * max(1.0, np.abs(truth).max())
    return truth, ref, direct, winos


@pytest.mark.parametrize("C,H,W,N", [(32, 32, 32, 8), (32, 48, 48, 8), (64, 24, 24, 8), (64, 40, 40, 8)])
def test_stationary_winograd_is_as_close_as_the_direct_kernel(C, H, W, N):
    truth, ref, direct, winos = _case(C, H, W, N, 1000 + C + H)
    e = lambda a, b: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    ref_t, dir_t, win_t, dir_r, win_r = e(ref, truth), e(direct, truth), e(winos, truth), e(direct, ref), e(winos, ref)
    print("C %d %dx%d: |max| %.2f  reference-truth %.3g  direct-truth %.3g  winos-truth %.3g  direct-reference %.3g  winos-reference %.3g"
          % (C, H, W, np.abs(truth).max(), ref_t, dir_t, win_t, dir_r, win_r))
    assert win_t <= 2.0 * dir_t
    assert win_r <= 1.25 * dir_r
