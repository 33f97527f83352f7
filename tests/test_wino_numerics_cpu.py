"""fp32 Winograd F(2x2,3x3) against the direct fp32 convolution, restated in numpy (no GPU): is it as close to the truth, and to
the reference, as the kernel it replaces?

Four ways to compute one 3x3 layer (leaky-activated normal inputs, He-scaled weights, a few filters, every pixel):
  truth      fp64
  reference  the reference's GEMM: one fp32 sum over k = (c, kh, kw) in order, product and sum rounded separately (gemm.c:74-88)
  direct     the matrix-core kernel: one fp32 accumulator per output, K in the kernel's order (32-channel chunk, tap, channel),
             two products entering per step with one rounding (v_mfma_f32_32x32x2_f32)
  winograd   V = B^T d B in fp32, U = G g G^T rounded once from double, sixteen accumulators per 2x2 patch summed over the
             channels the same way, A^T M A in fp32
The bounds: Winograd's distance from the truth at most twice the direct kernel's, its distance from the reference at most
1.25 times the direct kernel's (that distance is the reference's own sequential rounding either way)."""
import numpy as np
import pytest

F = np.float32
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _patches(x, k, stride):
    """x [C, H, W] zero-padded by one -> [C, k, k, nY, nX] windows at the given stride"""
    C, H, W = x.shape
    xp = np.zeros((C, H + 2, W + 2), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    ny, nx = (H + 2 - k) // stride + 1, (W + 2 - k) // stride + 1
    out = np.empty((C, k, k, ny, nx), x.dtype)
    for i in range(k):
        for j in range(k):
            out[:, i, j] = xp[:, i:i + stride * ny:stride, j:j + stride * nx:stride]
    return out


def _chain2(a, b):
    """fp32 accumulator chain over K, two products per step, one rounding per step: a [K, P], b [K, N] -> [P, N]"""
    acc = np.zeros((a.shape[1], b.shape[1]), F)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(0, a.shape[0], 2):
        acc = (acc.astype(np.float64) + a64[k][:, None] * b64[k][None, :] + a64[k + 1][:, None] * b64[k + 1][None, :]).astype(F)
    return acc


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
    # the kernel's K order: 32-channel chunk, tap, channel
    order = np.array([(c0 + c) * 9 + t for c0 in range(0, C, 32) for t in range(9) for c in range(32)])
    direct = _chain2(cols[order], wk[order])
    # Winograd
    d = _patches(x, 4, 2)                                               # [C, 4, 4, th, tw]
    th, tw = d.shape[3], d.shape[4]
    r = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]], axis=1)            # B^T d, fp32
    V = np.stack([r[:, :, 0] - r[:, :, 2], r[:, :, 1] + r[:, :, 2], r[:, :, 2] - r[:, :, 1], r[:, :, 1] - r[:, :, 3]], axis=2)
    assert V.dtype == F
    U = np.einsum("ik,nckl,jl->ncij", G, w.astype(np.float64), G).astype(F)                                      # rounded once
    M = np.empty((4, 4, th * tw, N), F)
    for i in range(4):
        for j in range(4):
            M[i, j] = _chain2(V[:, i, j].reshape(C, th * tw), U[:, :, i, j].T)
    s = np.stack([(M[0] + M[1]) + M[2], (M[1] - M[2]) - M[3]])                                                  # A^T M, fp32
    y = np.stack([(s[:, 0] + s[:, 1]) + s[:, 2], (s[:, 1] - s[:, 2]) - s[:, 3]], axis=1)                        # [2, 2, tiles, N]
    assert y.dtype == F
    wino = y.reshape(2, 2, th, tw, N).transpose(2, 0, 3, 1, 4).reshape(H * W, N)
    # the restatement itself: exact arithmetic gives the truth
    Vd, Ud = np.einsum("ik,cklyx,jl->cijyx", BT, d.astype(np.float64), BT), np.einsum("ik,nckl,jl->ncij", G, w.astype(np.float64), G)
    exact = np.einsum("ai,bj,ijyxn->yaxbn", AT, AT, np.einsum("cijyx,ncij->ijyxn", Vd, Ud)).reshape(H * W, N)
    assert np.abs(exact - truth).max() < 1e-12 * max(1.0, np.abs(truth).max())
    return truth, ref, direct, wino


@pytest.mark.parametrize("C,H,W,N", [(512, 18, 18, 4), (1024, 18, 18, 4), (256, 38, 38, 4), (128, 38, 38, 8)])
def test_winograd_is_as_close_as_the_direct_kernel(C, H, W, N):
    truth, ref, direct, wino = _case(C, H, W, N, 1000 + C + H)
    e = lambda a, b: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    ref_t, dir_t, win_t, dir_r, win_r = e(ref, truth), e(direct, truth), e(wino, truth), e(direct, ref), e(wino, ref)
    print("C %d %dx%d: |max| %.2f  reference-truth %.3g  direct-truth %.3g  winograd-truth %.3g  direct-reference %.3g  winograd-reference %.3g"
          % (C, H, W, np.abs(truth).max(), ref_t, dir_t, win_t, dir_r, win_r))
    assert win_t <= 2.0 * dir_t
    assert win_r <= 1.25 * dir_r
