"""float64 numpy oracle of the Bures-Wasserstein distance (sqfa_amd.transport, sqfa_bw_pairwise).

    bw2(A, B) = tr A + tr B - 2 sum_k sqrt(lambda_k(A B))
values through eigh of A^1/2 B A^1/2; gradients through the optimal-transport map T from N(0, A) to N(0, B):
    d bw2 / dA = I - T,    T = A^-1/2 (A^1/2 B A^1/2)^1/2 A^-1/2
    d bw2 / dB = I - T^-1
(pinned against central differences in test_transport_cabi.py)."""
import numpy as np

EPSILON = 1e-6


def _sqrtm(S):
    w, V = np.linalg.eigh(S)
    return (V * np.sqrt(w)) @ V.T


def _invsqrtm(S):
    w, V = np.linalg.eigh(S)
    return (V / np.sqrt(w)) @ V.T


def bw2(A, B):
    """bw2 of one pair (m x m SPD)."""
    As = _sqrtm(A)
    lam = np.linalg.eigvalsh(As @ B @ As)
    return float(np.trace(A) + np.trace(B) - 2.0 * np.sum(np.sqrt(np.clip(lam, 0.0, None))))


def transport_map(A, B):
    """T with T A T = B (the OT map from N(0, A) to N(0, B))."""
    As, Ais = _sqrtm(A), _invsqrtm(A)
    return Ais @ _sqrtm(As @ B @ As) @ Ais


def bw2_grads(A, B):
    """(d bw2/dA, d bw2/dB) of one pair."""
    T = transport_map(A, B)
    I = np.eye(A.shape[0])
    return I - T, I - np.linalg.inv(T)


def pairwise(A, B=None, sqrt_mode=True, weights=None):
    """D (nA, nB) and, with `weights` (nA, nB), the gradients of sum_ij w_ij D_ij with respect to A and B.
    B None: self mode -- D over all ordered pairs of A, the gradient with respect to the shared batch."""
    self_mode = B is None
    Bs = A if self_mode else B
    nA, nB = A.shape[0], Bs.shape[0]
    D = np.zeros((nA, nB))
    gA = np.zeros_like(A)
    gB = np.zeros_like(Bs)
    for i in range(nA):
        for j in range(nB):
            d2 = bw2(A[i], Bs[j])
            D[i, j] = np.sqrt(abs(d2) + EPSILON) if sqrt_mode else d2
            if weights is not None and weights[i, j] != 0.0:
                h = weights[i, j] * (np.sign(d2) * 0.5 / D[i, j] if sqrt_mode else 1.0)
                if h != 0.0:
                    ga, gb = bw2_grads(A[i], Bs[j])
                    gA[i] += h * ga
                    gB[j] += h * gb
    if self_mode:
        return D, gA + gB, None
    return D, gA, gB


def closure_loss_and_grad(S, sqrt_mode=True):
    """-mean over i > j of D(S_i, S_j) and its gradient (the fused closure's loss)."""
    C = S.shape[0]
    P = C * (C - 1) // 2
    W = np.tril(np.full((C, C), -1.0 / P), -1)
    D, g, _ = pairwise(S, None, sqrt_mode, W)
    return float(np.sum(W * D)), g, D
