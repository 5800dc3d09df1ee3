"""float64 numpy restatement of torch's orthogonal parametrization as the models register it (Householder map with a
`base` matrix; reference: src/sqfa/model.py:416-431 -> torch.nn.utils.parametrizations._Orthogonal) in compact WY form,
with its backward.  X (K,D) is the raw parameter, K < D; entries on and above the diagonal are ignored except the
diagonal's sign s_i = int(X[i,i]), which is not differentiated.

    V = strictly-lower(X^T) + [I_K; 0]            (D,K) unit lower trapezoidal
    M = striu(V^T V) + diag(|v_i|^2 / 2)          = T^-1 of  H_1 ... H_K = I - V T V^T,  H_i = I - (2/|v_i|^2) v_i v_i^T
    W = M^-1 V_top^T                              V_top = first K rows of V
    P = [I_K; 0] - V W                            the first K columns of H_1 ... H_K
    F = (base @ (P * s))^T                        (K,D)
"""
import numpy as np


def _parts(X):
    K, D = X.shape
    assert K < D
    V = np.tril(X.T.astype(np.float64), -1)
    V[np.arange(K), np.arange(K)] = 1.0
    G = V.T @ V
    M = np.triu(G, 1) + np.diag(np.diag(G) / 2.0)
    W = np.linalg.solve(M, V[:K].T)
    s = np.trunc(np.diag(X[:, :K])).astype(np.float64)
    return V, M, W, s


def forward(X, base):
    """(K,D) filters with orthonormal rows."""
    K, D = X.shape
    V, _, W, s = _parts(X)
    P = np.eye(D, K) - V @ W
    return (np.asarray(base, dtype=np.float64) @ (P * s[None, :])).T


def backward(X, base, gF):
    """Gradient of sum(F * gF) with respect to X; exactly zero on and above the diagonal."""
    K, D = X.shape
    V, M, W, s = _parts(X)
    gP = (np.asarray(base, dtype=np.float64).T @ np.asarray(gF, dtype=np.float64).T) * s[None, :]
    gW = -V.T @ gP
    Z = np.linalg.solve(M.T, gW)
    gM = -Z @ W.T
    N = np.triu(gM, 1)
    gV = -gP @ W.T + V @ (N + N.T + np.diag(np.diag(gM)))
    gV[:K] += Z.T
    return np.tril(gV, -1).T


SIGNS = ("negative", "mixed")


def make_case(K, D, signs, seed=0):
    """(X, base, R): raw parameter of the form the parametrization produces (a -1 / mixed +-1 diagonal) plus N(0, 0.3^2)
    on EVERY off-diagonal entry -- the upper ones must be ignored --, a random orthogonal base, a random upstream
    gradient."""
    rng = np.random.default_rng(1000 * K + D + seed)
    X = 0.3 * rng.standard_normal((K, D))
    diag = -np.ones(K)
    if signs == "mixed":
        diag[::2] = 1.0
        if K == 1:
            diag[0] = 1.0
    X[np.arange(K), np.arange(K)] = diag
    base, _ = np.linalg.qr(rng.standard_normal((D, D)))
    return X, base, rng.standard_normal((K, D))


def torch_reference(X, base, R, dtype=None, device="cpu"):
    """(F, gX) of torch's own _Orthogonal (Householder map, trivialization on) and its autograd for sum(F * R)."""
    import torch
    from torch.nn.utils.parametrizations import _Orthogonal, _OrthMaps
    dtype = dtype or torch.float64
    Xt = torch.tensor(X, dtype=dtype, device=device, requires_grad=True)
    par = _Orthogonal(Xt, _OrthMaps.householder, use_trivialization=True)
    par.base = torch.tensor(base, dtype=dtype, device=device)
    F = par(Xt)
    (F * torch.tensor(R, dtype=dtype, device=device)).sum().backward()
    return F.detach().cpu().numpy(), Xt.grad.cpu().numpy()
