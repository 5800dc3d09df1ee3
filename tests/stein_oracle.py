"""Numpy oracle of the Stein divergence for the tests.

Float64 route, independent of the three log-determinants: with the generalised eigenvalues lambda_k of (A, B)

    S(A, B) = logdet((A + B)/2) - 1/2 logdet A - 1/2 logdet B = sum_k [log((1 + lambda_k)/2) - 1/2 log lambda_k]

The closure loss  sum_{i>j} w_ij D_ij,  D = S or sqrt(|S| + eps), and its gradient wrt every S_c in closed form:

    dloss/dS_i = sum_{j != i} c_ij 1/2 (Sbar_ij^-1 - S_i^-1),   c_ij = w_ij  |  w_ij sign(S_ij) / (2 sqrt(|S_ij| + eps))

`three_logdets` evaluates the defining formula in a chosen numpy dtype: in float32 it is the yardstick the float32 kernels
are held against (numpy's own LU, no sqfa_amd code).  Inputs of the family the tests use: X X^T / (4m) + 0.05 I times a
per-class scale in [0.5, 2], fixed seeds."""
import numpy as np

EPS = 1e-6


def make_classes(n, m, seed):
    """(n,m,m) float64 SPD matrices, exactly symmetric; every S_ij is O(0.1) or larger."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m, 4 * m))
    S = X @ X.transpose(0, 2, 1) / (4 * m) + 0.05 * np.eye(m)
    S = S * rng.uniform(0.5, 2.0, size=(n, 1, 1))
    return 0.5 * (S + S.transpose(0, 2, 1))


def make_weights(n, seed):
    """Symmetric random (n,n) weights in [0.5, 1.5] with zero entries (when the class count allows)."""
    rng = np.random.default_rng(seed)
    W = 0.5 + rng.uniform(size=(n, n))
    W = 0.5 * (W + W.T)
    if n >= 3:
        W[1, 0] = W[0, 1] = 0.0
        W[n - 1, 1] = W[1, n - 1] = 0.0
    return W


def stein_eigenvalues(A, B):
    """(nA,nB) Stein divergences in float64 through the generalised eigenvalues of every pair."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for j in range(B.shape[0]):
        Linv = np.linalg.inv(np.linalg.cholesky(B[j]))
        lam = np.linalg.eigvalsh(Linv @ A @ Linv.T)          # (nA, m): eigenvalues of B^-1 A
        out[:, j] = (np.log((1.0 + lam) / 2.0) - 0.5 * np.log(lam)).sum(-1)
    return out


def three_logdets(A, B, dtype=np.float64):
    """(nA,nB) Stein divergences by the defining formula, every operation in `dtype`."""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    ldA = np.linalg.slogdet(A)[1].astype(dtype)
    ldB = np.linalg.slogdet(B)[1].astype(dtype)
    mid = dtype(0.5) * (A[:, None] + B[None])
    return (np.linalg.slogdet(mid)[1].astype(dtype) - dtype(0.5) * (ldA[:, None] + ldB[None])).astype(dtype)


def loss_and_gradient(S, sqrt_mode, weight, W=None, dtype=np.float64, div=None, clamp=False):
    """dict(loss, dist, grad) of sum_{i>j} w_ij D_ij for the classes S (n,m,m): dist the full unweighted (n,n) matrix, the
    diagonal 0 or sqrt(eps); grad (n,m,m) in closed form.  float64: the divergences come from the generalised eigenvalues;
    any other dtype: from three_logdets, and every operation of the gradient runs in that dtype.  `div`: these divergences
    where the caller has them already.  clamp: a negative divergence counts as 0, with derivative 0."""
    S = np.asarray(S, dtype)
    n = S.shape[0]
    if div is None:
        div = stein_eigenvalues(S, S) if dtype == np.float64 else three_logdets(S, S, dtype)
    div = np.array(div, dtype)
    div[np.arange(n), np.arange(n)] = 0
    eps = dtype(EPS)
    keep = np.ones_like(div)
    if clamp:
        keep = np.where(div < 0, dtype(0), dtype(1)).astype(dtype)
        div = np.where(div < 0, dtype(0), div).astype(dtype)
    if sqrt_mode:
        D = np.sqrt(np.abs(div) + eps).astype(dtype)
        dD = ((keep if clamp else np.sign(div)) / (dtype(2) * D)).astype(dtype)
    else:
        D, dD = div, keep
    Wm = np.full((n, n), weight, dtype) if W is None else np.asarray(W, dtype)
    r, c = np.tril_indices(n, -1)
    loss = (Wm[r, c] * D[r, c]).sum(dtype=dtype)
    C = (Wm * dD).astype(dtype)
    np.fill_diagonal(C, 0)
    P = np.linalg.inv(S).astype(dtype)
    grad = np.zeros_like(S)
    for i in range(n):
        mid_inv = np.linalg.inv(dtype(0.5) * (S[i][None] + S)).astype(dtype)      # (n, m, m)
        grad[i] = dtype(0.5) * ((C[i][:, None, None] * (mid_inv - P[i][None])).sum(0, dtype=dtype))
    return {"loss": loss, "dist": D, "grad": grad}


def max_rel(got, want):
    """max |got - want| / max |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.abs(want).max()
    return float(np.abs(got - want).max() / (den if den > 0 else 1.0))
