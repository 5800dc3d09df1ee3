"""float64 numpy oracle of the Gaussian class scores (sqfa_amd.classify), independent of the package's torch expression:

    score[n, c] = -1/2 |L_c^-1 (z_n - mu_c)|^2 - sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c,   Sigma_c = L_c L_c^T

numpy.linalg.cholesky and scipy.linalg.solve_triangular, one class at a time.  Also the generator of the test problems."""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import logsumexp


def log_priors(priors, n_classes):
    if priors is None:
        return np.full(n_classes, -np.log(n_classes))
    w = np.asarray(priors, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log(w / w.sum())


def scores(Z, means, covariances, priors=None):
    """(N, C) float64 scores; means None = zero means; priors None = uniform, else (C,) weights (normalised here)."""
    Z = np.asarray(Z, dtype=np.float64)
    cov = np.asarray(covariances, dtype=np.float64)
    C, K = cov.shape[0], cov.shape[-1]
    lp = log_priors(priors, C)
    out = np.empty((Z.shape[0], C))
    for c in range(C):
        L = np.linalg.cholesky(cov[c])
        diff = Z if means is None else Z - np.asarray(means, dtype=np.float64)[c]
        y = solve_triangular(L, diff.T, lower=True)
        out[:, c] = -0.5 * (y * y).sum(0) - np.log(np.diag(L)).sum() - 0.5 * K * np.log(2.0 * np.pi) + lp[c]
    return out


def predict(S):
    return np.argmax(S, axis=1)


def log_evidence(S):
    return logsumexp(S, axis=1)


def top_two_gap(S):
    """The gap between the largest and the second largest score of every row (inf for one class)."""
    if S.shape[1] < 2:
        return np.full(S.shape[0], np.inf)
    part = np.partition(S, -2, axis=1)
    return part[:, -1] - part[:, -2]


def problem(C, K, N, sep, seed=0):
    """Sigma_c = A A^T / (K + 3) + 0.05 I with A (K, K + 3) standard normal; mu_c = sep N(0, I); every sample drawn from its
    class's Gaussian (classes in turn): (Z (N,K), labels (N,), means (C,K), covariances (C,K,K)) float64."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((C, K, K + 3))
    cov = A @ A.transpose(0, 2, 1) / (K + 3) + 0.05 * np.eye(K)
    mu = sep * rng.standard_normal((C, K))
    labels = np.arange(N) % C
    L = np.linalg.cholesky(cov)
    Z = mu[labels] + np.einsum("nij,nj->ni", L[labels], rng.standard_normal((N, K)))
    return Z, labels, mu, cov
