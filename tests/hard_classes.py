"""Close, ill-conditioned classes for the class-pair losses, and their float64 truth.  numpy only; nothing of sqfa_amd.

Inputs.  close_classes: a base S0 = Q diag(ev) Q^T with ev log-spaced over `cond`, R = chol(S0), and classes
S_c = R (I + t E_c) R^T, E_c symmetric standard normal / sqrt(m), means mu_c = mu_0 + t R d_c: the classes are t apart in
the whitened metric whatever `cond` is, so every divergence is O(t^2).  Class 0 is the base itself, class n-1 a bitwise copy
of class 1.  LEVELS names the three settings the tests use.  mixed_classes: four far classes of a family's own generator plus
three classes t = 1e-3 around one of them.

Truth.  Everything a three-log-determinant or trace formula would cancel is written as an explicit difference.  For a pair
with Sbar = (S_i + S_j)/2 = L L^T, Delta = (S_i - S_j)/2, M = L^-1 Delta L^-T = V diag(mu_k) V^T:

    S_i = L (I + M) L^T,   S_j = L (I - M) L^T
    logdet Sbar - (logdet S_i + logdet S_j)/2 = -1/2 sum_k log1p(-mu_k^2)                      (Stein; twice Bhattacharyya's term)
    Sbar^-1 - S_i^-1 = Sbar^-1 Delta S_i^-1    = L^-T V diag(mu/(1 + mu)) V^T L^-1               (its gradient, times 1/2)
    -1/2 <P_i - P_j, S_i - S_j> = 1/2 tr(P_i dS P_j dS) = 2 sum_k mu_k^2 / (1 - mu_k^2)          (Jeffreys, dS = S_i - S_j)
    P_j - P_i S_j P_i = P_i dS (P_i + P_j)     = L^-T V diag(4 mu / ((1 - mu)(1 + mu)^2)) V^T L^-1  (its gradient, times 1/2)

The log-Euclidean distance has no such form: its truth is the float64 definition (eigh, log, explicit difference of the
logarithms), whose error grows as eps * cond / t; tests/test_hard_classes.py measures it against mpmath.

Every *_truth returns dict(loss, dist, gmu, gcov) of loss = sum_{i>j} W_ij D_ij: dist the unweighted (n,n) matrix with the
diagonal 0 or sqrt(eps), gcov the gradient wrt the symmetric matrices, gmu None for a means-free family."""
import numpy as np

EPS = 1e-6
LEVELS = {
    "L1": dict(t=1e-2, cond=1e1, round32=True),
    "L2": dict(t=1e-3, cond=1e3, round32=True),
    # not rounded: float32 rounding at cond 1e6 moves a class by 6e-8 * cond in the whitened metric, more than t
    "L3": dict(t=1e-5, cond=1e6, round32=False),
}
MIXED_T = 1e-3


def _sym_normal(rng, m):
    G = rng.standard_normal((m, m))
    return (G + G.T) / np.sqrt(2.0 * m)


def _round32(a):
    return a.astype(np.float32).astype(np.float64)


def _around(R, mu0, t, count, rng):
    """`count` classes t away from the class (mu0, R R^T) in its own whitened metric."""
    m = R.shape[0]
    S = np.stack([R @ (np.eye(m) + t * _sym_normal(rng, m)) @ R.T for _ in range(count)])
    mu = np.stack([mu0 + t * (R @ rng.standard_normal(m)) for _ in range(count)])
    return mu, S


def close_classes(n, m, t, cond, seed, round32):
    """(mu (n,m), S (n,m,m)) float64, S exactly symmetric; round32: every entry is a float32 number."""
    assert n >= 3 and m >= 2
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    ev = cond ** (-np.arange(m) / (m - 1.0))
    S0 = (Q * ev) @ Q.T
    S0 = 0.5 * (S0 + S0.T)
    R = np.linalg.cholesky(S0)
    mu0 = rng.standard_normal(m)
    mu, S = _around(R, mu0, t, n, rng)
    mu[0], S[0] = mu0, S0
    S = 0.5 * (S + S.transpose(0, 2, 1))
    if round32:
        mu, S = _round32(mu), _round32(S)
        S = 0.5 * (S + S.transpose(0, 2, 1))      # exact: the two halves are equal already
    mu[n - 1], S[n - 1] = mu[1], S[1]
    return mu, S


def level_classes(level, n, m, seed):
    return close_classes(n, m, seed=seed, **LEVELS[level])


def mixed_classes(far_mu, far_S, seed, around=1, count=3):
    """The far classes (far_mu (k,m) or None, far_S (k,m,m)) followed by `count` classes MIXED_T around class `around`,
    float32-rounded.  Returns (mu or None, S)."""
    rng = np.random.default_rng(seed)
    far_S = np.asarray(far_S, np.float64)
    m = far_S.shape[-1]
    mu0 = np.zeros(m) if far_mu is None else np.asarray(far_mu, np.float64)[around]
    mu_c, S_c = _around(np.linalg.cholesky(far_S[around]), mu0, MIXED_T, count, rng)
    S = _round32(np.concatenate([far_S, S_c]))
    S = 0.5 * (S + S.transpose(0, 2, 1))
    mu = None if far_mu is None else _round32(np.concatenate([np.asarray(far_mu, np.float64), mu_c]))
    return mu, S


def uniform_weights(n):
    return np.full((n, n), -1.0 / (n * (n - 1) // 2))


def random_weights(n, seed):
    """Symmetric (n,n) weights as a closure passes them, -W / sum_{i>j} W, W in [0.5, 1.5] with one zero pair."""
    rng = np.random.default_rng(seed)
    W = 0.5 + rng.uniform(size=(n, n))
    W = 0.5 * (W + W.T)
    W[2, 0] = W[0, 2] = 0.0
    return -W / np.tril(W, -1).sum()


# ---------------------------------------------------------------------------------------------------------------------
def pair_terms(mu, S):
    """The cancellation-free terms of every ordered pair (the diagonal stays zero): ld (n,n) the log-determinant term,
    jc (n,n) the covariance part of Jeffreys, Q (n,n) = delta^T Sbar^-1 delta, s (n,n,m) = Sbar^-1 delta, and the
    gradients wrt S_i:  Gld (n,n,m,m) of ld, Gjc (n,n,m,m) of jc.  mu None: zero means."""
    S = np.asarray(S, np.float64)
    n, m = S.shape[:2]
    mu = np.zeros((n, m)) if mu is None else np.asarray(mu, np.float64)
    out = {k: np.zeros((n, n)) for k in ("ld", "jc", "Q")}
    out["s"] = np.zeros((n, n, m))
    out["Gld"], out["Gjc"] = np.zeros((n, n, m, m)), np.zeros((n, n, m, m))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            Linv = np.linalg.inv(np.linalg.cholesky(0.5 * (S[i] + S[j])))
            M = Linv @ (0.5 * (S[i] - S[j])) @ Linv.T
            lam, V = np.linalg.eigh(0.5 * (M + M.T))
            B = Linv.T @ V                                     # L^-T V
            out["ld"][i, j] = -0.5 * np.log1p(-lam * lam).sum()
            out["jc"][i, j] = 2.0 * (lam * lam / (1.0 - lam * lam)).sum()
            out["Gld"][i, j] = 0.5 * (B * (lam / (1.0 + lam))) @ B.T
            out["Gjc"][i, j] = (B * (2.0 * lam / ((1.0 - lam) * (1.0 + lam) ** 2))) @ B.T
            z = Linv @ (mu[i] - mu[j])
            out["Q"][i, j] = z @ z
            out["s"][i, j] = Linv.T @ z
    return out


def _assemble(W, D, diagonal, dS, dmu):
    """loss, dist, gradients from D (n,n), dD_ij/dS_i (n,n,m,m) and dD_ij/dmu_i (n,n,m) or None."""
    n = D.shape[0]
    W = np.array(W, np.float64)
    np.fill_diagonal(W, 0.0)
    r, c = np.tril_indices(n, -1)
    dist = D.copy()
    np.fill_diagonal(dist, diagonal)
    gcov = np.einsum("ij,ijkl->ikl", W, dS)
    return {"loss": float((W[r, c] * D[r, c]).sum()), "dist": dist, "gcov": 0.5 * (gcov + gcov.transpose(0, 2, 1)),
            "gmu": None if dmu is None else np.einsum("ij,ijk->ik", W, dmu)}


def _root(V, dS, dmu, sqrt_mode, eps):
    """D = V or sqrt(V + eps) and the chain rule on the gradients of V."""
    if not sqrt_mode:
        return V, 0.0, dS, dmu
    D = np.sqrt(V + eps)
    c = 0.5 / D
    return D, np.sqrt(eps), c[:, :, None, None] * dS, None if dmu is None else c[:, :, None] * dmu


def stein_truth(S, sqrt_mode, W, terms=None, eps=EPS):
    t = pair_terms(None, S) if terms is None else terms
    return _assemble(W, *_root(t["ld"], t["Gld"], None, sqrt_mode, eps))


def jeffreys_truth(mu, S, sqrt_mode, W, terms=None, eps=EPS):
    t = pair_terms(mu, S) if terms is None else terms
    if mu is None:
        return _assemble(W, *_root(t["jc"], t["Gjc"], None, sqrt_mode, eps))
    mu = np.asarray(mu, np.float64)
    P = np.linalg.inv(np.asarray(S, np.float64))
    delta = mu[:, None] - mu[None]                                     # (n,n,m)
    Pid = np.einsum("ikl,ijl->ijk", P, delta)                          # P_i delta
    Pjd = np.einsum("jkl,ijl->ijk", P, delta)
    J = t["jc"] + 0.5 * ((Pid + Pjd) * delta).sum(-1)
    dS = t["Gjc"] - 0.5 * Pid[..., :, None] * Pid[..., None, :]
    return _assemble(W, *_root(J, dS, Pid + Pjd, sqrt_mode, eps))


def gauss_truth(mu, S, kind, W, terms=None, eps=EPS):
    """kind 0 bhattacharyya, 1 hellinger, 2 mahalanobis_sq, 3 mahalanobis."""
    t = pair_terms(mu, S) if terms is None else terms
    ss = t["s"][..., :, None] * t["s"][..., None, :]
    if kind in (2, 3):
        return _assemble(W, *_root(t["Q"], -0.5 * ss, 2.0 * t["s"], kind == 3, eps))
    Bh, dS, dmu = t["Q"] / 8 + 0.5 * t["ld"], -ss / 16 + 0.5 * t["Gld"], t["s"] / 4
    if kind == 0:
        return _assemble(W, Bh, 0.0, dS, dmu)
    D = np.sqrt(-np.expm1(-Bh) + eps)
    c = 0.5 * np.exp(-Bh) / D
    return _assemble(W, D, np.sqrt(eps), c[:, :, None, None] * dS, c[:, :, None] * dmu)


def log_euclidean_truth(S, sqrt_mode, W, eps=EPS):
    """The float64 definition: eigh, log, explicit differences; the gradient through the logarithm by Daleckii-Krein."""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    lam, Q = np.linalg.eigh(S)
    Lg = np.einsum("cka,ca,cla->ckl", Q, np.log(lam), Q)
    diff = Lg[:, None] - Lg[None]
    V = (diff * diff).sum((-2, -1))
    D, diagonal, dL, _ = _root(V, 2.0 * diff, None, sqrt_mode, eps)
    Wz = np.array(W, np.float64)
    np.fill_diagonal(Wz, 0.0)
    GL = np.einsum("ij,ijkl->ikl", Wz, dL)                             # gradient wrt log S_i
    x = (lam[:, :, None] - lam[:, None, :]) / lam[:, None, :]          # (la - lb) / lb
    small = np.abs(x) < 1e-8
    K = np.where(small, 1.0 - 0.5 * x, np.log1p(np.where(small, 1.0, x)) / np.where(small, 1.0, x)) / lam[:, None, :]
    inner = np.einsum("cka,ckl,clb->cab", Q, GL, Q) * K
    gcov = np.einsum("cka,cab,clb->ckl", Q, inner, Q)
    r, c = np.tril_indices(n, -1)
    dist = D.copy()
    np.fill_diagonal(dist, diagonal)
    return {"loss": float((Wz[r, c] * D[r, c]).sum()), "dist": dist, "gcov": 0.5 * (gcov + gcov.transpose(0, 2, 1)),
            "gmu": None}
