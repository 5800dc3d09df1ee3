"""Hard inputs for the Gaussian class scores (sqfa_amd.classify), their truth in numpy.longdouble and an a priori float32
error bound per entry.  Plain numpy; independent of classify_oracle.scores and of the package.

    score[n, c] = -1/2 |W_c (z_n - mu_c)|^2 + offset_c,   W_c = L_c^-1,   Sigma_c = L_c L_c^T,
    offset_c = -sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c

problem(level, C, K, N, seed)      unrelated classes Sigma_c = s^2 Q_c diag(logspace(0, -log10 cond, K)) Q_c^T (Q_c from the QR
                                   of a normal matrix), mu_c = s (shift + 0.3 N(0, I)), z_n = mu_c + far L_c N(0, I) with
                                   c = n % C; everything rounded through float32, so that both dtypes see the same numbers
truth(Z, mu, cov, log_priors)      (scores, log evidence, argmax) in long double: hand-written Cholesky and forward substitution
bound32(Z, mu, cov, log_priors)    the first-order forward error bound B[n, c] of the formula as the kernel documents it: factor
                                   and inverse in double, W and z - mu rounded to float32, float32 product and sum of squares.
                                   With u = 2^-24, y = W d, a = |W| |d|, dy = (K + 2) u a (one rounding of W, one of d, K of the
                                   inner product), tot = sum y^2:
                                       B = 1/2 (2 sum |y| dy + sum dy^2 + (K + 1) u tot) + 2 u (|S| + |offset|)
                                   (the squares and their sum: K + 1 roundings of tot; the halving is exact; rounding the offset
                                   to float32 and the final add: 2 u (|offset| + |S|)).  No tuned constant.
evidence_bound32(B, E)             logsumexp is 1-Lipschitz in the max norm: max_c B[n, c] + (C + 4) u (1 + |E_n|)
decided(S, B)                      samples whose winner leads every other finite class by more than the two bounds together
reference(level, C, K, ...)        all of the above for one case, cached and read-only, with the float64 yardstick: the error of
                                   the numpy float64 oracle classify_oracle.scores against the truth, |err| / (1 + |value|)
"""
import functools

import numpy as np

LD = np.longdouble
U32 = LD(2.0) ** -24
LOG_2PI = np.log(LD(8.0) * np.arctan(LD(1.0)))

# level -> (cond, shift, far, s)
LEVELS = {
    "base": (1e1, 0.0, 1.0, 1.0),
    "c1e3": (1e3, 0.0, 1.0, 1.0),
    "c1e6": (1e6, 0.0, 1.0, 1.0),
    "farmean": (1e2, 1e3, 1.0, 1.0),
    "farsample": (1e2, 0.0, 30.0, 1.0),
    "small": (1e2, 0.0, 1.0, 1e-4),
    "big": (1e2, 0.0, 1.0, 1e4),
}
# the GPU matrix (tests/test_gpu_classify_hard.py): both sides of every 16-row block of K, both staging variants; two full
# 64-sample tiles and a partial wave; C = 9: two groups of 4 and a tail, split 3 ways; C = 3: one group, never split
SIZES = (1, 4, 5, 16, 17, 32, 33, 48, 49, 64)
CLASS_COUNTS = (9, 3)
N_SAMPLES = 150
EXCLUSION_CAP = 0.02
F64_CONSTANT = 1e-10


def _weights(C, keep):
    return tuple(1.0 + c % 5 if keep(c) else 0.0 for c in range(C))


# prior edges, run on level c1e3 at K = 5, N = 150: name -> (C, weights).  C = 37 is 10 class groups on 3 sample tiles, so
# every group is its own split
PRIOR_EDGES = {
    "first-split": (37, _weights(37, lambda c: c >= 4)),             # the first split all -inf
    "middle-split": (37, _weights(37, lambda c: not 8 <= c < 12)),   # a middle split all -inf
    "lane-quarter": (37, _weights(37, lambda c: c % 4 != 1)),        # a whole lane quarter -inf in every group
    "only-last": (37, _weights(37, lambda c: c == 36)),              # every split but the last all -inf
    "unsplit-tiny": (3, (0.0, 1e-300, 1.0)),                         # never split; a log prior of -690.8
}
PRIOR_EDGE_LEVEL, PRIOR_EDGE_K = "c1e3", 5


def prior_edge(name):
    C, weights = PRIOR_EDGES[name]
    return reference(PRIOR_EDGE_LEVEL, C, PRIOR_EDGE_K, N_SAMPLES, weights), weights


def seed_of(level, C, K):
    return 100000 * list(LEVELS).index(level) + 100 * C + K


def _round32(a):
    return a.astype(np.float32).astype(np.float64)


def problem(level, C, K, N, seed):
    """(Z (N,K), labels (N,), means (C,K), covariances (C,K,K)) float64, every number a float32 number, cov symmetric."""
    cond, shift, far, s = LEVELS[level]
    rng = np.random.default_rng(seed)
    lam = np.logspace(0.0, -np.log10(cond), K)
    cov = np.empty((C, K, K))
    for c in range(C):
        Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
        cov[c] = s * s * (Q * lam) @ Q.T
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    mu = s * (shift + 0.3 * rng.standard_normal((C, K)))
    labels = np.arange(N) % C
    L = np.linalg.cholesky(cov)
    Z = mu[labels] + far * np.einsum("nij,nj->ni", L[labels], rng.standard_normal((N, K)))
    cov = _round32(cov)   # elementwise on a symmetric matrix: still symmetric
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    return _round32(Z), labels, _round32(mu), cov


def log_priors(weights, C):
    """(C,) float64, what the package hands its kernels: None = uniform; a zero weight gives -inf."""
    if weights is None:
        return np.full(C, -np.log(C))
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log(w / w.sum())


# ---- long double linear algebra, all classes at once -----------------------------------------------------------------
def cholesky(A):
    """Lower Cholesky factors of (C, K, K) long double matrices, column by column."""
    C, K, _ = A.shape
    L = np.zeros((C, K, K), dtype=LD)
    for j in range(K):
        d = A[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
        if not (d > 0).all():
            raise np.linalg.LinAlgError("not positive definite")
        L[:, j, j] = np.sqrt(d)
        if j + 1 < K:
            L[:, j + 1:, j] = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, None, j, :j]).sum(-1)) / L[:, j, j, None]
    return L


def lower_inverse(L):
    """L^-1 by forward substitution on the identity, row by row."""
    C, K, _ = L.shape
    W = np.zeros((C, K, K), dtype=LD)
    eye = np.eye(K, dtype=LD)
    for i in range(K):
        W[:, i, :] = (eye[i] - (L[:, i, :i, None] * W[:, :i, :]).sum(1)) / L[:, i, i, None]
    return W


def factors(cov, log_prior):
    """(W (C,K,K), offset (C,)) in long double."""
    L = cholesky(np.asarray(cov, dtype=np.float64).astype(LD))
    K = L.shape[-1]
    logdiag = np.log(np.diagonal(L, axis1=1, axis2=2)).sum(-1)
    return lower_inverse(L), -logdiag - LD(0.5) * K * LOG_2PI + np.asarray(log_prior, dtype=np.float64).astype(LD)


def _evaluate(Z, mu, cov, log_prior, chunk=8):
    """(S (N,C), offset (C,), B (N,C)) in long double, a chunk of classes at a time."""
    Z = np.asarray(Z, dtype=np.float64).astype(LD)
    C, K = np.shape(cov)[0], np.shape(cov)[-1]
    if log_prior is None:
        log_prior = log_priors(None, C)
    W, offset = factors(cov, log_prior)
    S = np.empty((Z.shape[0], C), dtype=LD)
    B = np.empty_like(S)
    for c0 in range(0, C, chunk):
        Wc = W[c0:c0 + chunk]
        d = Z[None] if mu is None else Z[None] - np.asarray(mu, dtype=np.float64).astype(LD)[c0:c0 + chunk, None]
        y = np.matmul(d, Wc.transpose(0, 2, 1))                    # (c, N, K)
        a = np.matmul(np.abs(d), np.abs(Wc).transpose(0, 2, 1))
        dy = (K + 2) * U32 * a
        tot = (y * y).sum(-1)
        off = offset[c0:c0 + chunk, None]
        Sc = -LD(0.5) * tot + off
        with np.errstate(invalid="ignore"):
            Bc = LD(0.5) * (2 * (np.abs(y) * dy).sum(-1) + (dy * dy).sum(-1) + (K + 1) * U32 * tot) \
                + 2 * U32 * (np.abs(Sc) + np.abs(off))
        S[:, c0:c0 + chunk], B[:, c0:c0 + chunk] = Sc.T, Bc.T
    return S, offset, B


def logsumexp(S):
    m = S.max(1)
    return m + np.log(np.exp(S - m[:, None]).sum(1))


def truth(Z, mu, cov, log_prior=None):
    """(scores (N,C), log evidence (N,), argmax (N,)); scores and evidence in long double."""
    S, _, _ = _evaluate(Z, mu, cov, log_prior)
    return S, logsumexp(S), S.argmax(1)


def bound32(Z, mu, cov, log_prior=None):
    """(N, C) long double; inf where the score is -inf."""
    return _evaluate(Z, mu, cov, log_prior)[2]


def truth_and_bound32(Z, mu, cov, log_prior=None):
    """(truth scores, bound32) from one evaluation."""
    S, _, B = _evaluate(Z, mu, cov, log_prior)
    return S, B


def evidence_bound32(B, E):
    C = B.shape[1]
    return np.where(np.isfinite(B), B, 0).max(1) + (C + 4) * U32 * (1 + np.abs(E))


def decided(S, B):
    """(N,) bool: S[n, best] - S[n, c] > B[n, best] + B[n, c] for every other finite class c."""
    n = np.arange(S.shape[0])
    best = S.argmax(1)
    with np.errstate(invalid="ignore"):
        ok = (S[n, best][:, None] - S > B[n, best][:, None] + B) | ~np.isfinite(S)
    ok[n, best] = True
    return ok.all(1)


def rel(got, want):
    """|got - want| / (1 + |want|) per entry, over the finite entries of want (0 elsewhere)."""
    fin = np.isfinite(want)
    out = np.zeros(np.shape(want), dtype=LD)
    out[fin] = np.abs(np.asarray(got, dtype=LD)[fin] - want[fin]) / (1 + np.abs(want[fin]))
    return out


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def reference(level, C, K, N=N_SAMPLES, weights=None):
    """One case, computed once and read-only.  weights: None or a tuple of C prior weights.  Keys: Z, labels, mu, cov,
    log_priors (float64); S, E, B, BE (long double: truth, bound32, evidence_bound32); pred; decided32; yard_S, yard_E (the
    float64 oracle's worst |err| / (1 + |value|) against the truth); tol64_S, tol64_E = max(1e-10, 5 x yardstick);
    decided64 (the same rule with the float64 bound tol64_S (1 + |S|))."""
    import classify_oracle
    Z, labels, mu, cov = problem(level, C, K, N, seed_of(level, C, K))
    lp = log_priors(weights, C)
    S, _, B = _evaluate(Z, mu, cov, lp)
    E = logsumexp(S)
    S_or = classify_oracle.scores(Z, mu, cov, None if weights is None else np.asarray(weights, dtype=np.float64))
    yard_S = float(rel(S_or, S).max())
    yard_E = float(rel(classify_oracle.log_evidence(S_or), E).max())
    tol_S, tol_E = max(F64_CONSTANT, 5 * yard_S), max(F64_CONSTANT, 5 * yard_E)
    with np.errstate(invalid="ignore"):
        B64 = tol_S * (1 + np.abs(S))
    return _frozen(Z=Z, labels=labels, mu=mu, cov=cov, log_priors=lp, S=S, E=E, B=B, BE=evidence_bound32(B, E),
                   pred=S.argmax(1), decided32=decided(S, B), decided64=decided(S, B64), yard_S=yard_S, yard_E=yard_E,
                   tol64_S=tol_S, tol64_E=tol_E)
