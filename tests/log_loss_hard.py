"""Hard inputs for the Gaussian log-loss and its gradients (sqfa_amd.classify.gaussian_log_loss, gauss_log_loss_kernel.hip),
their truth in numpy.longdouble by closed form and an a priori float32 error bound per entry.  Plain numpy; independent of the
package and of log_loss_oracle (which only supplies the float64 yardstick).  classify_hard supplies the long double factors
(W, offset), the scores with their bound B (bound32), the evidence bound BE, logsumexp, log_priors and U32.

Inputs (problem): K >= 1, every number rounded through float32 so that both dtypes see the same numbers.
    S0 = s^2 Q diag(logspace(0, -log10 cond, K)) Q^T,  R = chol(S0)             one base shared by the classes
    Sigma_c = R (I + t E_c) R^T,  E_c = (G + G^T) / sqrt(2K)                     spectrum of E_c within about [-2, 2]
    mu_c = s shift + R (delta / sqrt(2K)) N(0, I)                                two classes are delta apart, whitened
    z_n = mu_src(n) + far L_src(n) N(0, I)
The classes are delta apart in the whitened metric whatever cond is: the posteriors stay contested while |W| grows with cond.
LEVELS: level -> (cond, t, delta, far, s, shift).  LAYOUTS: name -> (labels, the class each sample is drawn from).

Truth, with W, offset = classify_hard.factors, y_nc = W_c (z_n - mu_c), S_nc = -1/2 |y_nc|^2 + offset_c, E_n = logsumexp_c S_nc,
p_nc = exp(S_nc - E_n), g the upstream scalar:
    ll_n = -log1p(sum_{c != y_n} exp(S_nc - S_{n,y_n})), the sum formed as a log-sum-exp;  loss = -1/N sum_n ll_n
    P_n = sum_{c != y_n} p_nc;  r_nc = g p_nc / N (c != y_n),  r_{n,y_n} = -g P_n / N
    gZ_n = -sum_c W_c^T (r_nc y_nc),  gmu_c = W_c^T sum_n r_nc y_nc,  gcov_c = 1/2 W_c^T (sum_n r_nc (y_nc y_nc^T - I)) W_c

float32 bound, per entry, first order, no tuned constant.  u = 2^-24, a = |W| |d|, dy = (K + 2) u a (classify_hard: one
rounding of W, one of d = z - mu, K of the inner product), tiny = 2^-126 (a float32 result below it may be flushed to zero).
The kernels recompute the score in the bits of the scores pass, so s_nc carries B_nc and lse_n carries BE_n.
    e_nc = B_nc + BE_n + u |S_nc - E_n|          the two errors and the rounding of the difference s - lse
    dp_nc = p_nc (expm1(e_nc) + 4 u) + tiny      exp of a perturbed argument, exactly; 4 u for the exp routine; underflow.
                                                 A class of zero weight has s = -inf and p = 0 exactly: dp = 0
    dP_n = sum_{c != y} dp_nc + (C - 1) u P_n    a float32 sum of C - 1 non-negative terms in any order, splits included
    dr_nc = |g|/N (dp_nc + 3 u p_nc) + tiny      g rounded to float32, the division by N, the product: 3 roundings.  The
    dr_{n,y} = |g|/N (dP_n + 3 u P_n) + tiny     + tiny is added here to the issue's term: g/N < 1 scales dp's tiny down, but
                                                 the product g/N p itself underflows with an absolute error of up to tiny
    ll_n: B_{n,y_n} + BE_n + u (1 + |ll_n|)      the label pass forms s_y in double from the float32 W and z - mu (inside B),
                                                 subtracts the float32 lse and rounds; the clamp at 0 only moves towards the
                                                 truth, which is <= 0.  loss: the mean of these + u |loss| (double sum, rounded)
    gZ[n,k]: sum_c (|W_c|^T (dr |y| + |r| dy))_k + (C K + splits + 4) u A_Z[n,k] + u |gZ[n,k]| + tiny (sum_c sum_i |W_c|_ik + C K)
             A_Z = sum_c |r_nc| (|W_c|^T |y_nc|)_k.  First term: the errors of r and y through the exact second product.  C K
             float32 accumulations of the MFMA chain over all classes, `splits` additions of the class splits (bounded here by
             min(16, ceil(C / 4)), the number of class groups, whatever the layout), the rounding of W, of the product r y,
             and two of the finish: + 4.  u |gZ|: the final rounding.  The labelled class's term is formed in double from the
             same float32 W and P_n: inside the same terms.  The tiny term is added to the issue's bound: each product r y_i
             and each product of the MFMA chain may underflow with an absolute error of tiny (confident rows are ~1e-33).
    gmu[c,k]: dv_i = sum_n (dr |y_i| + |r| dy_i) + (N + 4) u sum_n |r| |y_i| + N tiny  (float32 sum over the samples in any
             order; products r y_i that underflow: the N tiny is added to the issue's term for the same reason as above);
             bound (|W_c|^T (dv + u |v|))_k + u |gmu|  (the double finish reads the float32 W: u |v| through |W|^T; the final
             rounding).  A_mu = |W|^T sum_n |r| |y|.
    gcov[c]: dM_ij = sum_n (dr |y_i y_j| + |r| (dy_i |y_j| + |y_i| dy_j)) + (N + 4) u sum_n |r| |y_i y_j| + tiny (sum_n |y_i| + N)
             dR = sum_n dr + (N + 4) u sum_n |r|
             bound 1/2 |W|^T (dM + dR I + 2 u |M - R I|) |W| + u |gcov|   (two float32 W in the double finish: 2 u)
             A_cov = 1/2 |W|^T (sum_n |r| |y| |y|^T + sum_n |r| I) |W|
             (tiny term: the products r y_j, each then multiplied by |y_i|, and the N products of the MFMA chain.)

float64 rule, per entry: |err| <= max(1e-10, 5 x yardstick) x (A + C 2^-1022) for the gradients with the entry's own A_Z, A_mu,
A_cov; x (1 + |ll|) for ll and the loss.  The yardstick is the worst error of log_loss_oracle.evaluate in float64 (torch
autograd on the CPU) against the truth, in the same metric, per case and quantity.  Nothing a kernel returned enters a tolerance.

No (C, N, K, K) array is formed: every sum over the samples is a matrix product of (c, K, N) with (c, N, K), a chunk of
classes at a time.
"""
import functools

import numpy as np

import classify_hard as ch

LD = np.longdouble
U32 = ch.U32
TINY = LD(2.0) ** -126
FLOOR64 = LD(2.0) ** -1022
F64_CONSTANT = 1e-10
UPSTREAM = 0.7
N_SAMPLES = 150
N_SPLIT = 300   # sqfa_gauss_log_loss_layout reports 2 sample splits

# level -> (cond, t, delta, far, s, shift)
LEVELS = {
    "contested": (1e2, 0.3, 1.5, 1.0, 1.0, 0.0),
    "contested-c1e3": (1e3, 0.3, 1.5, 1.0, 1.0, 0.0),
    "contested-c1e6": (1e6, 0.3, 1.5, 1.0, 1.0, 0.0),
    "contested-far": (1e2, 0.3, 1.5, 6.0, 1.0, 0.0),
    "contested-farmean": (1e2, 0.3, 1.5, 1.0, 1.0, 1e3),
    "contested-small": (1e2, 0.3, 1.5, 1.0, 1e-4, 0.0),
    "contested-big": (1e2, 0.3, 1.5, 1.0, 1e4, 0.0),
    "confident": (1e3, 0.1, 12.0, 1.0, 1.0, 0.0),
}
OTHER_LEVEL_SIZES = (5, 17, 33, 64)
CONFIDENT_SIZES = tuple(K for K in ch.SIZES if K >= 5)
# layout -> (level, N)
LAYOUTS = {
    "round-robin": ("contested", N_SAMPLES),
    "sorted": ("contested", N_SPLIT),
    "tile-label": ("contested", N_SAMPLES),
    "one-class": ("contested", N_SAMPLES),
    "empty-classes": ("contested", N_SAMPLES),
    "mislabelled": ("confident", N_SAMPLES),
}
LAYOUT_SIZES = (5, 33)
PRIOR_EDGE_LEVEL, PRIOR_EDGE_K = "contested-c1e3", 5
# (level, C, K) -> added to the seed where a non-vacuity condition of tests/test_log_loss_hard.py failed with the plain seed
SEED_BUMP = {}


def seed_of(level, C, K):
    return 1000 * C + K + 100000 * list(LEVELS).index(level) + SEED_BUMP.get((level, C, K), 0)


def layout_labels(layout, N, C, weights=None):
    """(labels (N,), source (N,)): the label of every sample and the class it is drawn from."""
    n = np.arange(N)
    if weights is not None:   # prior edges: round-robin over the classes of non-zero weight
        nz = np.nonzero(np.asarray(weights) != 0)[0]
        labels = nz[n % len(nz)]
        return labels, labels
    if layout == "round-robin":
        return n % C, n % C
    if layout == "sorted":
        labels = np.sort(n % C)
        return labels, labels
    if layout == "tile-label":
        labels = (n // 16) % C
        return labels, labels
    if layout == "one-class":
        return np.full(N, 4), n % C
    if layout == "empty-classes":
        labels = n % 7 + 1
        return labels, labels
    if layout == "mislabelled":
        source = n % C
        return np.where(n % 10 == 0, (source + 1) % C, source), source
    raise KeyError(layout)


def problem(level, C, K, N, layout="round-robin", weights=None, seed=None):
    """(Z (N,K), labels (N,), source (N,), means (C,K), covariances (C,K,K)) float64, every number a float32 number."""
    cond, t, delta, far, s, shift = LEVELS[level]
    rng = np.random.default_rng(seed_of(level, C, K) if seed is None else seed)
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
    S0 = s * s * (Q * np.logspace(0.0, -np.log10(cond), K)) @ Q.T
    R = np.linalg.cholesky(0.5 * (S0 + S0.T))
    G = rng.standard_normal((C, K, K))
    E = (G + G.transpose(0, 2, 1)) / np.sqrt(2.0 * K)
    cov = R @ (np.eye(K) + t * E) @ R.T
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    mu = s * shift + (delta / np.sqrt(2.0 * K)) * rng.standard_normal((C, K)) @ R.T
    labels, source = layout_labels(layout, N, C, weights)
    L = np.linalg.cholesky(cov)
    Z = mu[source] + far * np.einsum("nij,nj->ni", L[source], rng.standard_normal((N, K)))
    cov = ch._round32(cov)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))   # halves of sums of two equal float32 numbers: exact
    return ch._round32(Z), labels, source, ch._round32(mu), cov


def class_split_bound(C):
    """At most one split per group of 4 classes, at most 16."""
    return min(16, (C + 3) // 4)


def evaluate(Z, labels, mu, cov, log_prior=None, upstream=UPSTREAM, chunk=8):
    """Truth, float32 bounds (b_*) and the scales A_* of the float64 rule, all long double.  mu None = zero means."""
    Zl = np.asarray(Z, dtype=np.float64).astype(LD)
    labels = np.asarray(labels)
    N, K = Zl.shape
    C = np.shape(cov)[0]
    if log_prior is None:
        log_prior = ch.log_priors(None, C)
    g = LD(upstream)
    S, _, B = ch._evaluate(Z, mu, cov, log_prior)
    W, _ = ch.factors(cov, log_prior)
    E = ch.logsumexp(S)
    BE = ch.evidence_bound32(B, E)
    rows = np.arange(N)
    own = labels[:, None] == np.arange(C)[None]
    fin = np.isfinite(S)
    assert fin[rows, labels].all(), "a label on a class of zero weight"
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rel = np.where(own, -np.inf, S - S[rows, labels][:, None])
        m = rel.max(1)
        m0 = np.where(np.isfinite(m), m, 0)
        x = m0 + np.log(np.exp(rel - m0[:, None]).sum(1)) if C > 1 else np.full(N, -np.inf, dtype=LD)
        ll = -(np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))))
        p = np.exp(S - E[:, None])
        P = np.where(own, 0, p).sum(1)
        e = np.where(fin, B + BE[:, None] + U32 * np.abs(S - E[:, None]), 0)
        dp = np.where(fin, p * (np.expm1(e) + 4 * U32) + TINY, 0)
    dP = np.where(own, 0, dp).sum(1) + (C - 1) * U32 * P
    r = g / N * np.where(own, -P[:, None], p)
    dr = np.abs(g) / N * np.where(own, (dP + 3 * U32 * P)[:, None], dp + 3 * U32 * p) + np.where(fin, TINY, 0)
    b_ll = B[rows, labels] + BE + U32 * (1 + np.abs(ll))
    loss = -ll.mean()
    b_loss = b_ll.mean() + U32 * np.abs(loss)

    gZ, bZ, AZ = (np.zeros((N, K), dtype=LD) for _ in range(3))
    flushZ = np.zeros(K, dtype=LD)
    gmu, b_mu, A_mu = (np.empty((C, K), dtype=LD) for _ in range(3))
    gcov, b_cov, A_cov = (np.empty((C, K, K), dtype=LD) for _ in range(3))
    eye = np.eye(K, dtype=LD)
    mul = None if mu is None else np.asarray(mu, dtype=np.float64).astype(LD)
    T = lambda a: a.transpose(0, 2, 1)
    for c0 in range(0, C, chunk):
        sl = slice(c0, min(C, c0 + chunk))
        Wc = W[sl]
        aW = np.abs(Wc)
        d = np.broadcast_to(Zl[None], (Wc.shape[0], N, K)) if mul is None else Zl[None] - mul[sl, None]
        y = np.matmul(d, T(Wc))
        ay = np.abs(y)
        dy = (K + 2) * U32 * np.matmul(np.abs(d), T(aW))
        rc, drc = r.T[sl][:, :, None], dr.T[sl][:, :, None]
        arc = np.abs(rc)
        ry, ary, t1 = rc * y, arc * ay, drc * ay + arc * dy
        gZ -= np.matmul(ry, Wc).sum(0)
        bZ += np.matmul(t1, aW).sum(0)
        AZ += np.matmul(ary, aW).sum(0)
        flushZ += aW.sum(1).sum(0)
        v, sary = ry.sum(1), ary.sum(1)
        dv = t1.sum(1) + (N + 4) * U32 * sary + N * TINY
        gmu[sl] = np.matmul(v[:, None, :], Wc)[:, 0]
        b_mu[sl] = np.matmul((dv + U32 * np.abs(v))[:, None, :], aW)[:, 0] + U32 * np.abs(gmu[sl])
        A_mu[sl] = np.matmul(sary[:, None, :], aW)[:, 0]
        M, aM = np.matmul(T(ry), y), np.matmul(T(ary), ay)
        dM = np.matmul(T(drc * ay), ay) + np.matmul(T(arc * dy), ay) + np.matmul(T(ary), dy) + (N + 4) * U32 * aM \
            + TINY * (ay.sum(1)[:, :, None] + N)
        R, aR = rc.sum(1)[:, :, None], arc.sum(1)[:, :, None]
        dR = drc.sum(1)[:, :, None] + (N + 4) * U32 * aR
        H = M - R * eye
        gcov[sl] = LD(0.5) * np.matmul(np.matmul(T(Wc), H), Wc)
        b_cov[sl] = LD(0.5) * np.matmul(np.matmul(T(aW), dM + dR * eye + 2 * U32 * np.abs(H)), aW) + U32 * np.abs(gcov[sl])
        A_cov[sl] = LD(0.5) * np.matmul(np.matmul(T(aW), aM + aR * eye), aW)
    b_Z = bZ + (C * K + class_split_bound(C) + 4) * U32 * AZ + U32 * np.abs(gZ) + TINY * (flushZ[None] + C * K)
    floor = C * FLOOR64
    return dict(S=S, E=E, P=P, ll=ll, loss=loss, gZ=gZ, gmu=gmu, gcov=gcov, b_ll=b_ll, b_loss=b_loss, b_gZ=b_Z, b_gmu=b_mu,
                b_gcov=b_cov, A_ll=1 + np.abs(ll), A_loss=1 + np.abs(loss), A_gZ=AZ + floor, A_gmu=A_mu + floor,
                A_gcov=A_cov + floor)


QUANTITIES = ("ll", "loss", "gZ", "gmu", "gcov")


def yardsticks(ev, oracle):
    """quantity -> worst |oracle - truth| / A of a float64 evaluation `oracle` (dict with the keys of QUANTITIES)."""
    out = {}
    for q in QUANTITIES:
        if oracle.get(q) is None:
            continue
        out[q] = float((np.abs(np.asarray(oracle[q], dtype=np.float64).astype(LD) - ev[q]) / ev["A_" + q]).max())
    return out


def tolerances64(yard):
    return {q: max(F64_CONSTANT, 5 * y) for q, y in yard.items()}


def bounds(ref, dtype):
    """quantity -> per-entry bound: "float32" the a priori one, "float64" tol64 x A."""
    if dtype == "float32":
        return {q: ref["b_" + q] for q in QUANTITIES}
    return {q: ref["tol64"][q] * ref["A_" + q] for q in ref["tol64"]}


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def reference(level, C, K, N=N_SAMPLES, layout="round-robin", weights=None):
    """One case, computed once and read-only: Z, labels, source, mu, cov, log_priors, weights, upstream; the keys of evaluate;
    yard and tol64 (quantity -> float)."""
    import log_loss_oracle
    Z, labels, source, mu, cov = problem(level, C, K, N, layout, weights)
    lp = ch.log_priors(weights, C)
    ev = evaluate(Z, labels, mu, cov, lp, UPSTREAM)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    yard = yardsticks(ev, log_loss_oracle.evaluate(Z, labels, mu, cov, w, UPSTREAM))
    return _frozen(dict(ev, Z=Z, labels=labels, source=source, mu=mu, cov=cov, log_priors=lp, weights=weights,
                        upstream=UPSTREAM, yard=yard, tol64=tolerances64(yard)))


def prior_edge(name):
    C, weights = ch.PRIOR_EDGES[name]
    return reference(PRIOR_EDGE_LEVEL, C, PRIOR_EDGE_K, N_SAMPLES, "round-robin", weights)


def gpu_matrix():
    """The (level, C, K, N, layout) cases of tests/test_gpu_log_loss_hard.py, round-robin first, then the layouts."""
    cases = [("contested", C, K, N_SAMPLES, "round-robin") for C in ch.CLASS_COUNTS for K in ch.SIZES]
    cases += [("confident", 9, K, N_SAMPLES, "round-robin") for K in CONFIDENT_SIZES]
    cases += [(level, 9, K, N_SAMPLES, "round-robin") for level in LEVELS if level not in ("contested", "confident")
              for K in OTHER_LEVEL_SIZES]
    return cases


def layout_cases():
    return [(level, 9, K, N, layout) for layout, (level, N) in LAYOUTS.items() for K in LAYOUT_SIZES]
