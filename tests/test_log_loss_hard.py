"""CPU tests of tests/log_loss_hard.py, so that tests/test_gpu_log_loss_hard.py cannot pass for the wrong reason: the inputs are
what they claim (contested or confident posteriors, the label layouts), the long double truth agrees with a 50-digit mpmath
evaluation (ll from the defining formula, the gradients by mpmath.diff of the 50-digit loss) to a tenth of the smaller bound
asserted with the entry, a float32 model of the kernels' documented arithmetic (numpy on the CPU, not the kernel) stays inside
every bound over the whole GPU matrix, and leaves it under four mutations: (a) the labelled residual taken as g (p - 1) / N,
(b) the labelled class not left out of u, (c) the last contraction row block of the second product dropped, (d) - R I left
out of grad_cov; and (e) a division by N rounded up to 64."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import classify_hard as ch
import log_loss_hard as lh
import log_loss_oracle

LD = np.longdouble
GRADS = ("gZ", "gmu", "gcov")


def _all_cases():
    """Every reference of the GPU matrix: (label, ref)."""
    for level, C, K, N, layout in lh.gpu_matrix() + lh.layout_cases():
        yield f"{level} C={C} K={K} N={N} {layout}", lh.reference(level, C, K, N, layout)
    for edge in ch.PRIOR_EDGES:
        yield f"priors {edge}", lh.prior_edge(edge)


# ---- the inputs -------------------------------------------------------------------------------------------------------------
def test_inputs_are_float32_numbers_and_symmetric():
    for level in lh.LEVELS:
        ref = lh.reference(level, 9, 17)
        for a in (ref["Z"], ref["mu"], ref["cov"]):
            assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
        assert np.array_equal(ref["cov"], ref["cov"].transpose(0, 2, 1))
        cond, s = lh.LEVELS[level][0], lh.LEVELS[level][4]
        lam = np.linalg.eigvalsh(ref["cov"] / (s * s))
        assert lam.min() > 0 and (lam[:, -1] / lam[:, 0] >= cond / 4).all() and (lam[:, -1] / lam[:, 0] <= 8 * cond).all()


def _share(ref, lo, hi):
    P = ref["P"]
    return float(((P > lo) & (P < hi)).mean())


def test_contested_levels_are_contested():
    """At least 80 % of the samples have 1e-3 < P_n < 1 - 1e-3 (P_n: the other classes' posteriors, from the truth)."""
    for level in ("contested", "contested-c1e6", "contested-c1e3", "contested-farmean", "contested-small", "contested-big"):
        sizes = ch.SIZES if level in ("contested", "contested-c1e6") else lh.OTHER_LEVEL_SIZES
        shares = {(C, K): _share(lh.reference(level, C, K), 1e-3, 1 - 1e-3) for C in ch.CLASS_COUNTS for K in sizes}
        print(f"log-loss-hard {level}: contested share {min(shares.values()):.2f} to {max(shares.values()):.2f}")
        assert min(shares.values()) >= 0.8, (level, shares)


def test_far_samples_mix_contested_and_confident_rows():
    """contested-far draws the samples 6 sigma out: rows of every kind, from contested to P_n < 1e-6, inside one tensor."""
    for K in lh.OTHER_LEVEL_SIZES:
        ref = lh.reference("contested-far", 9, K)
        a, b = _share(ref, 1e-3, 1 - 1e-3), _share(ref, 0, 1e-6)
        print(f"log-loss-hard contested-far K={K}: contested share {a:.2f}, P_n < 1e-6 share {b:.2f}")
        assert a >= 0.05 and b >= 0.05


def test_confident_level_is_confident():
    """C = 9, K >= 5: at least 70 % of the samples have 1e-30 < P_n < 1e-6."""
    shares = {K: _share(lh.reference("confident", 9, K), 1e-30, 1e-6) for K in lh.CONFIDENT_SIZES}
    print(f"log-loss-hard confident: share {min(shares.values()):.2f} to {max(shares.values()):.2f}")
    assert min(shares.values()) >= 0.7, shares


def test_prior_edges_keep_contested_samples():
    """The prior edges with more than one class of non-zero weight keep contested samples; only-last has P_n = 0 exactly."""
    for edge, (C, weights) in ch.PRIOR_EDGES.items():
        ref = lh.prior_edge(edge)
        zero = np.asarray(weights) == 0
        assert not zero[ref["labels"]].any() and set(ref["labels"]) == set(np.nonzero(~zero)[0])
        assert np.array_equal(np.isneginf(ref["S"]), np.broadcast_to(zero, ref["S"].shape))
        share = _share(ref, 1e-3, 1 - 1e-3)
        print(f"log-loss-hard priors {edge}: contested share {share:.2f}")
        if edge == "only-last":
            assert (ref["P"] == 0).all() and (ref["ll"] == 0).all() and not ref["gZ"].any()
        elif edge == "unsplit-tiny":
            # half of the labels on the class of weight 1e-300: ll ~ -690 there, P_n = 1 - tiny
            on_tiny = ref["labels"] == 1
            assert on_tiny.sum() == lh.N_SAMPLES // 2 and (ref["ll"][on_tiny] < -600).all() and (ref["P"][on_tiny] > 0.999).all()
        else:
            assert share >= 0.8, (edge, share)
        assert (ref["gmu"][zero] == 0).all() and (ref["gcov"][zero] == 0).all()


def test_layout_properties():
    C, N = 9, lh.N_SAMPLES
    counts = lambda labels: np.bincount(labels, minlength=C)
    lab, src = lh.layout_labels("round-robin", N, C)
    assert np.array_equal(lab, np.arange(N) % C) and np.array_equal(src, lab)
    lab, src = lh.layout_labels("sorted", lh.N_SPLIT, C)
    assert (np.diff(lab) >= 0).all() and np.array_equal(src, lab) and (counts(lab) > 0).all()
    # the second sample split (16 tiles of 16 samples on) holds no labelled sample of the low classes
    assert lab[256:].min() >= 7 and set(lab[:256]) == set(range(8))
    lab, src = lh.layout_labels("tile-label", N, C)
    assert np.array_equal(src, lab) and all(len(set(lab[t:t + 16])) == 1 for t in range(0, N, 16))
    assert (counts(lab) > 0).all()
    lab, src = lh.layout_labels("one-class", N, C)
    assert (lab == 4).all() and np.array_equal(src, np.arange(N) % C)
    lab, src = lh.layout_labels("empty-classes", N, C)
    assert np.array_equal(src, lab) and np.array_equal(np.nonzero(counts(lab) == 0)[0], [0, 8])
    lab, src = lh.layout_labels("mislabelled", N, C)
    assert np.array_equal(np.nonzero(lab != src)[0], np.arange(0, N, 10)) and np.array_equal(lab[::10], (src[::10] + 1) % C)
    # mislabelled samples on the confident level: ll far below, P_n = 1 - tiny
    for K in lh.LAYOUT_SIZES:
        ref = lh.reference("confident", C, K, N, "mislabelled")
        wrong = ref["labels"] != ref["source"]
        print(f"log-loss-hard mislabelled K={K}: ll down to {float(ref['ll'].min()):.3g}, "
              f"median of the mislabelled {float(np.median(ref['ll'][wrong])):.3g}")
        assert np.median(ref["ll"][wrong]) < -15 and np.median(1 - ref["P"][wrong]) < 1e-6
    # the samples of a layout are drawn from `source`: whitened distance to the source class about sqrt(K)
    ref = lh.reference("contested", C, 33, N, "one-class")
    W, _ = ch.factors(ref["cov"], ref["log_priors"])
    d = (ref["Z"] - ref["mu"][ref["source"]]).astype(LD)
    rr = np.sqrt((np.einsum("nij,nj->ni", W[ref["source"]], d) ** 2).sum(1) / 33).astype(float)
    assert 0.6 <= np.median(rr) <= 1.4


# ---- the truth against mpmath ------------------------------------------------------------------------------------------------
def _mp_of(x):
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


@pytest.mark.parametrize("K", [4, 8, 17])
@pytest.mark.parametrize("level", list(lh.LEVELS))
def test_truth_against_mpmath(level, K):
    """ll_n from the defining formula s_y - logsumexp s with s = -1/2 d^T Sigma^-1 d - 1/2 log det Sigma - K/2 log 2 pi + log
    pi, and a dozen coordinates each of Z, mu and Sigma (symmetric perturbations) by mpmath.diff of g x the 50-digit loss."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    C, N = 3, 12
    ref = lh.reference(level, C, K, N)
    g, y = mpmath.mpf(lh.UPSTREAM), ref["labels"]
    Z = [mpmath.matrix(ref["Z"][n].tolist()) for n in range(N)]
    mu = [mpmath.matrix(ref["mu"][c].tolist()) for c in range(C)]
    cov = [mpmath.matrix(ref["cov"][c].tolist()) for c in range(C)]
    lp = [mpmath.mpf(float(v)) for v in ref["log_priors"]]

    def inv_logdet(A):
        return mpmath.inverse(A), mpmath.log(mpmath.det(A))

    def score(z, m, P, ld, c):
        d = z - m
        return -(d.T * P * d)[0, 0] / 2 - ld / 2 - K * mpmath.log(2 * mpmath.pi) / 2 + lp[c]

    def lls(S):
        out = []
        for n in range(N):
            top = max(S[n])
            out.append(S[n][y[n]] - top - mpmath.log(sum(mpmath.exp(v - top) for v in S[n])))
        return out

    fac = [inv_logdet(A) for A in cov]
    S = [[score(Z[n], mu[c], fac[c][0], fac[c][1], c) for c in range(C)] for n in range(N)]
    b32, b64 = lh.bounds(ref, "float32"), lh.bounds(ref, "float64")
    worst = 0.0

    def compare(got, want, q, at, factor=1):
        nonlocal worst
        bound = factor * min(float(b32[q][at]), float(b64[q][at]))
        err = float(abs(factor * _mp_of(got) - want))
        worst = max(worst, err / bound)
        assert err <= 0.1 * bound, (level, K, q, at, err, bound)

    for n, v in enumerate(lls(S)):
        compare(ref["ll"][n], v, "ll", n)
    compare(ref["loss"], -sum(lls(S)) / N, "loss", ())
    objective = lambda S2: -g * sum(lls(S2)) / N
    rng = np.random.default_rng(K)
    for _ in range(12):
        n, k = int(rng.integers(N)), int(rng.integers(K))

        def f(x):
            z = Z[n].copy()
            z[k] = x
            S2 = list(S)
            S2[n] = [score(z, mu[c], fac[c][0], fac[c][1], c) for c in range(C)]
            return objective(S2)
        compare(ref["gZ"][n, k], mpmath.diff(f, Z[n][k]), "gZ", (n, k))
    for _ in range(12):
        c, k = int(rng.integers(C)), int(rng.integers(K))

        def f(x):
            m = mu[c].copy()
            m[k] = x
            S2 = [list(row) for row in S]
            for n in range(N):
                S2[n][c] = score(Z[n], m, fac[c][0], fac[c][1], c)
            return objective(S2)
        compare(ref["gmu"][c, k], mpmath.diff(f, mu[c][k]), "gmu", (c, k))
    for t in range(12):
        c, i = int(rng.integers(C)), int(rng.integers(K))
        j = i if t % 3 == 0 else int(rng.integers(K))

        def f(x):
            A = cov[c].copy()
            A[i, j] = A[j, i] = x
            P, ld = inv_logdet(A)
            S2 = [list(row) for row in S]
            for n in range(N):
                S2[n][c] = score(Z[n], mu[c], P, ld, c)
            return objective(S2)
        # the derivative along E_ij + E_ji is G_ij + G_ji = 2 G_ij off the diagonal
        compare(ref["gcov"][c, i, j], mpmath.diff(f, cov[c][i, j]), "gcov", (c, i, j), 1 if i == j else 2)
    print(f"log-loss-hard truth against mpmath {level} K={K}: worst error / smaller bound {worst:.2e} (allowed 0.1)")


# ---- the float64 yardsticks --------------------------------------------------------------------------------------------------
def test_float64_yardsticks():
    """log_loss_oracle.evaluate in float64 (torch autograd) against the truth: what the GPU test's float64 bound is made of."""
    worst = {}
    for label, ref in _all_cases():
        key = "priors" if label.startswith("priors") else label.split()[0]
        for q, v in ref["yard"].items():
            worst[key, q] = max(worst.get((key, q), 0.0), v)
    for key in dict.fromkeys(k for k, _ in worst):
        print(f"log-loss-hard float64 oracle {key}: " + " ".join(f"{q} {worst[key, q]:.1e}" for q in lh.QUANTITIES))
    assert max(worst.values()) < 1e-8   # a float64 evaluation, not a float32 one


# ---- a float32 model of the documented arithmetic ----------------------------------------------------------------------------
def model32(ref, mutation=None):
    """The kernels' documented arithmetic on the CPU.  W rounded from a double factor; z - mu, y, the squares, s and lse in
    float32; p = exp(s - lse), P the float32 sum of the others; r = (g / N) p in float32, the labelled class's -(g / N) P;
    float32 sums for u, v, M, R; the labelled term of gZ and the finish in double; ll in double from the float32 W and z - mu.
    Mutations: "p_minus_1" (a), "label_in_u" (b), "drop_row_block" (c), "no_trace" (d), "n_padded" (e)."""
    f = np.float32
    Z, mu, cov, lp, y = ref["Z"], ref["mu"], ref["cov"], ref["log_priors"], ref["labels"]
    N, K = Z.shape
    C = cov.shape[0]
    W = np.empty((C, K, K), dtype=f)
    off = np.empty(C)
    for c in range(C):
        L = np.linalg.cholesky(cov[c])
        W[c] = np.tril(solve_triangular(L, np.eye(K), lower=True)).astype(f)
        off[c] = -np.log(np.diag(L)).sum() - 0.5 * K * np.log(2.0 * np.pi) + lp[c]
    d = Z.astype(f)[None] - mu.astype(f)[:, None]                      # (C, N, K)
    Y = np.matmul(d, W.transpose(0, 2, 1))
    assert Y.dtype == f
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = (f(-0.5) * (Y * Y).sum(-1, dtype=f) + off.astype(f)[:, None]).T   # (N, C)
        m = s.max(1)
        lse = m + np.log(np.exp(s - m[:, None]).sum(1, dtype=f))
        p = np.exp(s - lse[:, None])
    assert lse.dtype == f and p.dtype == f
    own = y[:, None] == np.arange(C)[None]
    rows = np.arange(N)
    P = np.where(own, f(0), p).sum(1, dtype=f)
    n_div = 64 * ((N + 63) // 64) if mutation == "n_padded" else N
    gs = f(lh.UPSTREAM) / f(n_div)
    label_factor = p[rows, y] - f(1) if mutation == "p_minus_1" else -P      # r of the labelled class is gs x this
    r = gs * np.where(own, label_factor[:, None], p)
    assert r.dtype == f
    # ll and the loss: the label pass
    dl = d[y, rows].astype(np.float64)
    yl = np.einsum("nij,nj->ni", W[y].astype(np.float64), dl)
    ll = np.minimum(-0.5 * (yl * yl).sum(1) + off[y] - lse.astype(np.float64), 0.0)
    loss = f(-ll.mean())
    # the sample-owned pass: u over the other classes in float32, the labelled term in double
    u = np.zeros((N, K), dtype=f)
    i0 = 16 * ((K - 1) // 16) if mutation == "drop_row_block" else K
    for c in range(C):
        rc = gs * p[:, c] if mutation == "label_in_u" else np.where(own[:, c], f(0), r[:, c])
        u += ((rc[:, None] * Y[c])[:, :i0] @ W[c][:i0]).astype(f)
    dd = Z[rows] - mu[y]                                                    # the finish forms the difference in double
    Wy = W[y].astype(np.float64)
    t = np.einsum("nik,ni->nk", Wy, np.einsum("nij,nj->ni", Wy, dd))
    scale = float(f(lh.UPSTREAM)) / n_div * -label_factor.astype(np.float64)
    gZ = (scale[:, None] * t - u.astype(np.float64)).astype(f)
    # the class-owned pass: float32 sums over the samples, the finish in double
    gmu, gcov = np.empty((C, K), dtype=f), np.empty((C, K, K), dtype=f)
    for c in range(C):
        ry = r[:, c, None] * Y[c]
        v, M, R = ry.sum(0, dtype=f), (ry.T @ Y[c]).astype(f), r[:, c].sum(dtype=f)
        Wd = W[c].astype(np.float64)
        H = M.astype(np.float64) - (0.0 if mutation == "no_trace" else float(R)) * np.eye(K)
        gmu[c] = Wd.T @ v.astype(np.float64)
        gcov[c] = 0.5 * Wd.T @ H @ Wd
    return dict(ll=ll.astype(f), loss=loss, gZ=gZ, gmu=gmu, gcov=gcov)


def _ratios(ref, got, quantities=lh.QUANTITIES):
    b = lh.bounds(ref, "float32")
    out = {}
    for q in quantities:
        with np.errstate(invalid="ignore"):
            ratio = np.abs(np.asarray(got[q], dtype=np.float64).astype(LD) - ref[q]) / b[q]
        out[q] = float(np.nanmax(ratio))   # 0 / 0 only where a zero-weight class has the bound 0 and the value 0
    return out


def test_float32_model_stays_inside_every_bound():
    worst = {}
    for label, ref in _all_cases():
        got = model32(ref)
        ratios = _ratios(ref, got)
        key = "priors" if label.startswith("priors") else label.split()[0]
        for q, v in ratios.items():
            worst[key, q] = max(worst.get((key, q), 0.0), v)
        assert max(ratios.values()) <= 1, (label, ratios)
        zero = np.isneginf(ref["log_priors"])
        assert not got["gmu"][zero].any() and not got["gcov"][zero].any()
    for key in dict.fromkeys(k for k, _ in worst):
        print(f"log-loss-hard float32 model {key}: worst error / bound "
              + " ".join(f"{q} {worst[key, q]:.3f}" for q in lh.QUANTITIES))
    print(f"log-loss-hard float32 model: worst ratio {max(worst.values()):.3f}")


def _mutation_factor(ref, mutation):
    ratios = _ratios(ref, model32(ref, mutation), GRADS)
    q = max(ratios, key=ratios.get)
    return ratios[q], q


def _todays_metric(ref, mutation):
    """max error / max |gradient| per tensor: what tests/test_gpu_log_loss.py holds to 1e-5 in float32."""
    got = model32(ref, mutation)
    return {q: float(np.abs(got[q].astype(np.float64).astype(LD) - ref[q]).max() / np.abs(ref[q]).max()) for q in GRADS}


@pytest.mark.parametrize("K", [5, 17, 33])
@pytest.mark.parametrize("layout", ["round-robin", "mislabelled"])
def test_mutation_a_labelled_residual_as_p_minus_1(layout, K):
    ref = lh.reference("confident", 9, K, lh.N_SAMPLES, layout)
    factor, q = _mutation_factor(ref, "p_minus_1")
    today = _todays_metric(ref, "p_minus_1")
    passes = all(v <= 1e-5 for v in today.values())
    print(f"log-loss-hard mutation (a) p - 1, confident {layout} K={K}: {factor:.3g} x the bound ({q}); whole-tensor metric "
          + " ".join(f"{k} {v:.1e}" for k, v in today.items()) + f": {'passes' if passes else 'fails'} the 1e-5 rule")
    assert factor > 1


@pytest.mark.parametrize("level", list(lh.LEVELS))
def test_mutation_b_labelled_class_in_u(level):
    ref = lh.reference(level, 9, 17)
    factor, q = _mutation_factor(ref, "label_in_u")
    print(f"log-loss-hard mutation (b) labelled class in u, {level} K=17: {factor:.3g} x the bound ({q})")
    assert factor > 1 and q == "gZ"


@pytest.mark.parametrize("K", [17, 33])
@pytest.mark.parametrize("level", list(lh.LEVELS))
def test_mutation_c_dropped_row_block(level, K):
    ref = lh.reference(level, 9, K)
    factor, q = _mutation_factor(ref, "drop_row_block")
    print(f"log-loss-hard mutation (c) last row block of the second product dropped, {level} K={K}: {factor:.3g} x the bound")
    assert factor > 1 and q == "gZ"


@pytest.mark.parametrize("level", list(lh.LEVELS))
def test_mutation_d_no_trace_term(level):
    ref = lh.reference(level, 9, 17)
    factor, q = _mutation_factor(ref, "no_trace")
    print(f"log-loss-hard mutation (d) - R I left out, {level} K=17: {factor:.3g} x the bound")
    assert factor > 1 and q == "gcov"


@pytest.mark.parametrize("level", list(lh.LEVELS))
def test_mutation_e_division_by_padded_n(level):
    ref = lh.reference(level, 9, 17)
    ratios = _ratios(ref, model32(ref, "n_padded"), GRADS)
    print(f"log-loss-hard mutation (e) N rounded up to 64, {level} K=17: "
          + " ".join(f"{q} {v:.3g}" for q, v in ratios.items()) + " x the bound")
    assert min(ratios.values()) > 1


def test_oracle_meets_its_own_rule():
    """The float64 rule of the GPU test, applied to the oracle it is made of: holds by construction, with the factor 5."""
    ref = lh.reference("contested-c1e6", 9, 17)
    got = log_loss_oracle.evaluate(ref["Z"], ref["labels"], ref["mu"], ref["cov"], None, lh.UPSTREAM)
    b = lh.bounds(ref, "float64")
    for q in lh.QUANTITIES:
        assert (np.abs(np.asarray(got[q]).astype(LD) - ref[q]) <= b[q]).all()
