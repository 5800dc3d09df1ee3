"""CPU tests of tests/classify_hard.py, so that tests/test_gpu_classify_hard.py cannot pass for the wrong reason: the inputs are
what they claim, the long double truth agrees with a 50-digit mpmath evaluation of the defining formula to a tenth of the
smallest bound asserted with it, a float32 model of the kernel's documented arithmetic (numpy on the CPU, not the kernel) stays
inside bound32 and leaves it when it is made subtly wrong, the bound leaves at most 2 % of the samples undecided, and the
package's torch expression in float64 meets the float64 rule of the GPU test."""
import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular

import classify_hard as ch

MATRIX = [(level, C, K) for level in ch.LEVELS for C in ch.CLASS_COUNTS for K in ch.SIZES]
U32 = float(ch.U32)


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("K", [1, 5, 17, 64])
@pytest.mark.parametrize("level", list(ch.LEVELS))
def test_input_properties(level, K):
    cond, shift, far, s = ch.LEVELS[level]
    C, N = 5, 40
    Z, labels, mu, cov = ch.problem(level, C, K, N, seed=K)
    for a in (Z, mu, cov):
        assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(labels, np.arange(N) % C)
    lam = np.linalg.eigvalsh(cov / (s * s))
    assert lam.min() > 0
    got = lam[:, -1] / lam[:, 0]
    assert (got <= 2 * cond).all() and (got >= cond / 2).all() or K == 1, got
    assert np.abs(mu / s - shift).max() <= 0.3 * 6
    W, _ = ch.factors(cov, ch.log_priors(None, C))
    r = np.sqrt((np.einsum("nij,nj->ni", W[labels], (Z - mu[labels]).astype(np.longdouble)) ** 2).sum(1) / K).astype(float)
    assert 0.2 * far <= np.median(r) <= 2.5 * far, np.median(r)   # samples `far` standard deviations out, from their class


# ---------------------------------------------------------------------------------------------------------------------
def _mp_scores(Z, mu, cov, lp):
    """log p(z, c) = -1/2 d^T Sigma^-1 d - 1/2 log det Sigma - K/2 log 2 pi + log pi_c and its logsumexp, 50 digits."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    N, K = Z.shape
    C = cov.shape[0]
    S = [[None] * C for _ in range(N)]
    for c in range(C):
        A = mpmath.matrix(cov[c].tolist())
        P, ld = mpmath.inverse(A), mpmath.log(mpmath.det(A))
        for n in range(N):
            d = mpmath.matrix((Z[n]).tolist()) - mpmath.matrix(mu[c].tolist())
            S[n][c] = -(d.T * P * d)[0, 0] / 2 - ld / 2 - K * mpmath.log(2 * mpmath.pi) / 2 + mpmath.mpf(float(lp[c]))
    E = []
    for n in range(N):
        m = max(S[n])
        E.append(m + mpmath.log(sum(mpmath.exp(v - m) for v in S[n])))
    return S, E


@pytest.mark.parametrize("K", [4, 8, 17])
@pytest.mark.parametrize("level", list(ch.LEVELS))
def test_truth_against_mpmath(level, K):
    """Per entry the truth's own error is at most a tenth of the smaller of the float32 bound and the float64 bound."""
    mpmath = pytest.importorskip("mpmath")
    C, N = 3, 12
    ref = ch.reference(level, C, K, N, (1.0, 2.0, 3.0))
    S_mp, E_mp = _mp_scores(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"])
    worst = 0.0
    for n in range(N):
        for got, want, b32, tol in [(ref["S"][n, c], S_mp[n][c], ref["B"][n, c], ref["tol64_S"]) for c in range(C)] + \
                                   [(ref["E"][n], E_mp[n], ref["BE"][n], ref["tol64_E"])]:
            # the long double as an exact mpmath number: high part + remainder
            hi = float(got)
            err = abs(mpmath.mpf(hi) + mpmath.mpf(float(got - np.longdouble(hi))) - want)
            bound = min(float(b32), tol * (1 + abs(hi)))
            worst = max(worst, float(err) / bound)
            assert err <= 0.1 * bound, (level, K, n, float(err), bound)
    print(f"classify-hard truth against mpmath {level} K={K}: worst error / smallest bound {worst:.2e} (allowed 0.1), "
          f"float64 tolerances {ref['tol64_S']:.1e} {ref['tol64_E']:.1e}")


# ---------------------------------------------------------------------------------------------------------------------
def model32(Z, mu, cov, lp, mutation=None):
    """The kernel's documented arithmetic on the CPU: Cholesky and inverse in double, W rounded to float32, z - mu, the product
    and the sum of squares in float32, the double offset rounded to float32; the evidence by a float32 logsumexp.
    mutation "drop_last_k": the last contraction step is left out; "mean_after": W z - W mu in float32."""
    C, K = cov.shape[0], cov.shape[-1]
    f = np.float32
    S = np.empty((Z.shape[0], C), dtype=f)
    for c in range(C):
        L = np.linalg.cholesky(cov[c])
        W = np.tril(solve_triangular(L, np.eye(K), lower=True)).astype(f)
        off = f(-np.log(np.diag(L)).sum() - 0.5 * K * np.log(2.0 * np.pi) + lp[c])
        if mutation == "mean_after":
            y = Z.astype(f) @ W.T - (W @ mu[c].astype(f))[None]
        else:
            d = Z.astype(f) - mu[c].astype(f)
            kk = K - 1 if mutation == "drop_last_k" else K
            y = d[:, :kk] @ W[:, :kk].T
        assert y.dtype == f
        S[:, c] = f(-0.5) * (y * y).sum(1, dtype=f) + off
    m = S.max(1)
    E = m + np.log(np.exp(S - m[:, None]).sum(1, dtype=f))
    assert S.dtype == f and E.dtype == f
    return S, E


def _ratios(ref, S, E):
    fin = np.isfinite(ref["S"])
    rs = (np.abs(S[fin].astype(np.longdouble) - ref["S"][fin]) / ref["B"][fin]).max()
    re = (np.abs(E.astype(np.longdouble) - ref["E"]) / ref["BE"]).max()
    return float(rs), float(re)


def test_float32_model_stays_inside_the_bound():
    worst = {}
    for level, C, K in MATRIX:
        ref = ch.reference(level, C, K)
        rs, re = _ratios(ref, *model32(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"]))
        ws, we = worst.get(level, (0.0, 0.0))
        worst[level] = (max(ws, rs), max(we, re))
        assert rs < 1 and re < 1, (level, C, K, rs, re)
    for level, (rs, re) in worst.items():
        print(f"classify-hard float32 model {level}: worst error / bound scores {rs:.3f} evidence {re:.3f}")
    for edge in ch.PRIOR_EDGES:
        ref, _ = ch.prior_edge(edge)
        S, E = model32(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"])
        rs, re = _ratios(ref, S, E)
        print(f"classify-hard float32 model priors {edge}: error / bound scores {rs:.3f} evidence {re:.3f}")
        assert rs < 1 and re < 1 and np.array_equal(np.isneginf(S), np.isneginf(ref["S"])), (edge, rs, re)


@pytest.mark.parametrize("level", list(ch.LEVELS))
def test_a_dropped_contraction_step_leaves_the_bound(level):
    for C in ch.CLASS_COUNTS:
        ref = ch.reference(level, C, 17)
        rs, _ = _ratios(ref, *model32(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"], "drop_last_k"))
        print(f"classify-hard mutation drop_last_k {level} C={C} K=17: error / bound {rs:.3g}")
        assert rs > 1


@pytest.mark.parametrize("K", ch.SIZES[1:])
def test_a_mean_subtracted_after_the_product_leaves_the_bound(K):
    """Not K = 1: there Sigma = 1 and W = 1 exactly, and W z - W mu = z - mu is the same float32 number."""
    for C in ch.CLASS_COUNTS:
        ref = ch.reference("farmean", C, K)
        rs, _ = _ratios(ref, *model32(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"], "mean_after"))
        print(f"classify-hard mutation mean_after farmean C={C} K={K}: error / bound {rs:.3g}")
        assert rs > 1


def test_exclusion_cap():
    """From truth and bound alone: at most 2 % of the samples are undecided, in either dtype's rule."""
    for level in ch.LEVELS:
        worst = (0.0, (0, 0))
        for C in ch.CLASS_COUNTS:
            for K in ch.SIZES:
                ref = ch.reference(level, C, K)
                share = max(1 - ref["decided32"].mean(), 1 - ref["decided64"].mean())
                worst = max(worst, (share, (C, K)))
                assert share <= ch.EXCLUSION_CAP, (level, C, K, share)
        print(f"classify-hard undecided samples {level}: worst share {worst[0]:.2%} at (C, K) = {worst[1]}")
    for edge in ch.PRIOR_EDGES:
        ref, _ = ch.prior_edge(edge)
        share = max(1 - ref["decided32"].mean(), 1 - ref["decided64"].mean())
        print(f"classify-hard undecided samples priors {edge}: share {share:.2%}")
        assert share <= ch.EXCLUSION_CAP, (edge, share)


def test_float64_yardstick():
    """The numpy float64 oracle against the truth; what the GPU test's float64 bound is made of."""
    for level in ch.LEVELS:
        refs = [ch.reference(level, C, K) for C in ch.CLASS_COUNTS for K in ch.SIZES]
        ys, ye = max(r["yard_S"] for r in refs), max(r["yard_E"] for r in refs)
        print(f"classify-hard float64 oracle {level}: worst |err| / (1 + |value|) scores {ys:.2e} evidence {ye:.2e}")
        assert ys < 1e-6 and ye < 1e-6   # the oracle is a float64 evaluation, not a float32 one


@pytest.mark.parametrize("weights", [(0.0, 1e-300, 1.0), (1.0, 2.0, 3.0), [1, 2, 4]])
def test_prior_weights_are_normalised_in_float64(weights):
    """Python numbers go to float64, not through torch's default dtype: 1e-300 is not zero, 1/6 not a float32 number."""
    from sqfa_amd import classify
    for dtype in (torch.float32, torch.float64):
        clf = classify.GaussianClassifier(None, torch.eye(2, dtype=dtype).expand(3, 2, 2), weights)
        got, want = clf.log_priors.numpy(), ch.log_priors(weights, 3)
        assert clf.log_priors.dtype == torch.float64 and np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max() <= 4 * np.finfo(np.float64).eps * (1 + np.abs(want[fin]).max())


@pytest.mark.parametrize("edge", list(ch.PRIOR_EDGES))
def test_package_torch_expression_float64_prior_edges(edge):
    from sqfa_amd import classify
    ref, weights = ch.prior_edge(edge)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    clf = classify.GaussianClassifier(t(ref["mu"]), t(ref["cov"]), list(weights))
    S, E = clf.scores(t(ref["Z"])).numpy(), clf.log_evidence(t(ref["Z"])).numpy()
    assert np.array_equal(np.isneginf(S), np.isneginf(ref["S"])) and np.isfinite(E).all()
    assert float(ch.rel(S, ref["S"]).max()) <= ref["tol64_S"] and float(ch.rel(E, ref["E"]).max()) <= ref["tol64_E"]
    pred = clf.predict(t(ref["Z"])).numpy()
    assert np.array_equal(pred[ref["decided64"]], ref["pred"][ref["decided64"]])
    assert not np.isin(pred, np.nonzero(np.asarray(weights) == 0)[0]).any()


@pytest.mark.parametrize("C", ch.CLASS_COUNTS)
@pytest.mark.parametrize("level", list(ch.LEVELS))
def test_package_torch_expression_float64(level, C):
    from sqfa_amd import classify
    ref = ch.reference(level, C, 17)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    clf = classify.GaussianClassifier(t(ref["mu"]), t(ref["cov"]))
    assert clf._factors is None
    Z = t(ref["Z"])
    rs = float(ch.rel(clf.scores(Z).numpy(), ref["S"]).max())
    re = float(ch.rel(clf.log_evidence(Z).numpy(), ref["E"]).max())
    print(f"classify-hard torch float64 {level} C={C}: scores {rs:.2e} (allowed {ref['tol64_S']:.1e}), "
          f"evidence {re:.2e} (allowed {ref['tol64_E']:.1e})")
    assert rs <= ref["tol64_S"] and re <= ref["tol64_E"]
    sure = ref["decided64"]
    assert np.array_equal(clf.predict(Z).numpy()[sure], ref["pred"][sure])
