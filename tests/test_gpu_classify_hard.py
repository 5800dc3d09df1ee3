"""GPU tests of the native Gaussian class scores (gauss_factor_kernel, gauss_scores_kernel, gauss_merge_kernel through
sqfa_amd.classify) per entry on the hard inputs of tests/classify_hard.py: condition numbers up to 1e6, means 1e3 from the
origin, samples 30 sigma out, data at scale 1e-4 and 1e4, prior edges and a near-singular class.

Matrix: every level x K in classify_hard.SIZES (both sides of every 16-row block; four classes per stage up to K = 32, one
above) x C in (9, 3) x both dtypes at N = 150 (two full 64-sample tiles and a partial wave of 22).  C = 9: two groups of 4 and
a tail of 1, split 3 ways over the 3 tiles, so gauss_merge_kernel runs; C = 3: one group, never split, the workgroup writes the
results itself.

Accuracy, against the long double truth (checked against mpmath by tests/test_classify_hard.py), per entry:
  float32   |got - S[n, c]| <= bound32[n, c], the a priori forward bound of the documented arithmetic (classify_hard's
            docstring); the evidence within max_c bound32 + (C + 4) u (1 + |E|)
  float64   |err| / (1 + |value|) <= max(1e-10, 5 x yardstick), the yardstick being the numpy float64 oracle's error against
            the truth in the same metric, per case; never anything a kernel returned
Predictions equal the truth on every decided sample (the winner leads by more than the two entries' bounds together;
test_classify_hard.py caps the undecided at 2 %), and the index equals the argmax of the scores the same call wrote.  Worst
error, its bound and the ratio are printed and recorded.  ACCURACY_DROPPED would list (level, dtype) whose kernels miss the
bound for a reason of arithmetic with the measured ratio ("Class scores on hard inputs"); finiteness, the counter
and the decided predictions still hold for such a case.  It is empty: no case misses."""
import math

import numpy as np
import pytest
import torch

import classify_hard as ch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"float32": torch.float32, "float64": torch.float64}
LD = np.longdouble
# (level, dtype) -> worst measured error / bound
ACCURACY_DROPPED = {}


def _classifier(ref, dtype, weights=None):
    from sqfa_amd import classify
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    clf = classify.GaussianClassifier(t(ref["mu"]), t(ref["cov"]), None if weights is None else list(weights))
    assert clf._factors is not None, "the native factor pass did not run"
    return clf, t(ref["Z"])


def _ld(t):
    return t.double().cpu().numpy().astype(LD)


def _check(ref, dtype, weights, label, record_property):
    """Everything the issue asks of one case; returns the accuracy failures (the other conditions are asserted here)."""
    clf, Z = _classifier(ref, dtype, weights)
    S_t, A_t, E_t, bad = clf._native_call(Z, scores=True, argmax=True, logsumexp=True)
    pred = clf.predict(Z).cpu().numpy()
    assert int(bad.item()) == 0, label
    assert torch.equal(A_t, S_t.argmax(1)), label          # the index is the argmax of the scores the same call wrote
    S, E = _ld(S_t), _ld(E_t)
    want_S, want_E = ref["S"], ref["E"]
    fin = np.isfinite(want_S)
    assert (S[~fin] == -np.inf).all(), f"{label}: a zero-weight class's score is not -inf"
    assert np.isfinite(S[fin]).all() and np.isfinite(E).all(), label
    err_S, err_E = np.abs(S[fin] - want_S[fin]), np.abs(E - want_E)
    if dtype == "float32":
        bound_S, bound_E = ref["B"][fin], ref["BE"]
    else:
        bound_S, bound_E = ref["tol64_S"] * (1 + np.abs(want_S[fin])), ref["tol64_E"] * (1 + np.abs(want_E))
    failures = []
    for name, err, bound in (("scores", err_S, bound_S), ("evidence", err_E, bound_E)):
        ratio = err / bound
        at = int(ratio.argmax())
        print(f"classify-hard {label} {name}: worst err {float(err[at]):.3e} bound {float(bound[at]):.3e} "
              f"ratio {float(ratio[at]):.3f}")
        record_property(f"{name}_err", float(err[at]))
        record_property(f"{name}_bound", float(bound[at]))
        record_property(f"{name}_ratio", float(ratio[at]))
        if ratio[at] > 1:
            failures.append((label, name, float(err[at]), float(bound[at]), float(ratio[at])))
    sure = ref["decided32" if dtype == "float32" else "decided64"]
    assert np.array_equal(pred[sure], ref["pred"][sure]), label
    assert np.array_equal(A_t.cpu().numpy()[sure], ref["pred"][sure]), label
    if weights is not None:
        assert not np.isin(pred, np.nonzero(np.asarray(weights) == 0)[0]).any(), f"{label}: a zero-weight class predicted"
    return failures


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K", ch.SIZES)
@pytest.mark.parametrize("C", ch.CLASS_COUNTS)
@pytest.mark.parametrize("level", list(ch.LEVELS))
def test_hard_scores(level, C, K, dtype, record_property):
    ref = ch.reference(level, C, K)
    assert np.isfinite(ref["S"]).all()
    failures = _check(ref, dtype, None, f"{level} C={C} K={K} {dtype}", record_property)
    if (level, dtype) in ACCURACY_DROPPED:
        failures = []
    assert not failures, failures


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("edge", list(ch.PRIOR_EDGES))
def test_prior_edges(edge, dtype, record_property):
    """Whole splits, a whole lane quarter and all classes but one at zero weight (classify_hard.PRIOR_EDGES)."""
    ref, weights = ch.prior_edge(edge)
    zero = np.asarray(weights) == 0
    assert np.array_equal(np.isneginf(ref["S"]), np.broadcast_to(zero, ref["S"].shape)) and np.isfinite(ref["E"]).all()
    failures = _check(ref, dtype, weights, f"priors {edge} {dtype}", record_property)
    assert not failures, failures


@pytest.mark.parametrize("ridge", [0.0, 1e-5], ids=["singular", "ridge1e-5"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_counters_agree_on_a_near_singular_class(dtype, ridge):
    """Class 2 is A A^T with A (K, K - 1): singular before it is rounded to float32 (and the same plus 1e-5 I, which the
    rounding does not drown).  Either the factor pass refuses it (then it counts 1 class and writes NaN for it) or it factors
    (then the counter of a call is the number of score rows with a NaN and the index is -1 exactly there)."""
    from sqfa_amd import _lib, _native, classify
    C, K, N = 5, 8, ch.N_SAMPLES
    Z, _, mu, cov = ch.problem("base", C, K, N, seed=11)
    A = np.random.default_rng(12).standard_normal((K, K - 1))
    low = (A @ A.T + ridge * np.eye(K)).astype(np.float32).astype(np.float64)
    cov[2] = 0.5 * (low + low.T)
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    try:
        clf = classify.GaussianClassifier(t(mu), t(cov))
    except ValueError as err:
        assert "1 of 5 classes" in str(err)
        lib = _lib.load()
        mu_t, cov_t = t(mu), t(cov)
        lp = torch.full((C,), -math.log(C), dtype=torch.float64, device=DEV)
        with _native._on_stream(cov_t.device) as stream:
            W = torch.empty_like(cov_t)
            offset = torch.empty(C, dtype=torch.float64, device=DEV)
            bad = torch.empty(1, dtype=torch.int32, device=DEV)
            _lib.check(lib.sqfa_gauss_class_factors(_native._ptr(mu_t), _native._ptr(cov_t), _native._ptr(lp), C, K,
                                                    _native._dtype_code(cov_t), _native._ptr(W), _native._ptr(offset),
                                                    _native._ptr(bad), stream), "sqfa_gauss_class_factors")
        assert int(bad.item()) == 1
        good = [0, 1, 3, 4]
        assert torch.isnan(W[2]).all() and torch.isnan(offset[2])
        assert torch.isfinite(W[good]).all() and torch.isfinite(offset[good]).all()
        print(f"near-singular class {dtype}: refused by the factor pass")
        return
    assert clf._factors is not None
    S, A_t, E, bad = clf._native_call(t(Z), scores=True, argmax=True, logsumexp=True)
    rows = torch.isnan(S).any(1)
    print(f"near-singular class {dtype}: factored; {int(rows.sum())} of {N} score rows hold a NaN")
    assert int(bad.item()) == int(rows.sum())
    assert torch.equal(A_t == -1, rows) and torch.equal(torch.isnan(E), rows)
    assert torch.equal(A_t[~rows], S[~rows].argmax(1))
