"""GPU tests of the native nested Gaussian class scores (gauss_nested_factor_kernel, gauss_nested_kernel,
gauss_nested_merge_kernel, gauss_nested_label_kernel through sqfa_amd.classify) per entry, against the long double truth of
every prefix (tests/nested_oracle.py: classify_hard.truth_and_bound32 on the leading k features).

Matrix: levels base, c1e3, farmean, farsample x K in classify_hard.SIZES (both sides of every 16-row block; four classes per
stage up to K = 32, one above) x C in (9, 3) x both dtypes at N = 150 (two full 64-sample tiles and a partial wave of 22).
C = 9: two groups of 4 and a tail of 1, split 3 ways over the 3 tiles, so gauss_nested_merge_kernel runs; C = 3: one group,
never split, the workgroup writes the results itself.

Per entry and column k - 1:
  float32   the evidence within evidence_bound32 of the truth of the first k features; the labelled log posterior within the
            bound of its score plus the bound of its evidence
  float64   the same with tol64 (1 + |value|), tol64 = max(1e-10, 5 x the float64 yardstick of the case)
Predictions equal the truth on every sample decided for that prefix; the undecided share per column is capped at
classify_hard.EXCLUSION_CAP (on these inputs the long double reference leaves out at most 1 of 150 in any column)."""
import numpy as np
import pytest
import torch

import classify_hard as ch
import nested_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"float32": torch.float32, "float64": torch.float64}
LEVELS = ("base", "c1e3", "farmean", "farsample")
LD = np.longdouble


def _classifier(ref, dtype, weights=None, zero_means=False):
    from sqfa_amd import classify
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    clf = classify.GaussianClassifier(None if zero_means else t(ref["mu"]), t(ref["cov"]),
                                      None if weights is None else list(weights))
    assert clf._factors is not None, "the native factor pass did not run"
    Z = t(ref["Z"])
    assert clf._use_nested_native(Z), "the native nested path does not apply"
    return clf, Z, torch.tensor(ref["labels"], device=DEV)


def _ld(t):
    return t.double().cpu().numpy().astype(LD)


def _worst(label, name, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"nested {label} {name}: worst err {float(err[at]):.3e} bound {float(bound[at]):.3e} ratio {float(ratio[at]):.3f} "
          f"at (n, k) = ({at[0]}, {at[1] + 1})")
    return float(ratio[at])


def _check(want, dtype, label, weights=None, zero_means=False):
    """Everything asked of one case."""
    clf, Z, y = _classifier(want["ref"], dtype, weights, zero_means)
    N, K = Z.shape
    A_t, E_t, ll_t, flags = clf._nested(Z, argmax=True, logsumexp=True, labels=y)
    assert flags.tolist() == [0, 0, 0], label
    assert A_t.shape == E_t.shape == ll_t.shape == (N, K) and A_t.dtype == torch.int64, label
    # bitwise: a second call, and each output alone against the same output computed alongside the others
    A2, E2, ll2, _ = clf._nested(Z, argmax=True, logsumexp=True, labels=y)
    assert torch.equal(A_t, A2) and torch.equal(E_t, E2) and torch.equal(ll_t, ll2), label
    pred_t = clf.nested_predict(Z)
    assert torch.equal(pred_t, A_t) and torch.equal(clf.nested_log_evidence(Z), E_t), label
    assert torch.equal(clf.nested_label_log_proba(Z, y), ll_t), label

    E, ll = _ld(E_t), _ld(ll_t)
    assert np.isfinite(E).all() and np.isfinite(ll).all() and (ll <= 0).all(), label
    if dtype == "float32":
        bound_E, bound_ll = want["BE"], want["By"] + want["BE"]
    else:
        bound_E = want["tol64_E"] * (1 + np.abs(want["E"]))
        bound_ll = want["tol64_S"] * (1 + np.abs(want["Sy"])) + bound_E
    ratio_E = _worst(label, "evidence", np.abs(E - want["E"]), bound_E)
    ratio_ll = _worst(label, "label log posterior", np.abs(ll - want["ll"]), bound_ll)
    assert ratio_E <= 1 and ratio_ll <= 1, (label, ratio_E, ratio_ll)

    sure = want["decided32" if dtype == "float32" else "decided64"]
    assert (~sure).mean(0).max() <= ch.EXCLUSION_CAP, label
    assert np.array_equal(pred_t.cpu().numpy()[sure], want["pred"][sure]), label
    if weights is not None:
        assert not np.isin(pred_t.cpu().numpy(), np.nonzero(np.asarray(weights) == 0)[0]).any(), label

    acc, loss = clf.nested_accuracy(Z, y), clf.nested_log_loss(Z, y)
    assert acc.shape == loss.shape == (K,) and acc.dtype == loss.dtype == torch.float64 and not acc.is_cuda, label
    # the sums on the device, the division where the methods do it: on the host
    assert torch.equal(acc, (A_t == y[:, None]).sum(0).cpu().double() / N), label
    assert torch.equal(loss, -ll_t.double().sum(0).cpu() / N), label
    assert torch.equal(loss, clf.nested_log_loss(Z, y)), label


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K", ch.SIZES)
@pytest.mark.parametrize("C", ch.CLASS_COUNTS)
@pytest.mark.parametrize("level", LEVELS)
def test_nested_against_the_truth(level, C, K, dtype):
    _check(nested_oracle.prefixes(level, C, K), dtype, f"{level} C={C} K={K} {dtype}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("edge", list(ch.PRIOR_EDGES))
def test_prior_edges(edge, dtype):
    """Whole splits, a whole lane quarter and all classes but one at zero weight (classify_hard.PRIOR_EDGES), K = 5.  The
    labels of the oracle (n % C) fall on zero-weight classes, which the label pass refuses: the labelled entries are checked
    on labels moved to the nearest class with weight."""
    C, weights = ch.PRIOR_EDGES[edge]
    want = dict(nested_oracle.prefixes(ch.PRIOR_EDGE_LEVEL, C, ch.PRIOR_EDGE_K, ch.N_SAMPLES, weights))
    ref = want["ref"]
    live = np.nonzero(np.asarray(weights) > 0)[0]
    labels = live[np.abs(ref["labels"][:, None] - live[None]).argmin(1)]
    moved = nested_oracle.evaluate(ref["Z"], ref["mu"], ref["cov"], ref["log_priors"], labels, want["tol64_S"])
    assert np.array_equal(moved["pred"], want["pred"]) and np.isfinite(moved["ll"]).all()
    moved.update(ref=dict(ref, labels=labels), tol64_S=want["tol64_S"], tol64_E=want["tol64_E"])
    _check(moved, dtype, f"priors {edge} {dtype}", weights=weights)
    clf, Z, y = _classifier(ref, dtype, weights)
    zero = int((np.asarray(weights)[ref["labels"]] == 0).sum())
    with pytest.raises(ValueError, match=f"{zero} labels belong to a class with prior 0"):
        clf.nested_log_loss(Z, y)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C,K", [(9, 17), (3, 33), (9, 64)])
def test_zero_means(C, K, dtype):
    _check(nested_oracle.prefixes("c1e3", C, K, zero_means=True), dtype, f"zero means C={C} K={K} {dtype}", zero_means=True)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K", [5, 17, 64])
def test_ties_go_to_the_lowest_index_in_every_column(K, dtype):
    """Twins in the same class group (2, 3) and in the groups of two and of three different splits (1, 4, 8; every group of
    4 classes is its own split here): the same Gaussian gives the same bits wherever it is scored, and the lowest index
    wins."""
    from sqfa_amd import classify
    ref = ch.reference("base", 9, K)
    twin = [0, 1, 2, 2, 1, 5, 6, 7, 1]
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    clf = classify.GaussianClassifier(t(ref["mu"][twin]), t(ref["cov"][twin]))
    A = clf.nested_predict(t(ref["Z"])).cpu().numpy()
    assert not np.isin(A, (3, 4, 8)).any()
    assert (A == 1).any() and (A == 2).any()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C,K,feature", [(9, 5, 3), (3, 17, 3), (9, 33, 20), (3, 64, 63)])
def test_a_nan_refuses_the_whole_sample_and_counts_it_once(C, K, feature, dtype):
    """Samples 0, 63, 64 and 149 (the ends of a full tile, the start of the next, the last of a partial wave) with a NaN in
    one feature: all K columns are -1 / NaN, also those of the prefixes before the feature, and the device counter is 4."""
    want = nested_oracle.prefixes("base", C, K)
    clf, Z, y = _classifier(want["ref"], dtype)
    hit = [0, 63, 64, 149]
    Z[hit, feature] = float("nan")
    A, E, ll, flags = clf._nested(Z, argmax=True, logsumexp=True, labels=y)
    assert flags.tolist() == [4, 0, 0]
    rows = torch.zeros(Z.shape[0], dtype=torch.bool, device=DEV)
    rows[hit] = True
    rows = rows[:, None].expand(-1, K)
    assert torch.equal(A == -1, rows) and torch.equal(torch.isnan(E), rows) and torch.equal(torch.isnan(ll), rows)
    clean = clf._nested(torch.tensor(want["ref"]["Z"], dtype=DTYPES[dtype], device=DEV), argmax=True, logsumexp=True)
    assert torch.equal(A[~rows], clean[0][~rows]) and torch.equal(E[~rows], clean[1][~rows])   # the neighbours' bits stay
    assert clf._nested(Z, argmax=True)[3].tolist() == [4, 0, 0] and clf._nested(Z, logsumexp=True)[3].tolist() == [4, 0, 0]
    for call in (lambda: clf.nested_predict(Z), lambda: clf.nested_log_evidence(Z), lambda: clf.nested_accuracy(Z, y),
                 lambda: clf.nested_label_log_proba(Z, y), lambda: clf.nested_log_loss(Z, y)):
        with pytest.raises(ValueError, match="4 samples have non-finite scores"):
            call()


def _factor_passes(mu, cov, lp):
    """(W, offset (C,), bad) of sqfa_gauss_class_factors and (W, offsets (C, K), bad) of sqfa_gauss_class_factors_nested."""
    from sqfa_amd import _lib, _native
    lib = _lib.load()
    C, K = cov.shape[0], cov.shape[-1]
    out = []
    with _native._on_stream(cov.device) as stream:
        for fn, shape in ((lib.sqfa_gauss_class_factors, (C,)), (lib.sqfa_gauss_class_factors_nested, (C, K))):
            W = torch.full_like(cov, 7.0)
            offset = torch.full(shape, 7.0, dtype=torch.float64, device=DEV)
            bad = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            _lib.check(fn(_native._ptr(mu), _native._ptr(cov), _native._ptr(lp), C, K, _native._dtype_code(cov),
                          _native._ptr(W), _native._ptr(offset), _native._ptr(bad), stream), "factor pass")
            out.append((W, offset, int(bad.item())))
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("level,C,K", [("base", 3, 1), ("c1e3", 9, 17), ("farmean", 9, 33), ("farsample", 3, 64)])
def test_nested_factor_pass(level, C, K, dtype):
    """W bit-equal to the plain factor pass; offsets[:, K - 1] within 1e-14 relative of the plain offset; every offset_k
    against the long double offset of the leading block.  Its bound, with u = 2^-53: the Cholesky factorization in double is
    exact for a matrix perturbed by k u relative to |L||L^T|, which moves a pivot by at most k u cond relatively and the sum
    of k half log-pivots by k^2 u cond / 2 (taken as k^2 u cond); the k + 2 terms are then summed with at most k + 3
    roundings of the sum of their magnitudes (one more for each log)."""
    want = nested_oracle.prefixes(level, C, K)
    ref = want["ref"]
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    lp = torch.tensor(ref["log_priors"], dtype=torch.float64, device=DEV)
    (W, offset, bad), (W_n, offsets, bad_n) = _factor_passes(t(ref["mu"]), t(ref["cov"]).contiguous(), lp)
    assert bad == 0 and bad_n == 0
    assert torch.equal(W, W_n)
    assert ((offsets[:, K - 1] - offset).abs() <= 1e-14 * offset.abs()).all()
    got = offsets.cpu().numpy().astype(LD)
    u, k = LD(2.0) ** -53, np.arange(1, K + 1)
    bound = k * k * u * ch.LEVELS[level][0] + 2 * (k + 3) * u * want["offset_terms"]
    assert (np.abs(got - want["offsets"]) <= bound).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_nested_factor_pass_on_a_bad_class(dtype):
    """An indefinite class: NaN in its W and in all K of its offsets, counted once; the other classes as without it."""
    C, K = 5, 17
    ref = ch.reference("base", C, K)
    cov = ref["cov"].copy()
    cov[2] = -cov[2]
    t = lambda a: torch.tensor(a, dtype=DTYPES[dtype], device=DEV)
    lp = torch.tensor(ref["log_priors"], dtype=torch.float64, device=DEV)
    (W, offset, bad), (W_n, offsets, bad_n) = _factor_passes(t(ref["mu"]), t(cov), lp)
    assert bad == 1 and bad_n == 1
    good = [0, 1, 3, 4]
    assert torch.isnan(W_n[2]).all() and torch.isnan(offsets[2]).all()
    assert torch.equal(W[good], W_n[good]) and torch.isfinite(offsets[good]).all()
    assert ((offsets[good, K - 1] - offset[good]).abs() <= 1e-14 * offset[good].abs()).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_labels_out_of_range_are_counted(dtype):
    """Labels far outside [0, C) are counted and gather class 0: the run ends clean and the other samples keep their bits."""
    want = nested_oracle.prefixes("base", 9, 17)
    clf, Z, y = _classifier(want["ref"], dtype)
    ll = clf.nested_label_log_proba(Z, y)
    wild = y.clone()
    hit = [0, 63, 64, 149]
    wild[hit] = torch.tensor([-1, 9, 2 ** 40, -2 ** 62], device=DEV)
    _, _, got, flags = clf._nested(Z, labels=wild)
    assert flags.tolist() == [0, 4, 0]
    rows = torch.zeros(Z.shape[0], dtype=torch.bool, device=DEV)
    rows[hit] = True
    assert torch.isnan(got[rows]).all() and torch.equal(got[~rows], ll[~rows])
    for method in (clf.nested_log_loss, clf.nested_label_log_proba):
        with pytest.raises(ValueError, match=r"4 labels are outside \[0, 9\)"):
            method(Z, wild)


def test_the_switch_selects_the_torch_expression(monkeypatch):
    from sqfa_amd import classify
    want = nested_oracle.prefixes("base", 9, 17)
    clf, Z, y = _classifier(want["ref"], "float64")
    native = clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_log_loss(Z, y)
    monkeypatch.setattr(classify, "NATIVE_NESTED", False)
    assert not clf._use_nested_native(Z)
    sure = torch.tensor(want["decided64"], device=DEV)
    assert torch.equal(clf.nested_predict(Z)[sure], native[0][sure])
    assert torch.allclose(clf.nested_log_evidence(Z), native[1], rtol=1e-10, atol=1e-10)
    assert torch.allclose(clf.nested_log_loss(Z, y), native[2], rtol=1e-10, atol=1e-10)
