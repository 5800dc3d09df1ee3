"""CPU checks of OAS shrinkage in points mode: ClassPoints(estimator="oas") (coefficients one class at a time, the torch
expression with keep_c cov(F x | c) + shift_c F F^T) against the float64 oracle -- class_statistics_oracle with
estimator="oas", then class_points_oracle's dense projection and autograd --, the coefficient rho itself, that
"empirical" is untouched, a short fit against the dense OAS fit, and the argument checks of the new C entries (fake
non-null pointers: nothing is launched).  Bounds: the project's own for class statistics, 1e-11 / 2e-5."""
import ctypes

import numpy as np
import pytest
import torch

import class_points_oracle as cpo
import class_statistics_oracle as cso
import model_cases as mc
from conftest import rel_err
from sqfa_amd import _lib, statistics
from sqfa_amd.statistics import ClassPoints

Z, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(4096)
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-5)]
INPUTS = {"tailsL3": (lambda: cpo.tails_with_long_class(3), None), "tailsL17": (lambda: cpo.tails_with_long_class(17), None),
          "tailsL65": (lambda: cpo.tails_with_long_class(65), None), "ragged40": (cso.ragged_small, 40)}
_refs = {}


def reference(name):
    """(X, y, n_classes, dense float64 OAS oracle statistics, oracle rho, tr2 / (tr2 - tr^2 / D)) once per session."""
    if name not in _refs:
        make, n_classes = INPUTS[name]
        X, y = make()
        dense = cso.class_statistics(X, y, n_classes=n_classes, estimator="oas")
        C, D = dense["means"].shape
        rho, amp = np.full(C, np.nan), np.full(C, np.nan)
        for c in range(C):
            Xc = X[y == c]
            if Xc.shape[0] >= 2:
                S = cso.sample_covariance(Xc)
                tr, tr2 = np.trace(S), np.sum(S * S)
                rho[c] = min(((1 - 2 / D) * tr2 + tr * tr) / ((Xc.shape[0] + 1 - 2 / D) * (tr2 - tr * tr / D)), 1.0)
                amp[c] = tr2 / (tr2 - tr * tr / D)
        _refs[name] = (X, y, n_classes, dense, rho, amp)
    return _refs[name]


# ---- the torch expression and the coefficients against the oracle ---------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("name", ["ragged40", "tailsL17", "tailsL3", "tailsL65"])
def test_oas_points_against_the_oracle(name, dtype, tol):
    Xn, yn, n_classes, dense, _, _ = reference(name)
    D, K = Xn.shape[1], min(4, Xn.shape[1])
    Fn = cpo.filters(K, D)
    cp = ClassPoints(torch.tensor(Xn, dtype=dtype), torch.tensor(yn), n_classes=n_classes, estimator="oas")
    C = cp.n_classes
    F = torch.tensor(Fn, dtype=dtype, requires_grad=True)
    stats = cp.feature_statistics(F, second_moments=True)
    errs = cpo.check_values(stats, cpo.feature_moments(Xn, yn, Fn, stats=dense), tol, what=name)   # values and NaN pattern
    print(name, dtype, errs)
    some = cp.counts.numpy() > 0
    assert rel_err(cp.means[cp.counts > 0].numpy(), dense["means"][some]) < tol
    A, b = cpo.loss_terms(C, K, seed=5)
    for second in (False, True):
        _, g_ref, keep = cpo.loss_gradient(Xn, yn, Fn, A, b, n_classes=n_classes, second_moments=second, stats=dense)
        F.grad = None
        st = cp.feature_statistics(F, second_moments=second)
        S = st["second_moments" if second else "covariances"]
        kp = torch.tensor(keep)
        L = (torch.tensor(A, dtype=dtype)[kp] * S[kp]).sum() + (torch.tensor(b, dtype=dtype)[kp] * st["means"][kp]).sum()
        L.backward()
        err = rel_err(F.grad.numpy(), g_ref)
        print(name, dtype, "second" if second else "cov", "dL/dF", err)
        assert np.isfinite(F.grad.numpy()).all() and err < tol, (name, second, err)


INPUTS["tailsL5"] = (lambda: cpo.tails_with_long_class(5), None)   # the coefficients only: a second clamped class


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", ["ragged40", "tailsL17", "tailsL3", "tailsL5", "tailsL65"])
def test_shrinkage_equals_the_oracles_rho(name, dtype):
    """float64: 1e-11.  float32: rho is a ratio whose denominator tr2 - tr^2 / D cancels, so an error of the project's bound
    2e-5 in S is amplified by tr2 / (tr2 - tr^2 / D), at most 16 on these inputs."""
    Xn, yn, n_classes, _, rho, amp = reference(name)
    cp = ClassPoints(torch.tensor(Xn, dtype=dtype), torch.tensor(yn), n_classes=n_classes, estimator="oas")
    assert cp.estimator == "oas" and cp.shrinkage.dtype == torch.float64
    assert cp.shrink_keep.dtype == dtype and cp.shrink_shift.dtype == dtype
    got = cp.shrinkage.numpy()
    full = ~np.isnan(rho)
    assert np.array_equal(np.isnan(got), ~full) and np.array_equal(cp.counts.numpy() >= 2, full)
    assert torch.isnan(cp.shrink_keep[~torch.tensor(full)]).all() and torch.isnan(cp.shrink_shift[~torch.tensor(full)]).all()
    assert np.nanmax(amp) <= 16.0
    err = np.abs(got[full] - rho[full])
    print(name, dtype, "rho", np.nanmin(rho), "..", np.nanmax(rho), "max err", err.max(), "amplification", np.nanmax(amp))
    if dtype == torch.float64:
        assert (err < 1e-11).all()
    else:
        assert (err < 2e-5 * amp[full]).all()
    # keep and shift are rho's, rounded once to the dtype
    assert torch.equal(cp.shrink_keep[torch.tensor(full)], (1.0 - cp.shrinkage).to(dtype)[torch.tensor(full)])
    # Three points span two dimensions: with equal eigenvalues rho = (6 - 4/D) / ((4 - 2/D)(2 - 4/D)), 2.1 at D = 3, 1.2 at
    # D = 5 and 0.84 at D = 17.  So the oracle clamps the 3-point class at D = 3 and 5 and not at D = 17 (0.7195 there).
    if name in ("tailsL3", "tailsL5"):
        assert cp.counts[3] == 3 and rho[3] == 1.0 and got[3] == 1.0 and cp.shrink_keep[3] == 0.0
    if name == "tailsL17":
        assert cp.counts[3] == 3 and rho[3] < 1.0 and cp.shrink_keep[3] > 0.0


# ---- "empirical" is what it was ------------------------------------------------------------------------------------------------

def test_empirical_is_unchanged_and_unknown_estimators_are_refused():
    Xn, yn = cso.tails(17)
    X, y = torch.tensor(Xn, dtype=torch.float32), torch.tensor(yn)
    a, b = ClassPoints(X, y), ClassPoints(X, y, estimator="empirical")
    for cp in (a, b):
        assert cp.estimator == "empirical" and cp.shrink_keep is None and cp.shrink_shift is None and cp.shrinkage is None
    F = torch.tensor(cpo.filters(4, 17), dtype=torch.float32)
    sa, sb = a.feature_statistics(F, second_moments=True), b.feature_statistics(F, second_moments=True)
    for k in sa:
        assert torch.equal(torch.nan_to_num(sa[k], nan=-7.0), torch.nan_to_num(sb[k], nan=-7.0))
    for bad in ("OAS", "ledoit_wolf", None, ""):
        with pytest.raises(ValueError, match="estimator"):
            ClassPoints(X, y, estimator=bad)


def test_class_statistics_defaults_to_the_objects_estimator():
    Xn, yn = cso.ragged_small(C=5, D=7, empty=())
    X, y = torch.tensor(Xn), torch.tensor(yn)
    cp = ClassPoints(X, y, estimator="oas")
    assert torch.equal(cp.class_statistics()["covariances"], statistics.class_statistics(X, y, estimator="oas")["covariances"])
    assert torch.equal(cp.class_statistics("empirical")["covariances"], statistics.class_statistics(X, y)["covariances"])
    assert torch.equal(ClassPoints(X, y).class_statistics()["covariances"], statistics.class_statistics(X, y)["covariances"])


def test_one_dimension_has_no_shrinkage_target_and_gives_nan_as_the_dense_statistics():
    """D = 1: tr2 = tr^2, rho = 0 / 0.  The dense OAS statistics are NaN there, and so are the points'."""
    Xn, yn = cso.tails(1)
    X, y = torch.tensor(Xn), torch.tensor(yn)
    cp = ClassPoints(X, y, estimator="oas")
    assert torch.isnan(cp.shrinkage).all() and torch.isnan(cp.shrink_keep).all() and torch.isnan(cp.shrink_shift).all()
    assert torch.isnan(statistics.class_statistics(X, y, estimator="oas")["covariances"]).all()
    st = cp.feature_statistics(torch.ones(1, 1, dtype=torch.float64))
    assert torch.isnan(st["covariances"]).all() and torch.isfinite(st["means"][1:]).all()


# ---- a short fit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["smsqfa", "sqfa"])
def test_short_cpu_fit_from_oas_points_follows_the_dense_oas_fit(kind):
    """3 epochs from the same start, float64, CPU (distances that run there: log_euclidean, bhattacharyya): loss histories
    within 1e-8 and filters within 1e-5, the bounds of test_short_fit_from_points_follows_the_dense_fit."""
    from sqfa_amd import distances
    fn = distances.log_euclidean if kind == "smsqfa" else distances.bhattacharyya
    Xn, yn = cso.ragged_small(C=8, D=24, empty=(), lo=30, hi=60)
    X, y = torch.tensor(Xn), torch.tensor(yn)
    runs = {}
    for mode in ("dense", "points"):
        torch.manual_seed(5)
        model = mc.make_model(kind, 24, 4, 0.01, "sphere", torch.float64, "cpu")
        model.distance_fun = fn
        data = ClassPoints(X, y, estimator="oas") if mode == "points" else statistics.class_statistics(X, y, estimator="oas")
        loss, _ = model.fit(data_statistics=data, max_epochs=3, show_progress=False, return_loss=True)
        runs[mode] = (loss.numpy(), model.filters.detach().numpy())
    assert len(runs["points"][0]) == 3
    assert np.abs(runs["points"][0] - runs["dense"][0]).max() < 1e-8
    assert rel_err(runs["points"][1], runs["dense"][1]) < 1e-5
    # and it is the shrinkage that they share: the empirical fit is somewhere else
    torch.manual_seed(5)
    model = mc.make_model(kind, 24, 4, 0.01, "sphere", torch.float64, "cpu")
    model.distance_fun = fn
    loss, _ = model.fit(data_statistics=ClassPoints(X, y), max_epochs=3, show_progress=False, return_loss=True)
    assert np.abs(loss.numpy() - runs["dense"][0]).max() > 1e-6


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------

def shrinkage(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_shrinkage(g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("class_start", FAKE),
                                            g("C", 3), g("dtype", 0), g("means", FAKE), g("keep", FAKE), g("shift", FAKE),
                                            g("rho", Z), g("ws", FAKE), g("nbytes", 1 << 30), Z)


def forward(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_feature_moments_shrunk(
        g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("row_class", FAKE), g("class_start", FAKE), g("C", 3),
        g("means", FAKE), g("F", FAKE), g("K", 2), g("dtype", 0), 0.0, g("keep", FAKE), g("shift", FAKE), g("zc", FAKE),
        g("means_f", FAKE), g("cov_f", FAKE), g("second_f", Z), g("ws", FAKE), g("nbytes", 1 << 30), Z)


def backward(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_feature_moments_shrunk_backward(
        g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("row_class", FAKE), g("class_start", FAKE), g("C", 3),
        g("means", FAKE), g("F", FAKE), g("zc", FAKE), g("G", FAKE), g("ldg", 2), g("g_means", Z), g("keep", FAKE),
        g("shift", FAKE), g("K", 2), g("dtype", 0), g("n_groups", 4), g("partial", FAKE), g("ws", FAKE), g("nbytes", 1 << 30), Z)


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_shrunk_workspace_query(dtype):
    query = _lib.load().sqfa_class_feature_moments_shrunk_workspace_bytes
    plain = _lib.load().sqfa_class_feature_moments_workspace_bytes
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for N, C, D, K in ((1, 1, 1, 1), (222, 7, 17, 16), (60000, 1000, 784, 16), (60000, 1000, 2048, 32), (50000, 100, 3072, 64),
                       (60000, 10, 784, 16), (1 << 32, 10, 3, 2)):
        nbytes = query(N, C, D, K, dtype)
        assert nbytes >= (N + C + K) * K * esz and nbytes >= C * K * K * esz   # the weights of every virtual row; one Gram per class
        assert nbytes <= max((N + C + K) * K, 32 * C * K * K) * esz + K * K * esz + 16   # never anything of size D
        assert nbytes >= plain(N, C, D, K, dtype)
    for shape in ((10, 3, 5, 65), (-1, 3, 5, 2), (10, 0, 5, 2), (10, 3, 0, 2), (10, 3, 5, 0), (10, 1 << 20, 5, 2)):
        assert plain(*shape, dtype) == 0 and query(*shape, dtype) == 0          # 0 where the existing query is 0
    assert query(10, 3, 5, 2, 7) == 0                                           # bad dtype
    assert query(0, 3, 5, 2, dtype) > 0                                         # no point at all is a valid shape


def test_class_shrinkage_argument_checks():
    for bad in (dict(points=Z), dict(class_start=Z), dict(means=Z), dict(keep=Z), dict(shift=Z), dict(N=-1), dict(C=0),
                dict(D=0), dict(dtype=2), dict(dtype=-1)):
        assert shrinkage(**bad) == -1, bad
    assert shrinkage(C=1 << 20) == -2
    assert shrinkage(ws=Z) == -3 and shrinkage(nbytes=8) == -3
    assert shrinkage(nbytes=_lib.load().sqfa_class_moments_workspace_bytes(3, 5, 0) - 1) == -3
    # in this order: a bad argument wins over an unsupported shape, which wins over a short workspace
    assert shrinkage(dtype=9, C=1 << 20, ws=Z) == -1 and shrinkage(keep=Z, nbytes=8) == -1 and shrinkage(C=1 << 20, ws=Z) == -2


def test_shrunk_feature_moments_argument_checks():
    for bad in (dict(points=Z), dict(row_class=Z), dict(class_start=Z), dict(means=Z), dict(F=Z), dict(keep=Z), dict(shift=Z),
                dict(zc=Z), dict(means_f=Z), dict(cov_f=Z), dict(N=-1), dict(C=0), dict(D=0), dict(K=0), dict(dtype=2),
                dict(dtype=-1)):
        assert forward(**bad) == -1, bad
    assert forward(K=65) == -2 and forward(C=1 << 20) == -2
    assert forward(ws=Z) == -3 and forward(nbytes=8) == -3
    assert forward(dtype=9, K=65, ws=Z) == -1 and forward(keep=Z, nbytes=8) == -1 and forward(K=65, ws=Z) == -2


def test_shrunk_feature_moments_backward_argument_checks():
    for bad in (dict(points=Z), dict(row_class=Z), dict(class_start=Z), dict(means=Z), dict(F=Z), dict(zc=Z), dict(G=Z),
                dict(keep=Z), dict(shift=Z), dict(partial=Z), dict(N=-1), dict(C=0), dict(D=0), dict(K=0), dict(ldg=1),
                dict(n_groups=0), dict(n_groups=65536), dict(dtype=2)):
        assert backward(**bad) == -1, bad
    assert backward(K=65, ldg=65) == -2 and backward(C=1 << 20) == -2
    assert backward(ws=Z) == -3 and backward(nbytes=8) == -3
    assert backward(dtype=9, K=65, ldg=65, ws=Z) == -1 and backward(shift=Z, nbytes=8) == -1 and backward(K=65, ldg=65, ws=Z) == -2
