"""CPU tests of sqfa_amd.classify: names, the torch expression against the float64 numpy oracle, priors, ties, the refusals,
FeatureClassifier.from_model for both model classes and both kinds of statistics, and gradients through the expression."""
import math

import numpy as np
import pytest
import torch

import classify_oracle
import sqfa_amd
from sqfa_amd import classify, model
from sqfa_amd.statistics import ClassPoints, class_statistics


def _t(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def test_names():
    assert classify.__all__ == ["gaussian_class_scores", "GaussianClassifier", "FeatureClassifier"]
    assert "classify" in sqfa_amd.__all__ and sqfa_amd.classify is classify
    assert classify.NATIVE_CLASS_SCORES is True
    for name in ("scores", "predict", "log_evidence", "predict_log_proba", "predict_proba", "accuracy"):
        assert callable(getattr(classify.GaussianClassifier, name))
        assert callable(getattr(classify.FeatureClassifier, name))
    # the model classes do not grow
    assert not hasattr(model.SQFA, "predict") and "classify" not in dir(model)


@pytest.mark.parametrize("C,K,N,sep", [(1, 1, 1, 1.0), (3, 3, 17, 1.0), (17, 4, 257, 0.0), (37, 17, 300, 1.0), (5, 64, 50, 1.0),
                                       (4, 65, 30, 1.0)])
def test_torch_expression_against_the_oracle(C, K, N, sep):
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, sep, seed=3)
    S_ref = classify_oracle.scores(Z, mu, cov)
    clf = classify.GaussianClassifier(_t(mu), _t(cov))
    assert (clf.n_classes, clf.n_features) == (C, K)
    assert clf.log_priors.dtype == torch.float64 and torch.allclose(clf.log_priors, torch.full((C,), -math.log(C), dtype=torch.float64))
    S = clf.scores(_t(Z))
    assert S.shape == (N, C) and S.dtype == torch.float64
    assert (np.abs(S.numpy() - S_ref) / (1 + np.abs(S_ref))).max() <= 1e-10
    assert torch.equal(classify.gaussian_class_scores(_t(Z), _t(mu), _t(cov)), S)
    E_ref = classify_oracle.log_evidence(S_ref)
    E = clf.log_evidence(_t(Z)).numpy()
    assert (np.abs(E - E_ref) / (1 + np.abs(E_ref))).max() <= 1e-10
    pred = clf.predict(_t(Z))
    assert pred.dtype == torch.int64
    sure = classify_oracle.top_two_gap(S_ref) > 1e-9
    assert np.array_equal(pred.numpy()[sure], classify_oracle.predict(S_ref)[sure])
    logp = clf.predict_log_proba(_t(Z))
    assert torch.logsumexp(logp, 1).abs().max() <= 1e-10
    assert torch.allclose(clf.predict_proba(_t(Z)).sum(1), torch.ones(N, dtype=torch.float64), atol=1e-10)
    acc = clf.accuracy(_t(Z), torch.tensor(labels))
    assert isinstance(acc, float) and acc == float((pred.numpy() == labels).mean())


def test_chunked_expression_equals_the_unchunked(monkeypatch):
    Z, _, mu, cov = classify_oracle.problem(11, 5, 40, 1.0, seed=5)
    whole = classify.GaussianClassifier(_t(mu), _t(cov)).scores(_t(Z))
    monkeypatch.setattr(classify, "FALLBACK_BYTES", 3 * 40 * 5 * 8 * 3)   # three classes at a time
    assert torch.allclose(classify.GaussianClassifier(_t(mu), _t(cov)).scores(_t(Z)), whole, rtol=0, atol=1e-12)


def test_zero_means():
    Z, _, _, cov = classify_oracle.problem(4, 6, 30, 0.0, seed=7)
    S_ref = classify_oracle.scores(Z, None, cov)
    S = classify.GaussianClassifier(None, _t(cov)).scores(_t(Z)).numpy()
    assert (np.abs(S - S_ref) / (1 + np.abs(S_ref))).max() <= 1e-10


def test_priors():
    Z, _, mu, cov = classify_oracle.problem(4, 3, 60, 0.5, seed=2)
    w = np.array([3.0, 0.0, 1.0, 4.0])
    S_ref = classify_oracle.scores(Z, mu, cov, w)
    for priors in (w, list(w), _t(w), _t(w, torch.float32), 10 * w):
        clf = classify.GaussianClassifier(_t(mu), _t(cov), priors)
        assert torch.allclose(clf.log_priors.exp(), _t(w / w.sum()), atol=1e-15)
        S = clf.scores(_t(Z)).numpy()
        assert np.all(np.isneginf(S[:, 1])) and np.all(np.isneginf(S_ref[:, 1]))
        keep = [0, 2, 3]
        assert (np.abs(S[:, keep] - S_ref[:, keep]) / (1 + np.abs(S_ref[:, keep]))).max() <= 1e-10
        assert not (clf.predict(_t(Z)) == 1).any()                        # a class with zero prior never wins
        E_ref = classify_oracle.log_evidence(S_ref)
        assert np.abs(clf.log_evidence(_t(Z)).numpy() - E_ref).max() <= 1e-10 * (1 + np.abs(E_ref).max())   # and adds nothing
    uniform = classify.GaussianClassifier(_t(mu), _t(cov)).scores(_t(Z))
    assert torch.equal(classify.GaussianClassifier(_t(mu), _t(cov), "uniform").scores(_t(Z)), uniform)
    assert torch.equal(classify.GaussianClassifier(_t(mu), _t(cov), np.ones(4)).scores(_t(Z)), uniform)


@pytest.mark.parametrize("priors", ["empirical", "flat", [1.0, 2.0], [1.0, -1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0],
                                    [1.0, float("nan"), 1.0, 1.0], [1.0, float("inf"), 1.0, 1.0], np.ones((4, 1))])
def test_bad_priors(priors):
    _, _, mu, cov = classify_oracle.problem(4, 3, 5, 0.5)
    with pytest.raises(ValueError):
        classify.GaussianClassifier(_t(mu), _t(cov), priors)


def test_ties_go_to_the_lowest_index():
    Z, _, mu, cov = classify_oracle.problem(3, 4, 40, 1.0, seed=4)
    mu5, cov5 = mu[[0, 1, 1, 2, 1]], cov[[0, 1, 1, 2, 1]]   # classes 1, 2 and 4 are the same Gaussian
    pred = classify.GaussianClassifier(_t(mu5), _t(cov5)).predict(_t(Z)).numpy()
    base = classify.GaussianClassifier(_t(mu), _t(cov)).predict(_t(Z)).numpy()
    assert (base == 1).any()
    assert np.array_equal(pred, np.array([0, 1, 3])[base])


def test_refusals():
    Z, _, mu, cov = classify_oracle.problem(5, 3, 20, 1.0)
    bad = cov.copy()
    bad[1] = -bad[1]
    bad[3, 0, 0] = np.nan
    with pytest.raises(ValueError, match="2 of 5 classes"):
        classify.GaussianClassifier(_t(mu), _t(bad))
    bad_mu = mu.copy()
    bad_mu[4, 1] = np.inf
    with pytest.raises(ValueError, match="1 of 5 classes"):
        classify.GaussianClassifier(_t(bad_mu), _t(cov))
    with pytest.raises(ValueError):
        classify.GaussianClassifier(_t(mu[:4]), _t(cov))
    with pytest.raises(ValueError):
        classify.GaussianClassifier(_t(mu), _t(cov[0]))
    clf = classify.GaussianClassifier(_t(mu), _t(cov))
    Zn = Z.copy()
    Zn[3, 1] = np.nan
    Zn[7, 0] = np.nan
    for method in (clf.scores, clf.predict, clf.log_evidence, clf.predict_log_proba, clf.predict_proba):
        with pytest.raises(ValueError, match="2 samples"):
            method(_t(Zn))
    with pytest.raises(ValueError, match="2 samples"):
        clf.accuracy(_t(Zn), torch.zeros(20, dtype=torch.int64))
    with pytest.raises(ValueError):
        clf.scores(_t(Z[:, :2]))
    with pytest.raises(ValueError):
        clf.accuracy(_t(Z), torch.zeros(19, dtype=torch.int64))


def _points(C=3, D=8, per=60, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = 1.5 * torch.randn(C, D, generator=g)
    mix = torch.randn(C, D, D, generator=g) / math.sqrt(D)
    y = torch.arange(C).repeat_interleave(per)
    y[:10] = 0   # unequal counts
    X = centres[y] + torch.einsum("nij,nj->ni", mix[y], torch.randn(C * per, D, generator=g))
    return X, y


@pytest.mark.parametrize("kind", ["dict", "points", "xy"])
@pytest.mark.parametrize("regularized", [True, False])
def test_from_model_sqfa(kind, regularized):
    X, y = _points()
    m = model.SQFA(n_dim=8, n_filters=2, feature_noise=0.01, filters=torch.randn(2, 8, generator=torch.Generator().manual_seed(1)))
    stats = class_statistics(X, y)
    given = {"dict": dict(data_statistics=stats), "points": dict(data_statistics=ClassPoints(X, y)), "xy": dict(X=X, y=y)}[kind]
    fc = classify.FeatureClassifier.from_model(m, regularized=regularized, **given)
    F = m.filters.detach().double().numpy()
    assert torch.equal(fc.filters, m.filters.detach()) and fc.filters is not m.filters and not fc.filters.requires_grad
    assert (fc.n_classes, fc.n_features) == (3, 2)
    mu_f = stats["means"].double().numpy() @ F.T
    cov_f = F @ stats["covariances"].double().numpy() @ F.T + (0.01 * np.eye(2) if regularized else 0)
    S_ref = classify_oracle.scores(X.double().numpy() @ F.T, mu_f, cov_f)
    S = fc.scores(X)
    assert S.shape == (180, 3) and not S.requires_grad
    # the model, the statistics and the features are float32: the quadratic term carries eps32 = 6e-8 times the condition
    # number of a 2 x 2 feature covariance (variances of order 1 over eigenvalues of order 1e-2..1e-1: below 1e3), 6e-5
    assert (np.abs(S.double().numpy() - S_ref) / (1 + np.abs(S_ref))).max() <= 2e-4
    sure = classify_oracle.top_two_gap(S_ref) > 1e-3 * (1 + np.abs(S_ref).max())
    assert np.array_equal(fc.predict(X).numpy()[sure], classify_oracle.predict(S_ref)[sure])
    assert abs(fc.accuracy(X, y) - float((classify_oracle.predict(S_ref) == y.numpy()).mean())) <= (~sure).mean()
    assert torch.allclose(fc.log_evidence(X), torch.logsumexp(S, 1), atol=1e-5)
    assert torch.allclose(fc.predict_proba(X).sum(1), torch.ones(180), atol=1e-5)
    # the snapshot: a later change of the model does not move the classifier
    with torch.no_grad():
        m.filters = torch.randn(2, 8)
    assert torch.equal(fc.scores(X), S)


@pytest.mark.parametrize("kind", ["dict", "points", "tensor"])
def test_from_model_second_moments(kind):
    X, y = _points(seed=3)
    m = model.SecondMomentsSQFA(n_dim=8, n_filters=3, feature_noise=0.02,
                                filters=torch.randn(3, 8, generator=torch.Generator().manual_seed(2)))
    stats = class_statistics(X, y)
    given = {"dict": stats, "points": ClassPoints(X, y), "tensor": stats["second_moments"]}[kind]
    fc = classify.FeatureClassifier.from_model(m, data_statistics=given)
    F = m.filters.detach().double().numpy()
    second_f = F @ stats["second_moments"].double().numpy() @ F.T + 0.02 * np.eye(3)
    S_ref = classify_oracle.scores(X.double().numpy() @ F.T, None, second_f)
    assert (np.abs(fc.scores(X).double().numpy() - S_ref) / (1 + np.abs(S_ref))).max() <= 2e-4
    assert fc.classifier.means is None


def test_from_model_priors():
    X, y = _points()
    m = model.SQFA(n_dim=8, n_filters=2, feature_noise=0.01)
    counts = torch.bincount(y).double()
    want = torch.log(counts / counts.sum())
    for given in (dict(X=X, y=y), dict(data_statistics=ClassPoints(X, y)), dict(data_statistics=class_statistics(X, y), y=y)):
        fc = classify.FeatureClassifier.from_model(m, priors="empirical", **given)
        assert torch.allclose(fc.log_priors, want, atol=1e-15)
    uniform = classify.FeatureClassifier.from_model(m, X=X, y=y)
    assert torch.allclose(uniform.log_priors, torch.full((3,), -math.log(3.0), dtype=torch.float64))
    assert torch.allclose(classify.FeatureClassifier.from_model(m, X=X, y=y, priors=[1.0, 1.0, 2.0]).log_priors.exp(),
                          torch.tensor([0.25, 0.25, 0.5], dtype=torch.float64))
    with pytest.raises(ValueError, match="empirical"):
        classify.FeatureClassifier.from_model(m, data_statistics=class_statistics(X, y), priors="empirical")
    with pytest.raises(ValueError):
        classify.FeatureClassifier.from_model(m)
    with pytest.raises(ValueError):
        classify.FeatureClassifier.from_model(m, X=X, y=y, priors="flat")


def test_gradients_flow_through_the_expression():
    Z, _, mu, cov = classify_oracle.problem(3, 4, 12, 1.0, seed=6)
    Zt, mut, covt = _t(Z).requires_grad_(), _t(mu).requires_grad_(), _t(cov).requires_grad_()
    S = classify.gaussian_class_scores(Zt, mut, covt)
    assert S.requires_grad
    torch.logsumexp(S, 1).sum().backward()
    for g in (Zt.grad, mut.grad, covt.grad):
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    # d score[n, c] / d z_n = -Sigma_c^-1 (z_n - mu_c)
    Zt.grad = None
    classify.GaussianClassifier(_t(mu), _t(cov)).scores(Zt)[:, 1].sum().backward()
    want = -np.linalg.solve(cov[1], (Z - mu[1]).T).T
    assert np.abs(Zt.grad.numpy() - want).max() <= 1e-9 * (1 + np.abs(want).max())
    with torch.no_grad():
        assert not classify.gaussian_class_scores(Zt, mut, covt).requires_grad
    f = lambda z: classify.GaussianClassifier(_t(mu), _t(cov)).log_evidence(z)
    assert torch.autograd.gradcheck(f, (_t(Z[:3]).requires_grad_(),))
