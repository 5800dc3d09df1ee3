"""CPU tests of the nested classifiers of sqfa_amd.classify (nested_predict, nested_log_evidence, nested_accuracy,
nested_label_log_proba, nested_log_loss): the torch expression in float64 against the long double oracle of every prefix
(tests/nested_oracle.py), column K - 1 against the full classifier, column k - 1 against a classifier built on the leading
k features, ties, the flag rule, the refusals, and FeatureClassifier on both models."""
import numpy as np
import pytest
import torch

import classify_hard as ch
import nested_oracle
from sqfa_amd import classify, model

LD = np.longdouble
NESTED = ("nested_predict", "nested_log_evidence", "nested_accuracy", "nested_label_log_proba", "nested_log_loss")


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


def _classifier(ref, weights=None, zero_means=False):
    clf = classify.GaussianClassifier(None if zero_means else _t(ref["mu"]), _t(ref["cov"]),
                                      None if weights is None else list(weights))
    return clf, _t(ref["Z"]), torch.tensor(ref["labels"])


def _ld(t):
    return t.double().numpy().astype(LD)


def test_names():
    assert classify.NATIVE_NESTED is True
    for name in NESTED:
        assert callable(getattr(classify.GaussianClassifier, name)) and callable(getattr(classify.FeatureClassifier, name))


@pytest.mark.parametrize("zero_means", [False, True], ids=["means", "zero-means"])
@pytest.mark.parametrize("level,C,K", [("base", 9, 5), ("c1e3", 3, 17), ("farmean", 9, 16), ("farsample", 3, 33)])
def test_torch_expression_against_the_oracle(level, C, K, zero_means):
    want = nested_oracle.prefixes(level, C, K, zero_means=zero_means)
    clf, Z, y = _classifier(want["ref"], zero_means=zero_means)
    N = Z.shape[0]
    A, E, ll = clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_label_log_proba(Z, y)
    assert A.shape == E.shape == ll.shape == (N, K) and A.dtype == torch.int64 and E.dtype == ll.dtype == torch.float64
    tol_S, tol_E = want["tol64_S"], want["tol64_E"]   # max(1e-10, 5 x the float64 yardstick of the case)
    assert (np.abs(_ld(E) - want["E"]) <= tol_E * (1 + np.abs(want["E"]))).all()
    bound_ll = tol_S * (1 + np.abs(want["Sy"])) + tol_E * (1 + np.abs(want["E"]))
    assert (np.abs(_ld(ll) - want["ll"]) <= bound_ll).all() and (ll <= 0).all()
    sure = want["decided64"]
    assert (~sure).mean(0).max() <= ch.EXCLUSION_CAP
    assert np.array_equal(A.numpy()[sure], want["pred"][sure])
    acc, loss = clf.nested_accuracy(Z, y), clf.nested_log_loss(Z, y)
    assert acc.shape == loss.shape == (K,) and acc.dtype == loss.dtype == torch.float64 and not acc.is_cuda
    assert torch.equal(acc, (A == y[:, None]).double().sum(0) / N)
    assert torch.allclose(loss, -ll.sum(0) / N, rtol=1e-14, atol=0)


def test_last_column_is_the_full_classifier_and_every_column_a_sliced_one():
    ref = ch.reference("c1e3", 9, 17)
    weights = tuple(1.0 + c % 3 for c in range(9))
    clf, Z, y = _classifier(ref, weights)
    A, E, ll, loss = clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_label_log_proba(Z, y), clf.nested_log_loss(Z, y)
    for k in (1, 4, 16, 17):
        part = clf if k == 17 else classify.GaussianClassifier(_t(ref["mu"][:, :k]), _t(ref["cov"][:, :k, :k]), list(weights))
        Zk = Z[:, :k]
        assert torch.equal(A[:, k - 1], part.predict(Zk))
        assert torch.allclose(E[:, k - 1], part.log_evidence(Zk), rtol=1e-12, atol=1e-12)
        assert torch.allclose(ll[:, k - 1], part.label_log_proba(Zk, y), rtol=1e-12, atol=1e-12)
        assert abs(loss[k - 1].item() - part.log_loss(Zk, y)) <= 1e-12 * (1 + abs(loss[k - 1].item()))


def test_chunked_expression_equals_the_unchunked(monkeypatch):
    clf, Z, y = _classifier(ch.reference("base", 9, 5))
    whole = clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_label_log_proba(Z, y)
    monkeypatch.setattr(classify, "FALLBACK_BYTES", 1)   # one class per chunk
    parts = clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_label_log_proba(Z, y)
    assert torch.equal(whole[0], parts[0])
    assert torch.allclose(whole[1], parts[1], rtol=1e-13, atol=0) and torch.allclose(whole[2], parts[2], rtol=0, atol=1e-12)


def test_results_carry_no_graph():
    ref = ch.reference("base", 3, 4)
    clf, Z, y = _classifier(ref)
    Z.requires_grad_(True)
    for out in (clf.nested_predict(Z), clf.nested_log_evidence(Z), clf.nested_label_log_proba(Z, y)):
        assert not out.requires_grad


@pytest.mark.parametrize("step", [1 << 28, 1], ids=["one-chunk", "class-per-chunk"])
def test_ties_never_yield_the_higher_index(monkeypatch, step):
    monkeypatch.setattr(classify, "FALLBACK_BYTES", step)
    ref = ch.reference("base", 9, 17)
    twin = [0, 1, 2, 3, 1, 5, 2, 7, 1]   # classes 4 and 8 are class 1, class 6 is class 2
    clf = classify.GaussianClassifier(_t(ref["mu"][twin]), _t(ref["cov"][twin]))
    A = clf.nested_predict(_t(ref["Z"])).numpy()
    assert not np.isin(A, (4, 6, 8)).any()
    assert (A == 1).any(0).all() and (A == 2).any()


def test_a_nan_in_one_feature_refuses_the_sample():
    ref = ch.reference("base", 3, 5)
    clf, Z, y = _classifier(ref)
    Z[7, 3] = float("nan")
    A, E, ll, counts = clf._nested(Z, argmax=True, logsumexp=True, labels=y)
    assert counts.tolist() == [1, 0, 0]
    rows = torch.arange(Z.shape[0]) == 7
    assert torch.equal(A == -1, rows[:, None].expand_as(A)) and torch.equal(torch.isnan(E), rows[:, None].expand_as(E))
    assert torch.equal(torch.isnan(ll), rows[:, None].expand_as(ll))
    for call in (lambda: clf.nested_predict(Z), lambda: clf.nested_log_evidence(Z), lambda: clf.nested_accuracy(Z, y),
                 lambda: clf.nested_label_log_proba(Z, y), lambda: clf.nested_log_loss(Z, y)):
        with pytest.raises(ValueError, match="1 samples have non-finite scores"):
            call()


def test_label_refusals():
    ref = ch.reference("base", 3, 5)
    clf, Z, y = _classifier(ref, (0.0, 1.0, 2.0))
    N = Z.shape[0]
    with pytest.raises(ValueError, match="50 labels belong to a class with prior 0"):
        clf.nested_log_loss(Z, y)
    ok = torch.where(y == 0, 1, y)
    assert torch.isfinite(clf.nested_log_loss(Z, ok)).all()
    outside = ok.clone()
    outside[3], outside[9] = -1, 3
    for method in (clf.nested_log_loss, clf.nested_label_log_proba):
        with pytest.raises(ValueError, match=r"2 labels are outside \[0, 3\)"):
            method(Z, outside)
    for method in (clf.nested_log_loss, clf.nested_label_log_proba, clf.nested_accuracy):
        with pytest.raises(ValueError, match=rf"labels must be integers of shape \({N},\)"):
            method(Z, ok[:-1])
        with pytest.raises(ValueError, match="labels must be integers"):
            method(Z, ok.double())
    with pytest.raises(ValueError):
        clf.nested_predict(Z[:, :4])


def test_one_class():
    ref = ch.reference("base", 3, 4)
    clf = classify.GaussianClassifier(_t(ref["mu"][:1]), _t(ref["cov"][:1]))
    Z = _t(ref["Z"])
    y = torch.zeros(Z.shape[0], dtype=torch.int64)
    assert (clf.nested_predict(Z) == 0).all() and (clf.nested_label_log_proba(Z, y) == 0).all()
    assert torch.equal(clf.nested_accuracy(Z, y), torch.ones(4, dtype=torch.float64))


def _points(C=3, D=8, per=60, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = 1.5 * torch.randn(C, D, generator=g)
    mix = torch.randn(C, D, D, generator=g) / D ** 0.5
    y = torch.arange(C).repeat_interleave(per)
    X = centres[y] + torch.einsum("nij,nj->ni", mix[y], torch.randn(C * per, D, generator=g))
    return X, y


@pytest.mark.parametrize("kind", ["SQFA", "SecondMomentsSQFA"])
def test_feature_classifier(kind):
    X, y = _points()
    filters = torch.randn(4, 8, generator=torch.Generator().manual_seed(1))
    m = getattr(model, kind)(n_dim=8, n_filters=4, feature_noise=0.01, filters=filters)
    fc = classify.FeatureClassifier.from_model(m, X=X, y=y)
    assert (fc.classifier.means is None) == (kind == "SecondMomentsSQFA")
    A, E, ll = fc.nested_predict(X), fc.nested_log_evidence(X), fc.nested_label_log_proba(X, y)
    assert A.shape == E.shape == ll.shape == (180, 4)
    assert torch.equal(A, fc.classifier.nested_predict(fc.transform(X)))
    acc, loss = fc.nested_accuracy(X, y), fc.nested_log_loss(X, y)
    # the model is float32: column K - 1 against the full classifier to 1e-4 (test_classify.py derives 6e-5 for such features)
    assert torch.allclose(E[:, -1], fc.log_evidence(X), rtol=1e-4, atol=1e-4)
    assert abs(loss[-1].item() - fc.log_loss(X, y)) <= 1e-4 * (1 + abs(loss[-1].item()))
    assert torch.equal(acc, (A == y[:, None]).double().mean(0))
    # the first k filters alone: a model of k filters sees the same class Gaussians
    for k in (1, 3):
        mk = getattr(model, kind)(n_dim=8, n_filters=k, feature_noise=0.01, filters=filters[:k].clone())
        part = classify.FeatureClassifier.from_model(mk, X=X, y=y)
        assert torch.allclose(E[:, k - 1], part.log_evidence(X), rtol=1e-4, atol=1e-4)
        assert abs(loss[k - 1].item() - part.log_loss(X, y)) <= 1e-4 * (1 + abs(loss[k - 1].item()))
