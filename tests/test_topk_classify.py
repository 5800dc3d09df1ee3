"""CPU tests of predict_topk / label_rank / topk_accuracy (sqfa_amd.classify): the torch expression (a stable descending sort
and the tie-rule count over ``_torch_scores``, chunked over the samples) against the float64 numpy oracle
tests/classify_oracle.py and the interval helper tests/topk_oracle.py, the tie rule on duplicated classes, and every refusal.
The native kernels are tested in tests/test_gpu_topk_classify.py."""
import math

import numpy as np
import pytest
import torch

import classify_oracle
import topk_oracle
from sqfa_amd import classify

SHAPES = [(3, 3, 17), (17, 4, 257), (37, 17, 300)]   # (C, K, N)


def _problem(C, K, N, means=True, priors=False, seed=None):
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, 0.5, seed=C + 7 * K if seed is None else seed)
    w = None
    if priors:
        w = 1.0 + np.arange(C) % 5
        w[[1, C - 1]] = 0.0
    mu = mu if means else None
    S = classify_oracle.scores(Z, mu, cov, w)
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
    return classify.GaussianClassifier(t(mu), t(cov), w), t(Z), labels, S


def _ks(C):
    return sorted({k for k in (1, 2, 3, 5, 8, 11, C) if k <= C})


@pytest.mark.parametrize("priors", [False, True], ids=["uniform", "priors"])
@pytest.mark.parametrize("means", [True, False], ids=["means", "zeromean"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-K%d-N%d" % s)
def test_torch_path_against_the_oracle(shape, means, priors):
    C, K, N = shape
    clf, Z, labels, S = _problem(C, K, N, means, priors)
    assert clf._factors is None
    e = topk_oracle.bounds64(S)
    y = torch.tensor(labels)
    rank = clf.label_rank(Z, y)
    assert rank.dtype == torch.int64 and rank.shape == (N,) and not rank.requires_grad
    undecided = topk_oracle.check_rank(rank.numpy(), S, e, labels)
    assert undecided <= 0.01
    pred = clf.predict(Z)
    assert torch.equal(rank == 0, pred == y)
    for k in _ks(C):
        index, score = clf.predict_topk(Z, k, return_scores=True)
        assert index.dtype == torch.int64 and score.dtype == torch.float64 and index.shape == score.shape == (N, k)
        assert torch.equal(index, clf.predict_topk(Z, k))
        assert torch.equal(index[:, 0], pred)
        assert topk_oracle.check_topk(index.numpy(), score.numpy(), S, e, k) <= 0.01
    if priors:   # k reaches into the classes of prior 0: -inf entries, in the order of their indices, after the finite ones
        index, score = clf.predict_topk(Z, C, return_scores=True)
        assert torch.isneginf(score[:, -2:]).all() and (index[:, -2:] == torch.tensor([1, C - 1])).all()
        on_zero = torch.full((N,), C - 1)
        assert torch.equal(clf.label_rank(Z, on_zero), torch.full((N,), C - 1))   # a label of prior 0 is ranked, not refused
    want = [int((rank.numpy() < k).sum()) / N for k in (1, 5)]
    got = clf.topk_accuracy(Z, y)
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.tolist() == want
    assert want[0] == clf.accuracy(Z, y)


def test_chunks_over_the_samples_give_the_same(monkeypatch):
    clf, Z, labels, _ = _problem(17, 4, 257)
    y = torch.tensor(labels)
    whole = clf.predict_topk(Z, 5, return_scores=True), clf.label_rank(Z, y)
    monkeypatch.setattr(classify, "FALLBACK_BYTES", 17 * (3 * 4 * 8 + 3 * 8 + 16) * 10)   # ten samples per chunk
    assert len(clf._sample_chunks(257, 17 * (3 * 4 * 8 + 3 * 8 + 16))) == 26
    index, score = clf.predict_topk(Z, 5, return_scores=True)
    # the matrix products of other shapes round differently: the scores agree to rounding, the order at these gaps exactly
    assert torch.equal(index, whole[0][0]) and torch.allclose(score, whole[0][1], rtol=1e-13, atol=0)
    assert torch.equal(clf.label_rank(Z, y), whole[1])


def test_ties_go_to_the_lowest_index():
    Z, _, mu, cov = classify_oracle.problem(5, 4, 200, 1.0, seed=3)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    pick = list(range(5)) * 2   # class c again at c + 5: equal scores, bit for bit
    clf = classify.GaussianClassifier(t(mu[pick]), t(cov[pick]))
    S = clf.scores(t(Z))
    assert torch.equal(S[:, :5], S[:, 5:])
    index, score = clf.predict_topk(t(Z), 10, return_scores=True)
    assert torch.equal(index[:, 0::2] + 5, index[:, 1::2])   # every class directly before its copy
    assert torch.equal(score[:, 0::2], score[:, 1::2])
    assert torch.equal(index, torch.tensor(topk_oracle.stable_order(S.numpy())))
    base = classify.GaussianClassifier(t(mu), t(cov))
    y = torch.arange(200) % 5
    r = base.label_rank(t(Z), y)
    assert torch.equal(clf.label_rank(t(Z), y), 2 * r)          # before the label: the classes before it and their copies
    assert torch.equal(clf.label_rank(t(Z), y + 5), 2 * r + 1)  # ... and the label's own first copy
    assert np.array_equal(clf.label_rank(t(Z), y + 5).numpy(), topk_oracle.rank(S.numpy(), (y + 5).numpy()))


def test_topk_accuracy_forms():
    clf, Z, labels, S = _problem(17, 4, 257)
    y = torch.tensor(labels)
    rank = topk_oracle.rank(clf.scores(Z).numpy(), labels)
    one = clf.topk_accuracy(Z, y, k=3)
    assert isinstance(one, float) and one == int((rank < 3).sum()) / 257
    many = clf.topk_accuracy(Z, y, k=(1, 2, 17, 40))
    assert many.shape == (4,) and many.tolist() == [int((rank < k).sum()) / 257 for k in (1, 2)] + [1.0, 1.0]
    assert clf.topk_accuracy(Z, y, k=[5]).shape == (1,)
    assert clf.topk_accuracy(Z, y, k=1000) == 1.0
    assert clf.topk_accuracy(Z, labels.tolist(), k=1) == clf.accuracy(Z, y)


def test_feature_classifier_forwards():
    clf, Z, labels, _ = _problem(5, 4, 100)
    filters = torch.randn(4, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    X = Z @ torch.linalg.pinv(filters).T
    fc = classify.FeatureClassifier(filters, clf)
    Zf, y = fc.transform(X), torch.tensor(labels)
    index, score = fc.predict_topk(X, 3, return_scores=True)
    want = clf.predict_topk(Zf, 3, return_scores=True)
    assert torch.equal(index, want[0]) and torch.equal(score, want[1])
    assert torch.equal(fc.predict_topk(X, 2), clf.predict_topk(Zf, 2))
    assert torch.equal(fc.label_rank(X, y), clf.label_rank(Zf, y))
    assert torch.equal(fc.topk_accuracy(X, y), clf.topk_accuracy(Zf, y))
    assert fc.topk_accuracy(X, y, k=2) == clf.topk_accuracy(Zf, y, k=2)


def test_refusals():
    clf, Z, labels, _ = _problem(17, 4, 257)
    y = torch.tensor(labels)
    for k in (0, -1, 18, 2.0, "3", None, True, (1, 2)):
        with pytest.raises(ValueError, match="k must be an int in \\[1, 17\\]"):
            clf.predict_topk(Z, k)
    for k in (0, -3, 1.5, True, (1, 0), (), (2, 2.0), "5"):
        with pytest.raises(ValueError, match="k must be an int >= 1"):
            clf.topk_accuracy(Z, y, k=k)
    with pytest.raises(ValueError, match="samples must have shape"):
        clf.predict_topk(Z[:, :3], 2)
    with pytest.raises(ValueError, match="samples must have shape"):
        clf.label_rank(Z[:0], y[:0])
    for method in (clf.label_rank, clf.topk_accuracy):
        with pytest.raises(ValueError, match="labels must be integers of shape \\(257,\\)"):
            method(Z, y[:-1])
        with pytest.raises(ValueError, match="labels must be integers"):
            method(Z, y.double())
        with pytest.raises(ValueError, match="labels must be integers"):
            method(Z, y[:, None])
        bad = y.clone()
        bad[[0, 5, 256]] = torch.tensor([-1, 17, 2 ** 40])
        with pytest.raises(ValueError, match="3 labels are outside \\[0, 17\\)"):
            method(Z, bad)
        Zn = Z.clone()
        Zn[[3, 200], [0, 2]] = torch.tensor([math.nan, math.inf], dtype=torch.float64)
        with pytest.raises(ValueError, match="2 samples have non-finite scores"):
            method(Zn, y)
    with pytest.raises(ValueError, match="2 samples have non-finite scores"):
        clf.predict_topk(Zn, 3)
    # the counts come from the whole batch, whichever chunk holds them, and the rows are marked
    index, score, count = clf._torch_topk(Zn, 3, True)
    assert count.tolist() == [2] and (index[[3, 200]] == -1).all() and torch.isnan(score[[3, 200]]).all()
    assert (index[[2, 4, 199, 201]] >= 0).all()
    rank, flags = clf._torch_rank(Zn, bad)
    assert flags.tolist() == [2, 3] and (rank[[0, 3, 5, 200, 256]] == -1).all() and (rank[[1, 2, 4, 6]] >= 0).all()

