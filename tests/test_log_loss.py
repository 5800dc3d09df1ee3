"""CPU tests of the Gaussian log-loss in sqfa_amd.classify (the torch expression: no GPU here): values and gradients against
the float64 oracle tests/log_loss_oracle.py, the exact zeros of one class, every refusal, label_log_proba against
predict_log_proba, feature_log_loss against a plain torch chain written here, and fit_log_loss on a toy problem."""
import math

import numpy as np
import pytest
import torch

import log_loss_oracle
from sqfa_amd import classify

# (C, K, N, sep, means, priors)
CASES = [(3, 3, 17, 1.0, True, False), (3, 3, 17, 0.0, True, False), (37, 16, 200, 1.0, True, False),
         (9, 33, 120, 1.0, False, False), (9, 5, 150, 1.0, True, True), (6, 4, 90, 0.0, False, True)]


def _inputs(case, requires_grad=True):
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=requires_grad)
    return t(case["Z"]), torch.tensor(case["labels"]), t(case["mu"]), t(case["cov"]), case["w"]


def _rel(got, want):
    return np.abs(got.detach().numpy() - want).max() / max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "C{}-K{}-N{}-sep{:g}-{}-{}".format(*s))
def test_torch_path_matches_the_oracle(shape):
    C, K, N, sep, means, priors = shape
    case = log_loss_oracle.case(C, K, N, sep, means, priors, upstream=0.7)
    ref = case["ref"]
    Z, y, mu, cov, w = _inputs(case)
    loss = classify.gaussian_log_loss(Z, y, mu, cov, w)
    assert loss.dim() == 0 and loss.dtype == torch.float64
    assert abs(loss.item() - ref["loss"]) <= 1e-10 * (1 + abs(ref["loss"]))
    (0.7 * loss).backward()
    assert _rel(Z.grad, ref["gZ"]) <= 1e-10
    assert _rel(cov.grad, ref["gcov"]) <= 1e-10
    if means:
        assert _rel(mu.grad, ref["gmu"]) <= 1e-10
    clf = classify.GaussianClassifier(mu.detach() if means else None, cov.detach(), w)
    ll = clf.label_log_proba(Z.detach(), y)
    assert ll.shape == (N,) and not ll.requires_grad and (ll <= 0).all()
    assert np.abs(ll.numpy() - ref["ll"]).max() <= 1e-10 * (1 + np.abs(ref["ll"]).max())
    value = clf.log_loss(Z.detach(), y)
    assert isinstance(value, float) and abs(value - ref["loss"]) <= 1e-10 * (1 + abs(ref["loss"]))


def test_label_log_proba_is_the_labelled_entry_of_predict_log_proba():
    case = log_loss_oracle.case(9, 5, 150, 1.0, True, True)
    Z, y, mu, cov, w = _inputs(case, requires_grad=False)
    clf = classify.GaussianClassifier(mu, cov, w)
    assert torch.equal(clf.label_log_proba(Z, y), clf.predict_log_proba(Z).gather(1, y[:, None])[:, 0])
    assert torch.equal(clf.label_log_proba(Z, y.to(torch.int32)), clf.label_log_proba(Z, y))   # any integer dtype


@pytest.mark.parametrize("means", [True, False])
def test_one_class_gives_exact_zeros(means):
    case = log_loss_oracle.case(1, 4, 30, 1.0, means)
    Z, y, mu, cov, _ = _inputs(case)
    loss = classify.gaussian_log_loss(Z, y, mu, cov)
    loss.backward()
    assert loss.item() == 0.0
    for g in (Z.grad, cov.grad) + ((mu.grad,) if means else ()):
        assert torch.count_nonzero(g) == 0


def test_refusals():
    case = log_loss_oracle.case(9, 5, 150, 1.0, True, True)
    Z, y, mu, cov, w = _inputs(case, requires_grad=False)
    clf = classify.GaussianClassifier(mu, cov, w)
    calls = [lambda Z, y: classify.gaussian_log_loss(Z, y, mu, cov, w), clf.label_log_proba, clf.log_loss]
    for call in calls:
        with pytest.raises(ValueError, match=r"labels must be integers of shape \(150,\)"):
            call(Z, y[:-1])
        with pytest.raises(ValueError, match="labels must be integers"):
            call(Z, y.double())
        with pytest.raises(ValueError, match="labels must be integers"):
            call(Z, y[:, None])
        bad = y.clone()
        bad[[0, 7, 149]] = torch.tensor([-1, 9, 2 ** 40])
        with pytest.raises(ValueError, match=r"3 labels are outside \[0, 9\)"):
            call(Z, bad)
        bad = y.clone()
        bad[[3, 4]] = torch.tensor([2, 8])   # the classes of prior 0
        with pytest.raises(ValueError, match="2 labels belong to a class with prior 0"):
            call(Z, bad)
        Zn = Z.clone()
        Zn[[1, 64, 100], [0, 2, 4]] = math.nan
        with pytest.raises(ValueError, match="3 samples have non-finite scores"):
            call(Zn, y)
    broken = cov.clone()
    broken[1] = -broken[1]
    broken[6, 2, 2] = math.nan
    with pytest.raises(ValueError, match="2 of 9 classes"):
        classify.gaussian_log_loss(Z, y, mu, broken, w)
    with pytest.raises(ValueError, match="means must have shape"):
        classify.gaussian_log_loss(Z, y, mu[:-1], cov, None)
    with pytest.raises(ValueError, match="samples must have shape"):
        classify.gaussian_log_loss(Z[:, :-1], y, mu, cov, None)
    with pytest.raises(ValueError, match="covariances must be"):
        classify.gaussian_log_loss(Z, y, mu, cov[0], None)


# ---- feature_log_loss: (D, K, C, N) = (8, 3, 3, 50) against a plain float64 torch chain -------------------------------------

def _toy(D=8, C=3, N=50, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = 0.8 * torch.randn(C, D, generator=g, dtype=torch.float64)
    mix = torch.randn(C, D, D, generator=g, dtype=torch.float64) / D ** 0.5
    y = torch.arange(N) % C
    X = centres[y] + torch.einsum("nij,nj->ni", mix[y], torch.randn(N, D, generator=g, dtype=torch.float64))
    return X, y


def _plain_log_loss(Z, y, mu, cov, log_priors):
    """The definition, one class at a time with inv and slogdet."""
    K = Z.shape[1]
    cols = []
    for c in range(cov.shape[0]):
        d = Z if mu is None else Z - mu[c]
        quad = torch.einsum("nk,kl,nl->n", d, torch.linalg.inv(cov[c]), d)
        cols.append(-0.5 * quad - 0.5 * torch.linalg.slogdet(cov[c])[1] - 0.5 * K * math.log(2 * math.pi) + log_priors[c])
    S = torch.stack(cols, 1)
    return -(S.gather(1, y[:, None])[:, 0] - torch.logsumexp(S, 1)).mean()


@pytest.mark.parametrize("constraint", ["sphere", "none", "orthogonal"])
@pytest.mark.parametrize("second_moments", [False, True], ids=["SQFA", "SecondMomentsSQFA"])
def test_feature_log_loss_gradient_against_a_plain_chain(second_moments, constraint):
    import sqfa_amd
    from sqfa_amd.statistics import ClassPoints, class_statistics
    X, y = _toy()
    torch.manual_seed(3)
    cls = sqfa_amd.model.SecondMomentsSQFA if second_moments else sqfa_amd.model.SQFA
    model = cls(n_dim=8, n_filters=3, feature_noise=0.05, constraint=constraint).double()
    raw = list(model.parameters())
    assert len(raw) == 1
    stats = class_statistics(X, y)
    counts = torch.bincount(y).double()

    def chain(log_priors):
        F = model.filters
        Z = X @ F.T
        noise = model.noise_mat
        if second_moments:
            S = stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
            return _plain_log_loss(Z, y, None, F @ S @ F.T + noise, log_priors)
        return _plain_log_loss(Z, y, stats["means"] @ F.T, F @ stats["covariances"] @ F.T + noise, log_priors)

    uniform = torch.full((3,), -math.log(3), dtype=torch.float64)
    want = chain(uniform)
    g_want, = torch.autograd.grad(want, raw)
    for given in (dict(), dict(data_statistics=stats), dict(data_statistics=ClassPoints(X, y))):
        loss = classify.feature_log_loss(model, X, y, **given)
        assert loss.dim() == 0 and abs(loss.item() - want.item()) <= 1e-10 * (1 + abs(want.item()))
        g, = torch.autograd.grad(loss, raw)
        assert (g - g_want).abs().max() <= 1e-9 * g_want.abs().max()
    # empirical priors: the class counts of y
    want = chain(torch.log(counts / counts.sum()))
    loss = classify.feature_log_loss(model, X, y, data_statistics=stats, priors="empirical")
    assert abs(loss.item() - want.item()) <= 1e-10 * (1 + abs(want.item()))
    # the loss of the current filters is what the frozen classifier reports
    fc = classify.FeatureClassifier.from_model(model, y=y, data_statistics=stats, priors="empirical")
    assert abs(fc.log_loss(X, y) - want.item()) <= 1e-10 * (1 + abs(want.item()))
    assert torch.equal(fc.label_log_proba(X, y), fc.classifier.label_log_proba(fc.transform(X), y))


def test_fit_log_loss_lowers_the_loss_and_returns_its_history():
    import sqfa_amd
    X, y = _toy(N=150, seed=1)
    torch.manual_seed(0)
    model = sqfa_amd.model.SQFA(n_dim=8, n_filters=2, feature_noise=0.05).double()
    before = classify.feature_log_loss(model, X, y).item()
    losses, times = classify.fit_log_loss(model, X, y, max_epochs=6)
    after = classify.feature_log_loss(model, X, y).item()
    assert losses.shape == times.shape and 1 <= len(losses) <= 6
    assert (times[1:] >= times[:-1]).all()
    # L-BFGS reports the loss at the start of each step: the history begins at the initial loss and falls
    assert abs(losses[0].item() - before) <= 1e-6 * (1 + abs(before))   # the history is a float32 tensor
    assert after < before and (len(losses) == 1 or losses[-1].item() < before)
