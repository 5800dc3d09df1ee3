"""Oracle of the Gaussian log-loss (sqfa_amd.classify.gaussian_log_loss), independent of the package's expression:

    ll_n = score[n, y_n] - logsumexp_c score[n, c]  (evaluated with the log-sum-exp anchored at the labelled score),
    loss = -1/N sum_n ll_n

with the scores of tests/classify_oracle.py written in torch, one class at a time (Cholesky, a triangular solve, the log of
the diagonal), and torch autograd for the gradients of ``upstream * loss`` with respect to the samples, the class means and
the class covariances.  float64 is the oracle; the same function in float32 is the yardstick of the float32 tolerance."""
import functools
import math

import numpy as np
import torch

import classify_oracle


def evaluate(Z, labels, means, covariances, priors=None, upstream=1.0, dtype=torch.float64):
    """dict(loss (float), ll (N,), gZ (N,K), gmu (C,K) | None, gcov (C,K,K)) as float64 numpy arrays.  means None = zero
    means; priors None = uniform, else (C,) weights (normalised; a zero weight is a class that never wins)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    Zt, cov = t(Z), t(covariances)
    mu = t(means) if means is not None else None
    C, K = cov.shape[0], cov.shape[-1]
    lp = torch.tensor(classify_oracle.log_priors(priors, C), dtype=dtype)
    y = torch.tensor(np.asarray(labels), dtype=torch.int64)
    columns = []
    for c in range(C):
        L = torch.linalg.cholesky(cov[c])
        diff = Zt if mu is None else Zt - mu[c]
        w = torch.linalg.solve_triangular(L, diff.T, upper=False)
        columns.append(-0.5 * (w * w).sum(0) - torch.log(torch.diagonal(L)).sum() - 0.5 * K * math.log(2.0 * math.pi) + lp[c])
    S = torch.stack(columns, 1)
    s_label = S.gather(1, y[:, None])
    if C == 1:
        ll = s_label[:, 0] - torch.logsumexp(S, 1)
    else:
        # the log-sum-exp anchored at the labelled score: ll = -log(1 + sum_{c != y} exp(s_c - s_y)) = -softplus(x).  Where a
        # sample is classified with near certainty this keeps 1 - p_y, and with it the gradients, to relative accuracy;
        # s_y - logsumexp(s) would leave them to the rounding of p_y - 1.
        others = (S - s_label).masked_fill(torch.nn.functional.one_hot(y, C).bool(), -math.inf)
        x = torch.logsumexp(others, 1)
        ll = -(x.clamp(min=0) + torch.log1p(torch.exp(-x.abs())))
    loss = -ll.mean()
    (upstream * loss).backward()
    n = lambda a: a.detach().double().numpy()
    return dict(loss=float(loss.detach().double()), ll=n(ll), gZ=n(Zt.grad), gmu=None if mu is None else n(mu.grad),
                gcov=n(cov.grad))


@functools.lru_cache(maxsize=None)
def case(C, K, N, sep, means=True, priors=False, np_dtype=np.float64, upstream=1.0):
    """A problem of classify_oracle.problem rounded to ``np_dtype`` (what every implementation is given) and the float64
    oracle on exactly those numbers.  ``priors``: non-uniform weights that include zeros (classes 2 and C - 1); the labels
    of those classes move to class 0, since a label on a class of prior 0 is refused."""
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, sep, seed=C + 7 * K)
    Z, mu, cov = Z.astype(np_dtype), mu.astype(np_dtype), cov.astype(np_dtype)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    w = None
    if priors:
        w = 1.0 + np.arange(C) % 5
        w[[2, C - 1]] = 0.0
        labels = np.where(w[labels] == 0.0, 0, labels)
    if not means:
        mu = None
    out = dict(Z=Z, labels=labels, mu=mu, cov=cov, w=w, upstream=upstream)
    out["ref"] = evaluate(Z, labels, mu, cov, w, upstream)
    return out
