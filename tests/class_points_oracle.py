"""Float64 oracle of the feature moments of labelled points: the dense class statistics of
tests/class_statistics_oracle.py (numpy, one class at a time), then F cov F^T, F mu and cov_f + m m^T; for gradients,
float64 torch autograd on the CPU through that dense expression for
    L = sum_c <A_c, S_c> + sum_c <b_c, m_c>     over the classes with at least two points,
with A (C,K,K) random and NOT symmetric and b (C,K) random.  Nothing here uses the formulas under test (centred
features, per-row weights): the (C,D,D) statistics are formed and projected."""
import numpy as np
import torch

import class_statistics_oracle as cso

ROW_BLOCK = 64    # B: grouped rows per workgroup of the projection kernel
ROW_RANGE = 64    # R: rows per range of the backward product at these sizes (one or two chunks of 32)
LONG_CLASS = 2 * max(ROW_BLOCK, ROW_RANGE) + 1


def feature_moments(X, y, F, n_classes=None, stats=None):
    """{'means' (C,K), 'covariances' (C,K,K), 'second_moments' (C,K,K)} in float64; NaN where the dense statistics are."""
    st = cso.class_statistics(X, y, n_classes=n_classes) if stats is None else stats
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        cov = np.einsum("kd,cde,le->ckl", F, st["covariances"], F)
        means = st["means"] @ F.T
    return {"means": means, "covariances": cov, "second_moments": cov + means[:, :, None] * means[:, None, :]}


def loss_terms(C, K, seed):
    """Random (A (C,K,K) non-symmetric, b (C,K)) of the test loss."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((C, K, K)), rng.standard_normal((C, K))


def loss_gradient(X, y, F, A, b, n_classes=None, second_moments=False, stats=None):
    """(L, dL/dF (K,D), keep (C) bool) of L = sum <A_c, S_c> + sum <b_c, m_c> over the classes `keep` with n_c >= 2,
    S the feature covariances (or second moments), through float64 autograd on the dense expression."""
    st = cso.class_statistics(X, y, n_classes=n_classes) if stats is None else stats
    C = st["means"].shape[0]
    keep = np.bincount(np.asarray(y).astype(np.int64), minlength=C) >= 2
    Ft = torch.tensor(np.asarray(F, dtype=np.float64), requires_grad=True)
    cov, mu = torch.tensor(st["covariances"][keep]), torch.tensor(st["means"][keep])
    S = Ft @ cov @ Ft.T
    m = mu @ Ft.T
    if second_moments:
        S = S + m[:, :, None] * m[:, None, :]
    L = (torch.tensor(A[keep]) * S).sum() + (torch.tensor(b[keep]) * m).sum()
    L.backward()
    return float(L.detach()), Ft.grad.numpy(), keep


def filters(K, D, seed=0):
    """(K,D) float32-representable filters with rows of about unit norm."""
    rng = np.random.default_rng(1000 * K + D + seed)
    return (rng.standard_normal((K, D)) / np.sqrt(D)).astype(np.float32).astype(np.float64)


def tails_with_long_class(D):
    """class_statistics_oracle.tails(D) (classes of 0, 1, 2, 3, 17 and 70 points) and one more class of LONG_CLASS points:
    longer than two row blocks of the projection and two row ranges of the backward product.  Shuffled."""
    X, y = cso.tails(D)
    rng = np.random.default_rng(500 + D)
    C = len(cso.TAIL_SIZES)
    Xl = rng.standard_normal((LONG_CLASS, D)) * rng.uniform(0.5, 2.0, size=(1, D)) + 0.5 * rng.standard_normal((1, D))
    X = np.concatenate([X, Xl.astype(np.float32).astype(np.float64)])
    y = np.concatenate([y, np.full(LONG_CLASS, C)])
    perm = rng.permutation(len(y))
    return X[perm], y[perm]


def few_long_classes(C=2, D=24, n=300, seed=8):
    """Few classes of many points: the Gram kernel splits each class over several workgroups (C = 2, N = 600: 5 shares)."""
    rng = np.random.default_rng(seed)
    y = np.repeat(np.arange(C), n)
    X = rng.standard_normal((C * n, D)) * rng.uniform(0.5, 2.0, size=(1, D)) + 0.5 * rng.standard_normal((C, D))[y]
    perm = rng.permutation(C * n)
    return X.astype(np.float32).astype(np.float64)[perm], y[perm]


def check_values(stats, ref, tol, keys=("means", "covariances", "second_moments"), what=""):
    """Same NaN pattern and rel_err below tol over the finite entries, per key (class_statistics_oracle.check_against for
    the keys present).  Returns the errors."""
    errs = {}
    for key in keys:
        got = np.asarray(stats[key].detach().cpu().numpy(), dtype=np.float64)
        want = ref[key]
        assert got.shape == want.shape, (what, key, got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, key, "NaN pattern")
        ok = ~np.isnan(want)
        den = np.linalg.norm(want[ok])
        errs[key] = np.linalg.norm(got[ok] - want[ok]) / (den if den > 0 else 1.0)
        assert errs[key] < tol, (what, key, errs[key])
    return errs
