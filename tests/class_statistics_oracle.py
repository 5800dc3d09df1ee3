"""Float64 numpy oracle of the class statistics, straight from their definition, one class at a time:
mean, centred X^T X / (n - 1), OAS shrinkage (Chen et al. 2010; reference src/sqfa/statistics.py:57-94) and the
second moment cov + mu mu^T.  An empty class is NaN throughout and a class of one point has a NaN covariance, as the
reference's expressions give.  tests/test_class_statistics_oracle.py pins it to the reference's recorded outputs."""
import numpy as np


def sample_covariance(X):
    n = X.shape[0]
    centred = X - X.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return centred.T @ centred / np.float64(n - 1)


def oas(S, n):
    d = S.shape[0]
    tr = np.trace(S)
    tr2 = np.sum(S * S)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = ((1 - 2 / d) * tr2 + tr * tr) / ((n + 1 - 2 / d) * (tr2 - tr * tr / d))
    if rho > 1.0:      # NaN stays NaN
        rho = 1.0
    return (1 - rho) * S + rho * (tr / d) * np.eye(d)


def class_statistics(X, y, n_classes=None, estimator="empirical"):
    """X (N,D), y (N) integer labels -> dict of float64 means (C,D), covariances and second_moments (C,D,D)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y).astype(np.int64)
    C = int(y.max()) + 1 if n_classes is None else int(n_classes)
    D = X.shape[1]
    means = np.full((C, D), np.nan)
    covs = np.full((C, D, D), np.nan)
    for c in range(C):
        Xc = X[y == c]
        if Xc.shape[0] == 0:
            continue
        means[c] = Xc.mean(axis=0)
        S = sample_covariance(Xc)
        covs[c] = oas(S, Xc.shape[0]) if estimator == "oas" and Xc.shape[0] > 1 else S
    second = covs + means[:, :, None] * means[:, None, :]
    return {"means": means, "covariances": covs, "second_moments": second}


def check_against(stats, ref, tol, what=""):
    """Same NaN pattern, and rel_err (the project's metric: Frobenius norm of the difference over that of the oracle)
    below `tol` over the finite entries, for each of the three keys.  Returns the errors."""
    errs = {}
    for key in ("means", "covariances", "second_moments"):
        got = np.asarray(stats[key].detach().cpu().numpy() if hasattr(stats[key], "detach") else stats[key], dtype=np.float64)
        want = ref[key]
        assert got.shape == want.shape, (what, key, got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, key, "NaN pattern")
        ok = ~np.isnan(want)
        den = np.linalg.norm(want[ok])
        errs[key] = np.linalg.norm(got[ok] - want[ok]) / (den if den > 0 else 1.0)
        assert errs[key] < tol, (what, key, errs[key])
    return errs


def ragged_small(C=37, D=13, seed=909, dtype=np.float64, empty=(5, 20), lo=2, hi=42):
    """ragged_points-style data (tests/model_cases.py) at a small size: ragged class sizes, per-column scales, class
    offsets, shuffled; the classes in `empty` have no point.  Values are float32-representable."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi, size=C)
    sizes[list(empty)] = 0
    y = np.repeat(np.arange(C), sizes)
    X = rng.standard_normal((len(y), D)) * rng.uniform(0.5, 2.0, size=(1, D)) + 0.3 * rng.standard_normal((C, D))[y]
    X = X.astype(np.float32).astype(dtype)
    perm = rng.permutation(len(y))
    return X[perm], y[perm]


TAIL_SIZES = [0, 1, 2, 3, 17, 70]   # empty, singleton, not multiples of 4, one longer than two row chunks of 32


def tails(D):
    """One class per size in TAIL_SIZES, D columns, shuffled."""
    rng = np.random.default_rng(100 + D)
    C = len(TAIL_SIZES)
    y = np.repeat(np.arange(C), TAIL_SIZES)
    X = rng.standard_normal((len(y), D)) * rng.uniform(0.5, 2.0, size=(1, D)) + 0.5 * rng.standard_normal((C, D))[y]
    perm = rng.permutation(len(y))
    return X.astype(np.float32).astype(np.float64)[perm], y[perm]


def uneven_batches(n, parts=7, seed=11):
    """`parts` consecutive slices of range(n) of very different lengths."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 3.0, size=parts)
    cuts = np.concatenate([[0], np.round(np.cumsum(w) / w.sum() * n).astype(int)])
    cuts[-1] = n
    return [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def far_means(C=4, D=20, n=50, seed=3, dtype=np.float32):
    """Unit-variance classes whose means sit 100 standard deviations from the origin: a raw-moment formulation
    (sum x x^T - n mu mu^T) loses about four digits of the covariance here in float32."""
    rng = np.random.default_rng(seed)
    mu = 100.0 * rng.choice([-1.0, 1.0], size=(C, D))
    y = np.repeat(np.arange(C), n)
    X = (rng.standard_normal((C * n, D)) + mu[y]).astype(dtype)
    perm = rng.permutation(C * n)
    return X[perm], y[perm]
