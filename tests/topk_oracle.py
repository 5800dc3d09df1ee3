"""numpy helper of the top-k and label-rank tests (sqfa_amd.classify.predict_topk / label_rank / topk_accuracy).

The order of (score, class): higher score first, equal scores: lower class index first.  From an (N, C) score matrix:

    stable_order(S)              (N, C) class indices in that order
    rank(S, y)                   (N,) the number of classes placed before the labelled one
    rank_interval(S, e, y)       (lo, hi): what every score matrix within the per-entry bounds e of S can give
    topk_sets(S, e, k)           (surely_in, possibly_in) (N, C) bool, as below
    order_determined(S, e, k)    (N,) bool: the first k places are the same for every matrix within the bounds

Intervals.  With S the true scores and e >= 0 the bound of every computed entry (|computed - S| <= e), class c is *surely
before* the label y when S_c - e_c > S_y + e_y and *possibly before* it when S_c + e_c >= S_y - e_y; lo and hi are the two
counts.  For top-k, with tau the k-th largest true score and e_tau its entry's bound, the *surely-in* set is the classes
with S_c - e_c > tau + e_tau and the *possibly-in* set those with S_c + e_c >= tau - e_tau.  A -inf score (a class of prior 0)
is exact in every implementation (bound 0); between two -inf entries the class index decides, exactly.

The bounds: float32, classify_hard.truth_and_bound32 (long double truth and the a priori per-entry bound); float64, the
float64 oracle with e = 1e-10 (1 + |S|), the float64 tolerance of the class-score tests.
"""
import numpy as np


def stable_order(S):
    return np.argsort(-np.asarray(S), axis=1, kind="stable")


def rank(S, y):
    S = np.asarray(S)
    n = np.arange(S.shape[0])
    s_y = S[n, y][:, None]
    classes = np.arange(S.shape[1])[None]
    return ((S > s_y) | ((S == s_y) & (classes < np.asarray(y)[:, None]))).sum(1)


def bounds64(S):
    """The float64 tolerance as a per-entry bound; 0 where the score is -inf."""
    S = np.asarray(S)
    return np.where(np.isfinite(S), 1e-10 * (1 + np.abs(np.where(np.isfinite(S), S, 0))), 0.0)


def _exact(e, S):
    """The bound with 0 in place of whatever stands at the -inf entries (classify_hard puts inf there)."""
    return np.where(np.isneginf(S), 0, e)


def rank_interval(S, e, y):
    S, y = np.asarray(S), np.asarray(y)
    e = _exact(np.asarray(e), S)
    n = np.arange(S.shape[0])
    classes = np.arange(S.shape[1])[None]
    s_y, e_y = S[n, y][:, None], e[n, y][:, None]
    other = classes != y[:, None]
    both_inf = np.isneginf(S) & np.isneginf(s_y)   # decided by the index, exactly
    by_index = classes < y[:, None]
    with np.errstate(invalid="ignore"):
        sure = np.where(both_inf, by_index, S - e > s_y + e_y) & other
        possible = np.where(both_inf, by_index, S + e >= s_y - e_y) & other
    return sure.sum(1), possible.sum(1)


def topk_sets(S, e, k):
    S = np.asarray(S)
    e = _exact(np.asarray(e), S)
    n = np.arange(S.shape[0])
    at = stable_order(S)[:, k - 1]
    tau, e_tau = S[n, at][:, None], e[n, at][:, None]
    classes = np.arange(S.shape[1])[None]
    both_inf = np.isneginf(S) & np.isneginf(tau)
    with np.errstate(invalid="ignore"):
        sure = np.where(both_inf, classes < at[:, None], S - e > tau + e_tau)
        possible = np.where(both_inf, classes <= at[:, None], S + e >= tau - e_tau)
    return sure, possible


def order_determined(S, e, k):
    """Place i < k is determined when its entry's lower end lies above the upper end of every entry after it (two -inf
    entries: by their indices, always)."""
    S = np.asarray(S)
    e = _exact(np.asarray(e), S)
    order = stable_order(S)
    Ss, es = np.take_along_axis(S, order, 1), np.take_along_axis(e, order, 1)
    upper = Ss + es
    C = S.shape[1]
    # the largest upper end after place i; -inf after the last
    after = np.concatenate((np.maximum.accumulate(upper[:, ::-1], axis=1)[:, ::-1][:, 1:], np.full((S.shape[0], 1), -np.inf)), 1)
    k = min(k, C)
    ok = (Ss[:, :k] - es[:, :k] > after[:, :k]) | np.isneginf(Ss[:, :k])
    return ok.all(1)


def check_topk(index, scores, S, e, k):
    """The returned (N, k) indices (and scores, or None) against the intervals: surely-in within returned within possibly-in,
    k distinct classes, scores within the bound of the truth of their class and non-increasing.  Returns the share of samples
    whose returned order is not the true stable order (reported, not asserted)."""
    index = np.asarray(index)
    S = np.asarray(S)
    N, C = S.shape
    assert index.shape == (N, k) and index.min() >= 0 and index.max() < C
    returned = np.zeros((N, C), dtype=bool)
    returned[np.arange(N)[:, None], index] = True
    assert (returned.sum(1) == k).all(), "a class is returned twice"
    sure, possible = topk_sets(S, e, k)
    assert not (sure & ~returned).any(), "a class that is surely among the k best is missing"
    assert not (returned & ~possible).any(), "a class that cannot be among the k best is returned"
    if scores is not None:
        scores = np.asarray(scores)
        truth = np.take_along_axis(S, index, 1)
        bound = np.take_along_axis(_exact(np.asarray(e), S), index, 1)
        inf = np.isneginf(truth)
        assert np.array_equal(np.isneginf(scores), inf)
        err = np.abs(np.where(inf, 0, scores) - np.where(inf, 0, truth))
        assert (err <= bound).all(), f"a returned score misses its bound by {float((err - bound).max()):.3e}"
        assert (scores[:, 1:] <= scores[:, :-1]).all(), "the returned scores increase somewhere"
    return float((index != stable_order(S)[:, :k]).any(1).mean())


def check_rank(got, S, e, y):
    lo, hi = rank_interval(S, e, y)
    got = np.asarray(got)
    assert ((lo <= got) & (got <= hi)).all(), "a rank lies outside its interval"
    return float((lo != hi).mean())
