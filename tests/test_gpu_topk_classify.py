"""GPU tests of the native top-k and label-rank kernels (sqfa_gauss_scores_topk, sqfa_gauss_label_rank through
sqfa_amd.classify and through the C ABI).

Two references.  (1) The native scores ``clf.scores(Z)``: the kernels form every score with the scorer's statements, so
predict_topk is the first k columns of a stable descending sort of that matrix, label_rank the tie-rule count on it and the
pre-pass's label score its gathered entry, all bit for bit, no tolerance and no exclusions.  (2) The independent oracle
(tests/classify_oracle.py in float64, the long double truth of tests/classify_hard.py in float32) with per-entry error
bounds, through the intervals of tests/topk_oracle.py: every sample is held to its interval.

The shapes are those of tests/test_gpu_classify.py (every row-block variant, one and four classes per stage, N = 1, 17, 65,
257, 513, class groups of 4 with tails, 15 splits at (300, 16, 2000), the unsplit path at (5, 3, 65537)); k in {1, 2, 3, 5,
8} capped at C, plus k = C where C <= 8: every list size 1, 2, 4, 8, full and partly used.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import classify_hard
import classify_oracle
import topk_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
SHAPES = [(1, 1, 1), (2, 1, 65), (3, 3, 17), (17, 4, 257), (37, 16, 1000), (37, 17, 1000), (130, 5, 513), (9, 33, 300),
          (5, 64, 200), (300, 16, 2000), (4, 48, 100), (5, 3, 65537)]
# (C, K, N, sep, means, priors), as tests/test_gpu_classify.py, and (130, 5, 513) with sep 0
CASES = [(C, K, N, 1.0, True, False) for C, K, N in SHAPES] + \
        [(C, K, N, 0.0, True, False) for C, K, N in [(3, 3, 17), (37, 17, 1000), (300, 16, 2000), (130, 5, 513)]] + \
        [(9, 33, 300, 0.0, False, False), (37, 16, 1000, 1.0, True, True)]


def _ids(case):
    C, K, N, sep, means, priors = case
    return f"C{C}-K{K}-N{N}-sep{sep:g}" + ("" if means else "-zeromean") + ("-priors" if priors else "")


def _ks(C):
    return sorted({min(k, C) for k in (1, 2, 3, 5, 8)} | ({C} if C <= 8 else set()))


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    """The problem rounded to `dtype`, the true scores S of exactly those numbers and the per-entry bound e of a computed
    score (float64: the float64 oracle and 1e-10 (1 + |S|); float32: the long double truth and the a priori bound of
    tests/classify_hard.py), and what the oracle alone determines: the rank intervals and the samples whose first five places
    are determined."""
    C, K, N, sep, means, priors = case
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, sep, seed=C + 7 * K)
    npdt = _np_dtype(dtype)
    Z, mu, cov = Z.astype(npdt), mu.astype(npdt), cov.astype(npdt)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    if not means:
        mu = None
    w = None
    if priors:
        w = 1.0 + np.arange(C) % 5
        w[[2, C - 1]] = 0.0
    if dtype == torch.float64:
        S = classify_oracle.scores(Z, mu, cov, w)
        e = topk_oracle.bounds64(S)
    else:
        S, e = classify_hard.truth_and_bound32(Z, mu, cov, classify_oracle.log_priors(w, C))
    lo, hi = topk_oracle.rank_interval(S, e, labels)
    out = dict(Z=Z, labels=labels, mu=mu, cov=cov, w=w, S=S, e=e, lo=lo, hi=hi,
               determined=topk_oracle.order_determined(S, e, 5))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _classifier(ref, dtype):
    from sqfa_amd import classify
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype, device=DEV)
    clf = classify.GaussianClassifier(t(ref["mu"]), t(ref["cov"]), None if ref["w"] is None else ref["w"].copy())
    assert clf._factors is not None, "the native factor pass did not run"
    return clf, t(ref["Z"]), torch.tensor(ref["labels"], device=DEV)


# ---- the C ABI, with every optional output ---------------------------------------------------------------------------------

def _abi_topk(clf, Z, k, want_scores=True):
    """(index (N,k), score (N,k) | None, the counter as a Python int) from one sqfa_gauss_scores_topk call."""
    from sqfa_amd import _lib, _native
    lib = _lib.load()
    Z = Z.contiguous()
    W, offset = clf._factors
    N, K, C = Z.shape[0], clf.n_features, clf.n_classes
    code = _native._dtype_code(Z)
    nbytes = lib.sqfa_gauss_scores_topk_workspace_bytes(N, C, K, code, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Z.device)
    index = torch.full((N, k), -7, dtype=torch.int64, device=Z.device)
    score = torch.full((N, k), 123.0, dtype=Z.dtype, device=Z.device) if want_scores else None
    bad = torch.full((1,), -7, dtype=torch.int32, device=Z.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sqfa_gauss_scores_topk(_native._ptr(Z), N, _native._ptr(clf._means_native), _native._ptr(W), _native._ptr(offset),
                                    C, K, code, k, _native._ptr(index), _native._ptr(score), _native._ptr(bad),
                                    _native._ptr(ws), nbytes, stream)
    assert rc == 0, lib.sqfa_hip_last_error()
    return index, score, int(bad.item())


def _abi_rank(clf, Z, y, want_score=True):
    """(rank (N,), label score (N,) | None, the two flags as Python ints) from one sqfa_gauss_label_rank call."""
    from sqfa_amd import _lib, _native
    lib = _lib.load()
    Z, y = Z.contiguous(), y.contiguous()
    W, offset = clf._factors
    N, K, C = Z.shape[0], clf.n_features, clf.n_classes
    code = _native._dtype_code(Z)
    nbytes = lib.sqfa_gauss_label_rank_workspace_bytes(N, C, K, code)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Z.device)
    rank = torch.full((N,), -7, dtype=torch.int64, device=Z.device)
    score = torch.full((N,), 123.0, dtype=Z.dtype, device=Z.device) if want_score else None
    flags = torch.full((2,), -7, dtype=torch.int32, device=Z.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sqfa_gauss_label_rank(_native._ptr(Z), _native._ptr(y), N, _native._ptr(clf._means_native), _native._ptr(W),
                                   _native._ptr(offset), C, K, code, _native._ptr(rank), _native._ptr(score),
                                   _native._ptr(flags), _native._ptr(ws), nbytes, stream)
    assert rc == 0, lib.sqfa_hip_last_error()
    return rank, score, flags.tolist()


def _tie_rule_rank(S, y):
    s_y = S.gather(1, y[:, None])
    classes = torch.arange(S.shape[1], device=S.device)[None]
    return ((S > s_y) | ((S == s_y) & (classes < y[:, None]))).sum(1)


def _check_exact(clf, Z, y, ks):
    """Test 1 of the module docstring on one classifier: everything against the native scores, bit for bit."""
    N = Z.shape[0]
    S = clf.scores(Z)
    top, order = torch.sort(S, dim=1, descending=True, stable=True)
    pred = clf.predict(Z)
    for k in ks:
        index, score = clf.predict_topk(Z, k, return_scores=True)
        assert index.shape == (N, k) and index.dtype == torch.int64 and score.dtype == Z.dtype and not score.requires_grad
        assert torch.equal(index, order[:, :k]), f"k = {k}: indices differ from the stable sort of the native scores"
        assert torch.equal(_bits(score), _bits(top[:, :k])), f"k = {k}: scores are not the native scores' bits"
        assert torch.equal(index[:, 0], pred)
    rank = clf.label_rank(Z, y)
    assert rank.shape == (N,) and rank.dtype == torch.int64
    assert torch.equal(rank, _tie_rule_rank(S, y))
    assert torch.equal(rank == 0, pred == y)
    abi_rank, label_score, flags = _abi_rank(clf, Z, y)
    assert flags == [0, 0] and torch.equal(abi_rank, rank)
    assert torch.equal(_bits(label_score), _bits(S.gather(1, y[:, None])[:, 0])), "the pre-pass misses the scorer's bits"
    acc = clf.topk_accuracy(Z, y, k=(1, 2, 5))
    assert acc.tolist() == [int((rank < k).sum().item()) / N for k in (1, 2, 5)]   # the share as the method forms it: count / N
    assert clf.topk_accuracy(Z, y, k=1) == clf.accuracy(Z, y)
    return S, rank


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact_against_the_native_scores(case, dtype):
    ref = _reference(case, dtype)
    clf, Z, y = _classifier(ref, dtype)
    _check_exact(clf, Z, y, _ks(case[0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_sample_within_its_oracle_interval(case, dtype):
    ref = _reference(case, dtype)
    C, N = case[0], case[2]
    # the condition, from the oracle alone: the intervals pin down nearly every sample
    decided = (ref["lo"] == ref["hi"]) & ref["determined"]
    print(f"{_ids(case)}: {decided.mean():.4%} of the samples have lo == hi and a determined top-5 order")
    assert decided.mean() >= 0.99
    clf, Z, y = _classifier(ref, dtype)
    rank = clf.label_rank(Z, y).cpu().numpy()
    topk_oracle.check_rank(rank, ref["S"], ref["e"], ref["labels"])
    for k in _ks(C):
        index, score = clf.predict_topk(Z, k, return_scores=True)
        index, score = index.cpu().numpy(), score.cpu().numpy().astype(np.longdouble)
        topk_oracle.check_topk(index, score, ref["S"], ref["e"], k)
        if k <= 5:
            sure = ref["determined"]
            assert np.array_equal(index[sure], topk_oracle.stable_order(ref["S"])[sure, :k])
    # the torch expression on the same GPU agrees wherever the oracle determines the answer
    from sqfa_amd import classify
    classify.NATIVE_TOPK = False
    try:
        k = min(5, C)
        index_t = clf.predict_topk(Z, k).cpu().numpy()
        rank_t = clf.label_rank(Z, y).cpu().numpy()
    finally:
        classify.NATIVE_TOPK = True
    index = clf.predict_topk(Z, k).cpu().numpy()
    assert np.array_equal(index_t[ref["determined"]], index[ref["determined"]])
    same = ref["lo"] == ref["hi"]
    assert np.array_equal(rank_t[same], rank[same])


def _duplicated(C, N, dtype, seed):
    """C classes, class c again at c + C / 2: equal scores bit for bit."""
    from sqfa_amd import classify
    Z, labels, mu, cov = classify_oracle.problem(C // 2, 16, N, 0.5, seed=seed)
    pick = list(range(C // 2)) * 2
    t = lambda a: torch.tensor(a, dtype=dtype, device=DEV)
    y = torch.tensor(labels + (np.arange(N) % 2) * (C // 2), device=DEV)   # labels on first and on second copies
    return classify.GaussianClassifier(t(mu[pick]), t(cov[pick])), t(Z), y


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("C", [10, 302])
def test_ties_across_groups_stages_and_splits(C, dtype):
    # N = 300: five sample tiles, so the class groups are split (C = 10: 3 splits of one group; C = 302: 16 splits of 5
    # groups) and c, c + C / 2 fall into different lane quarters, groups (= stages at K = 16) and splits
    clf, Z, y = _duplicated(C, 300, dtype, seed=C)
    S, rank = _check_exact(clf, Z, y, _ks(C))
    assert torch.equal(_bits(S[:, :C // 2]), _bits(S[:, C // 2:])), "the copies do not tie"
    index = clf.predict_topk(Z, 8)
    assert torch.equal(index[:, 0::2] + C // 2, index[:, 1::2])   # every class directly before its copy
    first = y < C // 2
    assert (rank[first] % 2 == 0).all() and (rank[~first] % 2 == 1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_k_reaches_into_the_classes_of_prior_zero(dtype):
    from sqfa_amd import classify
    C, K, N = 9, 16, 300
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, 0.5, seed=5)
    w = np.array([0, 1.0, 0, 0, 2.0, 0, 0, 0.5, 0])   # 6 zeros: three finite scores per row
    t = lambda a: torch.tensor(a, dtype=dtype, device=DEV)
    clf = classify.GaussianClassifier(t(mu), t(cov), w)
    y = torch.tensor(labels, device=DEV)               # two thirds of the labels lie on classes of prior 0
    _check_exact(clf, t(Z), y, [1, 3, 4, 5, 8])
    index, score = clf.predict_topk(t(Z), 5, return_scores=True)
    assert torch.isfinite(score[:, :3]).all() and torch.isneginf(score[:, 3:]).all()
    assert (index[:, 3:] == torch.tensor([0, 2], device=DEV)).all()   # among -inf entries the lower index first
    rank = clf.label_rank(t(Z), y)
    zero = torch.tensor(w == 0, device=DEV)[y]
    assert torch.equal(rank[zero], 3 + torch.tensor(np.cumsum(w == 0) - 1, device=DEV)[y][zero])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(37, 16, 1000), (5, 3, 65537), (300, 16, 2000)], ids=lambda s: "C%d-K%d-N%d" % s)
def test_flags_through_the_c_abi(shape, dtype):
    from sqfa_amd import classify
    C, K, N = shape
    ref = _reference((C, K, N, 1.0, True, False), dtype)
    clf, Z, y = _classifier(ref, dtype)
    clean_index, clean_score, count = _abi_topk(clf, Z, 3)
    clean_rank, clean_label, flags = _abi_rank(clf, Z, y)
    assert count == 0 and flags == [0, 0]
    # one sample with a NaN feature and one with +inf
    Zb = Z.clone()
    rows = [70, N - 1]
    Zb[rows[0], 0], Zb[rows[1], K - 1] = float("nan"), float("inf")
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[rows] = False
    index, score, count = _abi_topk(clf, Zb, 3)
    assert count == 2
    assert (index[rows] == -1).all() and torch.isnan(score[rows]).all()
    assert torch.equal(index[keep], clean_index[keep]) and torch.equal(_bits(score[keep]), _bits(clean_score[keep]))
    # labels -1, C and 2^40: nothing is addressed with them
    yb = y.clone()
    where = [0, 71, N - 2]
    yb[where] = torch.tensor([-1, C, 2 ** 40], device=DEV)
    rank, label, flags = _abi_rank(clf, Zb, yb)
    assert flags == [2, 3]
    assert (rank[rows + where] == -1).all() and torch.isnan(label[rows + where]).all()
    keep[where] = False
    assert torch.equal(rank[keep], clean_rank[keep]) and torch.equal(_bits(label[keep]), _bits(clean_label[keep]))
    # the Python methods name the counts
    with pytest.raises(ValueError, match="2 samples have non-finite scores"):
        clf.predict_topk(Zb, 3)
    with pytest.raises(ValueError, match="2 samples have non-finite scores"):
        clf.label_rank(Zb, y)
    with pytest.raises(ValueError, match=f"3 labels are outside \\[0, {C}\\)"):
        clf.label_rank(Z, yb)
    with pytest.raises(ValueError, match=f"3 labels are outside \\[0, {C}\\)"):
        clf.topk_accuracy(Zb, yb)
    with pytest.raises(ValueError, match="2 samples have non-finite scores"):
        clf.topk_accuracy(Zb, y, k=3)
    assert classify.NATIVE_TOPK is True


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[7], CASES[8], CASES[9], CASES[11], CASES[-1]], ids=_ids)
def test_reproducible_and_independent_of_the_outputs_asked_for(case, dtype):
    ref = _reference(case, dtype)
    clf, Z, y = _classifier(ref, dtype)
    for k in _ks(case[0]):
        index, score, _ = _abi_topk(clf, Z, k)
        index2, score2, _ = _abi_topk(clf, Z, k)
        alone, none, _ = _abi_topk(clf, Z, k, want_scores=False)
        assert none is None
        assert torch.equal(index, index2) and torch.equal(_bits(score), _bits(score2)) and torch.equal(index, alone)
    rank, label, _ = _abi_rank(clf, Z, y)
    rank2, label2, _ = _abi_rank(clf, Z, y)
    alone, none, _ = _abi_rank(clf, Z, y, want_score=False)
    assert none is None
    assert torch.equal(rank, rank2) and torch.equal(_bits(label), _bits(label2)) and torch.equal(rank, alone)


def test_nothing_of_size_n_by_c_is_formed():
    from sqfa_amd import _lib, classify
    C, K, N = 257, 16, 4096
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, 1.0, seed=1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    clf, Zt, y = classify.GaussianClassifier(t(mu), t(cov)), t(Z), torch.tensor(labels, device=DEV)
    clf.predict_topk(Zt[:64], 5), clf.label_rank(Zt[:64], y[:64])   # the library and the allocator are warm
    lib = _lib.load()
    ws_topk = lib.sqfa_gauss_scores_topk_workspace_bytes(N, C, K, _lib.SQFA_F32, 5)
    ws_rank = lib.sqfa_gauss_label_rank_workspace_bytes(N, C, K, _lib.SQFA_F32)
    for call, allowed in ((lambda: clf.predict_topk(Zt, 5, return_scores=True), ws_topk + N * 5 * 12),
                          (lambda: clf.label_rank(Zt, y), ws_rank + N * 8)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print(f"peak rise {rise} bytes, allowed {allowed} + 1 MiB, (N, C) float32 {N * C * 4}")
        assert rise < allowed + (1 << 20) and rise < N * C * 4
        del out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_feature_classifier(dtype):
    import sqfa_amd
    from sqfa_amd import classify
    C, D, K, N = 5, 12, 4, 100
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(C, D, generator=g)
    y = torch.arange(N) % C
    X = (centres[y] + torch.randn(N, D, generator=g)).to(dtype).to(DEV)
    y = y.to(DEV)
    torch.manual_seed(1)
    m = sqfa_amd.model.SQFA(n_dim=D, n_filters=K, feature_noise=0.01).to(dtype).to(DEV)
    fc = classify.FeatureClassifier.from_model(m, X=X, y=y)
    assert fc.classifier._factors is not None
    Zf = fc.transform(X)
    for k in (1, 3, 5):
        index, score = fc.predict_topk(X, k, return_scores=True)
        want = fc.classifier.predict_topk(Zf, k, return_scores=True)
        assert torch.equal(index, want[0]) and torch.equal(_bits(score), _bits(want[1]))
    assert torch.equal(fc.predict_topk(X, 2), fc.classifier.predict_topk(Zf, 2))
    assert torch.equal(fc.label_rank(X, y), fc.classifier.label_rank(Zf, y))
    assert torch.equal(fc.topk_accuracy(X, y), fc.classifier.topk_accuracy(Zf, y))
    assert fc.topk_accuracy(X, y, k=1) == fc.accuracy(X, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_wide_shapes_with_few_classes_rank_through_the_native_scores(dtype):
    """K > 48 with fewer than 512 classes: label_rank counts on the native scores (the shape condition of the README's
    table); the rank kernels give the same ranks and flags there."""
    from sqfa_amd import classify
    assert (classify.RANK_WIDE_FEATURES, classify.RANK_WIDE_MIN_CLASSES) == (48, 512)
    ref = _reference(CASES[8], dtype)   # (5, 64, 200)
    clf, Z, y = _classifier(ref, dtype)
    y = y.clone()
    y[[3, 150]] = torch.tensor([-2, 5], device=DEV)
    Z = Z.clone()
    Z[17, 63] = float("nan")
    by_scores, by_kernels = clf._scores_rank(Z, y), clf._native_rank(Z, y)
    assert torch.equal(by_scores[0], by_kernels[0]) and by_scores[1].tolist() == by_kernels[1].tolist() == [1, 2]
    assert (by_scores[0][[3, 17, 150]] == -1).all()
    assert torch.equal(clf._rank(Z, y)[0], by_scores[0])
