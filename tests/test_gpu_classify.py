"""GPU tests of the native Gaussian class scores (sqfa_gauss_class_factors, sqfa_gauss_scores through sqfa_amd.classify)
against the float64 numpy oracle tests/classify_oracle.py.

Shapes (C, K, N).  The kernel's boundaries: the MFMA k-step of 4 and the 16-row block of K (K = 1, 3, 4, 5, 16, 17, 33, 48,
64: every one of the four row-block variants, one and four classes per stage), 16 samples per wave and 64 per workgroup
(N = 1, 17, 65, 257 = 4 x 64 + 1, 513), classes in groups of 4 (C = 1, 2, 3, 5, 9, 17 = 4 x 4 + 1, 37, 130 = 4 x 32 + 2, and
300, a multiple of 4), and the class splits: below 1024 sample tiles the groups are split over up to 16 workgroups whose
partial reductions a second launch merges ((300, 16, 2000): 15 splits of 5 groups); (5, 3, 65537) has 1025 tiles, the
smallest N at which several groups run unsplit and the workgroup writes the results itself.

The float32 scores are also held, entry by entry, to the a priori bound of tests/classify_hard.py against its long double
truth; tests/test_gpu_classify_hard.py does the same on hard inputs at small shapes.
"""
import functools

import numpy as np
import pytest
import torch

import classify_hard
import classify_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
SHAPES = [(1, 1, 1), (2, 1, 65), (3, 3, 17), (17, 4, 257), (37, 16, 1000), (37, 17, 1000), (130, 5, 513), (9, 33, 300),
          (5, 64, 200), (300, 16, 2000), (4, 48, 100), (5, 3, 65537)]
# (C, K, N, sep, means, priors): every shape with sep 1 and uniform priors, a few with sep 0, one with zero means, one with
# non-uniform priors that include a zero
CASES = [(C, K, N, 1.0, True, False) for C, K, N in SHAPES] + \
        [(C, K, N, 0.0, True, False) for C, K, N in [(3, 3, 17), (37, 17, 1000), (300, 16, 2000)]] + \
        [(9, 33, 300, 0.0, False, False), (37, 16, 1000, 1.0, True, True)]


def _ids(case):
    C, K, N, sep, means, priors = case
    return f"C{C}-K{K}-N{N}-sep{sep:g}" + ("" if means else "-zeromean") + ("-priors" if priors else "")


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    """The problem rounded to `dtype` (what every implementation is given), the float64 oracle on exactly those numbers, and
    for float32 the bound of the project's float32 convention: max(1e-5 (1 + max |score|), 5 x the max abs error of the same
    formula in float32 torch on the same inputs), with the long double truth and the per-entry a priori bound of
    tests/classify_hard.py (truth_and_bound32) for the scores."""
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
    S = classify_oracle.scores(Z, mu, cov, w)
    E = classify_oracle.log_evidence(S)
    out = dict(Z=Z, labels=labels, mu=mu, cov=cov, w=w, S=S, E=E, pred=classify_oracle.predict(S),
               gap=classify_oracle.top_two_gap(S), finite=np.isfinite(S))
    smax = np.abs(S[out["finite"]]).max()
    if dtype == torch.float64:
        out["bound"], out["torch_err"] = None, None
    else:
        # the same formula in float32 torch (CPU): Cholesky, triangular solve, squares, offset
        Zt, covt = torch.tensor(Z), torch.tensor(cov)
        L = torch.linalg.cholesky(covt)
        diff = Zt[None] - torch.tensor(mu)[:, None] if mu is not None else Zt[None].expand(C, N, K)
        y = torch.linalg.solve_triangular(L, diff.transpose(-1, -2), upper=False)
        lp = torch.tensor(classify_oracle.log_priors(w, C), dtype=torch.float32)
        St = (-0.5 * (y * y).sum(1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)[:, None]
              - np.float32(0.5 * K * np.log(2 * np.pi)) + lp[:, None]).T.double().numpy()
        out["torch_err"] = np.abs(St[out["finite"]] - S[out["finite"]]).max()
        out["bound"] = max(1e-5 * (1 + smax), 5 * out["torch_err"])
        out["torch_pred_wrong"] = int((St.argmax(1) != out["pred"]).sum())
        # per entry: the long double truth and the a priori float32 bound of tests/classify_hard.py
        out["S_true"], out["entry_bound"] = classify_hard.truth_and_bound32(Z, mu, cov, classify_oracle.log_priors(w, C))
    return out


def _classifier(ref, dtype):
    from sqfa_amd import classify
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype, device=DEV)
    clf = classify.GaussianClassifier(t(ref["mu"]), t(ref["cov"]), None if ref["w"] is None else ref["w"])
    assert clf._factors is not None, "the native factor pass did not run"
    return clf, t(ref["Z"])


def _check_values(got, want, ref, dtype, what):
    got = got.double().cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), f"{what}: -inf entries differ"
    err = np.abs(got[fin] - want[fin])
    if dtype == torch.float64:
        rel = (err / (1 + np.abs(want[fin]))).max()
        print(f"{what}: max error relative to 1 + |value| {rel:.3e}")
        assert rel <= 1e-10
    else:
        print(f"{what}: max abs error {err.max():.3e}, bound {ref['bound']:.3e}, float32 torch {ref['torch_err']:.3e}, "
              f"ratio to torch {err.max() / max(ref['torch_err'], 1e-30):.2f}")
        assert err.max() <= ref["bound"]
        if what == "scores":
            ratio = (np.abs(got[fin].astype(np.longdouble) - ref["S_true"][fin]) / ref["entry_bound"][fin]).max()
            print(f"{what}: worst error / per-entry bound {float(ratio):.3f}")
            assert ratio <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_scores_evidence_and_predictions(case, dtype):
    ref = _reference(case, dtype)
    clf, Z = _classifier(ref, dtype)
    S = clf.scores(Z)
    assert S.shape == ref["S"].shape and S.dtype == dtype and not S.requires_grad
    _check_values(S, ref["S"], ref, dtype, "scores")
    E = clf.log_evidence(Z)
    _check_values(E, ref["E"], ref, dtype, "log_evidence")
    pred = clf.predict(Z)
    assert pred.dtype == torch.int64 and pred.shape == (case[2],)
    pred = pred.cpu().numpy()
    sure = ref["gap"] > (0.0 if dtype == torch.float64 else ref["bound"])
    excluded = 1.0 - sure.mean()
    print(f"predict: {excluded:.4%} of the samples excluded (top-two gap within the bound), "
          f"{int((pred != ref['pred']).sum())} of {len(pred)} differ from the oracle"
          + ("" if dtype == torch.float64 else f", float32 torch mispredicts {ref['torch_pred_wrong']}"))
    assert np.array_equal(pred[sure], ref["pred"][sure])
    if dtype == torch.float32:
        assert excluded <= 0.02   # float64: only exact ties (gap == 0) are excluded
    if ref["w"] is not None:
        assert not np.isin(pred, np.nonzero(ref["w"] == 0)[0]).any()
    acc = clf.accuracy(Z, torch.tensor(ref["labels"], device=DEV))
    assert isinstance(acc, float) and acc == float((pred == ref["labels"]).mean())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[7], CASES[9], CASES[11], CASES[-2], CASES[-1]], ids=_ids)
def test_outputs_are_consistent_and_reproducible(case, dtype):
    ref = _reference(case, dtype)
    clf, Z = _classifier(ref, dtype)
    S, A, E, bad = clf._native_call(Z, scores=True, argmax=True, logsumexp=True)
    _, A1, _, _ = clf._native_call(Z, argmax=True)
    _, _, E1, _ = clf._native_call(Z, logsumexp=True)
    _, A2, E2, _ = clf._native_call(Z, argmax=True, logsumexp=True)
    S3, A3, E3, _ = clf._native_call(Z, scores=True, argmax=True, logsumexp=True)
    assert int(bad.item()) == 0
    assert torch.equal(A, A1) and torch.equal(A, A2) and torch.equal(A, A3)
    bits = lambda t: t.view(torch.int32 if dtype == torch.float32 else torch.int64)
    assert torch.equal(bits(E), bits(E1)) and torch.equal(bits(E), bits(E2)) and torch.equal(bits(E), bits(E3))
    assert torch.equal(bits(S), bits(S3))
    # the index is the argmax of the scores the same call wrote, ties to the lowest index
    assert torch.equal(A, S.argmax(1))
    logp = clf.predict_log_proba(Z)
    resid = torch.logsumexp(logp.double(), 1).abs().max().item()
    print(f"predict_log_proba: rows logsumexp to 0 within {resid:.3e}")
    assert resid <= (1e-10 * (1 + np.abs(ref["E"]).max()) if dtype == torch.float64 else ref["bound"])
    assert torch.allclose(clf.predict_proba(Z).sum(1), torch.ones(case[2], dtype=dtype, device=DEV), atol=1e-4)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_ties_go_to_the_lowest_index(dtype):
    Z, _, mu, cov = classify_oracle.problem(3, 5, 300, 1.0, seed=4)
    from sqfa_amd import classify
    t = lambda a: torch.tensor(a, dtype=dtype, device=DEV)
    pick = [0, 1, 1, 2, 1, 1, 2, 0, 1]   # copies of a class in other groups of 4 and, with 300 samples, in other splits
    first = np.array([0, 1, 3])
    base = classify.GaussianClassifier(t(mu), t(cov)).predict(t(Z)).cpu().numpy()
    pred = classify.GaussianClassifier(t(mu[pick]), t(cov[pick])).predict(t(Z)).cpu().numpy()
    assert set(base) == {0, 1, 2}
    assert np.array_equal(pred, first[base])


def test_predict_forms_nothing_of_size_n_by_c():
    from sqfa_amd import _lib, classify
    C, K, N = 257, 16, 4096
    Z, _, mu, cov = classify_oracle.problem(C, K, N, 1.0, seed=1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    clf, Zt = classify.GaussianClassifier(t(mu), t(cov)), t(Z)
    clf.predict(Zt[:64])   # the library and the allocator are warm
    ws = _lib.load().sqfa_gauss_scores_workspace_bytes(N, C, K, _lib.SQFA_F32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pred = clf.predict(Zt)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"predict at (C, K, N) = ({C}, {K}, {N}): peak rise {rise} bytes, workspace {ws}, (N, C) float32 {N * C * 4}")
    assert rise < ws + N * 8 + (1 << 20)
    assert pred.shape == (N,)
    rise0 = rise
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ev = clf.log_evidence(Zt)
    acc = clf.accuracy(Zt, pred)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < ws + N * 8 + N * 4 + N * 8 + (1 << 20) and acc == 1.0 and ev.shape == (N,) and rise0 < N * C * 4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_errors_come_through_the_device_counters(dtype):
    from sqfa_amd import classify
    Z, _, mu, cov = classify_oracle.problem(9, 5, 200, 1.0, seed=2)
    t = lambda a: torch.tensor(a, dtype=dtype, device=DEV)
    bad = cov.copy()
    bad[1] = -bad[1]
    bad[6, 2, 2] = np.nan
    bad[8, 4, 4] = 0.0
    bad[8, 4, :4] = bad[8, :4, 4] = 0.0
    with pytest.raises(ValueError, match="3 of 9 classes"):
        classify.GaussianClassifier(t(mu), t(bad))
    bad_mu = mu.copy()
    bad_mu[5, 0] = np.inf
    with pytest.raises(ValueError, match="1 of 9 classes"):
        classify.GaussianClassifier(t(bad_mu), t(cov))
    clf = classify.GaussianClassifier(t(mu), t(cov))
    assert clf._factors is not None
    Zn = Z.copy()
    Zn[[0, 63, 64, 199], [0, 1, 2, 4]] = np.nan
    for method in (clf.scores, clf.predict, clf.log_evidence, clf.predict_log_proba):
        with pytest.raises(ValueError, match="4 samples"):
            method(t(Zn))
    with pytest.raises(ValueError, match="4 samples"):
        clf.accuracy(t(Zn), torch.zeros(200, dtype=torch.int64, device=DEV))
    _, A, E, n_bad = clf._native_call(t(Zn), argmax=True, logsumexp=True)
    assert int(n_bad.item()) == 4
    assert (A.cpu().numpy() == -1).nonzero()[0].tolist() == [0, 63, 64, 199]
    assert torch.isnan(E).nonzero().flatten().tolist() == [0, 63, 64, 199]


def test_dispatch():
    from sqfa_amd import classify
    # K = 65: the torch expression, on the GPU
    Z, _, mu, cov = classify_oracle.problem(3, 65, 40, 1.0, seed=9)
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=DEV)
    clf = classify.GaussianClassifier(t(mu), t(cov))
    assert clf._factors is None
    S_ref = classify_oracle.scores(Z, mu, cov)
    S = clf.scores(t(Z))
    assert S.device.type == "cuda" and (np.abs(S.cpu().numpy() - S_ref) / (1 + np.abs(S_ref))).max() <= 1e-10
    assert np.array_equal(clf.predict(t(Z)).cpu().numpy(), classify_oracle.predict(S_ref))
    # an input that asks for a gradient: the torch expression, differentiable; without one the native pass, no graph
    Z, _, mu, cov = classify_oracle.problem(5, 6, 30, 1.0, seed=9)
    clf = classify.GaussianClassifier(t(mu), t(cov))
    assert clf._factors is not None
    Zg = t(Z).requires_grad_()
    Sg = clf.scores(Zg)
    assert Sg.requires_grad
    Sg.sum().backward()
    assert torch.isfinite(Zg.grad).all()
    with torch.no_grad():
        Sn = clf.scores(Zg)
    assert not Sn.requires_grad and torch.allclose(Sn, Sg.detach(), rtol=0, atol=1e-10 * (1 + Sg.detach().abs().max().item()))
    assert classify.GaussianClassifier(t(mu), t(cov).requires_grad_())._factors is None
    # the switch
    classify.NATIVE_CLASS_SCORES = False
    try:
        off = classify.GaussianClassifier(t(mu), t(cov))
        assert off._factors is None
        assert torch.allclose(off.scores(t(Z)), Sn, rtol=0, atol=1e-10 * (1 + Sn.abs().max().item()))
    finally:
        classify.NATIVE_CLASS_SCORES = True


def test_from_model_on_a_fitted_sqfa():
    import sqfa_amd
    from sqfa_amd import classify
    from sqfa_amd.statistics import ClassPoints, class_statistics
    C, D, per = 3, 8, 120
    g = torch.Generator().manual_seed(0)
    centres = 0.7 * torch.randn(C, D, generator=g)
    mix = torch.randn(C, D, D, generator=g) / D ** 0.5
    y = torch.arange(C).repeat_interleave(per)
    X = centres[y] + torch.einsum("nij,nj->ni", mix[y], torch.randn(C * per, D, generator=g))
    X, y = X.double().to(DEV), y.to(DEV)
    torch.manual_seed(1)
    m = sqfa_amd.model.SQFA(n_dim=D, n_filters=2, feature_noise=0.01).double().to(DEV)
    stats = class_statistics(X, y)
    m.fit(data_statistics=stats, max_epochs=5, show_progress=False)
    F = m.filters.detach().cpu().numpy()
    mu_f = stats["means"].cpu().numpy() @ F.T
    cov_f = F @ stats["covariances"].cpu().numpy() @ F.T + m.noise_mat.cpu().numpy()   # float32(0.01) widened, not 0.01
    S_ref = classify_oracle.scores(X.cpu().numpy() @ F.T, mu_f, cov_f)
    acc_ref = float((classify_oracle.predict(S_ref) == y.cpu().numpy()).mean())
    for given in (dict(data_statistics=stats), dict(data_statistics=ClassPoints(X, y)), dict(X=X, y=y)):
        fc = classify.FeatureClassifier.from_model(m, **given)
        assert fc.classifier._factors is not None
        S = fc.scores(X).cpu().numpy()
        assert (np.abs(S - S_ref) / (1 + np.abs(S_ref))).max() <= 1e-9
        assert classify_oracle.top_two_gap(S_ref).min() > 1e-8
        assert fc.accuracy(X, y) == acc_ref
    assert 1.0 / C < acc_ref <= 1.0
