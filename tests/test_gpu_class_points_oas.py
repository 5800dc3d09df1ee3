"""GPU tests of OAS shrinkage in points mode (sqfa_class_shrinkage, sqfa_class_feature_moments_shrunk and its backward,
statistics.ClassPoints(estimator="oas"), fit(data_statistics=ClassPoints(X, y, estimator="oas"))) against the float64 oracle:
tests/class_statistics_oracle.py with estimator="oas", then the dense projection and autograd of
tests/class_points_oracle.py.  Bounds: the project's own for class statistics, rel_err < 1e-11 in float64 and < 2e-5 in
float32, on values and on dL/dF; model level: the float64 gradient bound 1e-8 and the README's float32 rule.  The models,
closures and shapes are those of tests/test_gpu_class_points.py, whose helpers are used here."""
import numpy as np
import pytest
import torch

import class_points_oracle as cpo
import class_statistics_oracle as cso
import model_cases as mc
import test_gpu_class_points as base
from conftest import rel_err
from sqfa_amd import _native, linalg, model as model_module, statistics
from sqfa_amd.statistics import ClassPoints

pytestmark = pytest.mark.gpu
DEV = base.DEV
DTYPES = base.DTYPES
KS = base.KS
OAS_OPS = ["affine_invariant", "bhattacharyya", "fisher_rao_lower_bound", "log_euclidean"]


@pytest.fixture
def no_index_add(monkeypatch):
    """The torch expression's index_add raises: whatever passes ran the native kernels."""
    def refuse(*a, **k):
        raise AssertionError("index_add called: the torch path ran")
    monkeypatch.setattr(torch, "index_add", refuse)
    monkeypatch.setattr(torch.Tensor, "index_add_", refuse)


_refs, _grads = {}, {}


def reference(name, make, n_classes=None):
    """(X, y, dense float64 OAS oracle statistics) of a named input, computed once per session and shared."""
    if name not in _refs:
        X, y = make()
        _refs[name] = (X, y, cso.class_statistics(X, y, n_classes=n_classes, estimator="oas"))
    return _refs[name]


def reference_gradient(name, K, second, seed):
    key = (name, K, second, seed)
    if key not in _grads:
        X, y, dense = _refs[name]
        A, b = cpo.loss_terms(dense["means"].shape[0], K, seed)
        _, g, keep = cpo.loss_gradient(X, y, cpo.filters(K, X.shape[1]), A, b, second_moments=second, stats=dense)
        _grads[key] = (A, b, g, keep)
    return _grads[key]


def nan_as(t, value=-7.0):
    return torch.nan_to_num(t, nan=value)


def check_input(name, Xn, yn, dense, dtype, tol, Ks, n_classes=None):
    X, y = base.dev(Xn, yn, dtype)
    cp = ClassPoints(X, y, n_classes=n_classes, estimator="oas")
    D = Xn.shape[1]
    for K in Ks:
        Fn = cpo.filters(K, D)
        F = torch.tensor(Fn, dtype=dtype, device=DEV)
        st = cp.feature_statistics(F, second_moments=True)
        errs = cpo.check_values(st, cpo.feature_moments(Xn, yn, Fn, stats=dense), tol, what=(name, K))
        gerr = []
        for second in (False, True):
            A, b, g_ref, keep = reference_gradient(name, K, second, seed=7 * D + K)
            g = base.loss_gradient(cp, F, A, b, keep, second)
            assert torch.isfinite(g).all()
            gerr.append(rel_err(g.cpu().numpy(), g_ref))
        print(f"oas {name} K={K} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", grad {gerr[0]:.2e} / {gerr[1]:.2e}")
        assert max(gerr) < tol, (name, K, gerr)
    return cp


# ---- the coefficients are the dense kernel's -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [5, 65, 132])
def test_coefficients_are_the_dense_kernels(D, dtype, no_index_add):
    """class_statistics(oas) = keep_c class_statistics(empirical) + shift_c I with the keep and shift of ClassPoints: off the
    diagonal one rounding, so bit for bit (NaN classes equal as NaN); on the diagonal within 4 ulp of the diagonal's largest
    entry (the compiler may contract the dense kernel's multiply-add).  Classes of 0, 1, 2, 3, 17 and 70 points; D = 65 and
    132 have off-diagonal tiles."""
    Xn, yn = cso.tails(D)
    X, y = base.dev(Xn, yn, dtype)
    oas = statistics.class_statistics(X, y, estimator="oas")["covariances"]
    emp = statistics.class_statistics(X, y)["covariances"]
    cp = ClassPoints(X, y, estimator="oas")
    again = ClassPoints(X, y, estimator="oas")
    for a, b in ((cp.shrink_keep, again.shrink_keep), (cp.shrink_shift, again.shrink_shift), (cp.shrinkage, again.shrinkage)):
        assert torch.equal(nan_as(a), nan_as(b))
    full = cp.counts >= 2
    assert cp.shrink_keep.dtype == dtype and cp.shrinkage.dtype == torch.float64
    for t in (cp.shrink_keep, cp.shrink_shift, cp.shrinkage):
        assert torch.isnan(t[~full]).all() and torch.isfinite(t[full]).all()
    assert torch.equal(cp.shrink_keep[full], (1.0 - cp.shrinkage[full]).to(dtype))
    off = ~torch.eye(D, dtype=torch.bool, device=DEV)
    kept = cp.shrink_keep[:, None, None] * emp
    assert torch.equal(nan_as(oas[:, off]), nan_as(kept[:, off]))
    diag = torch.diagonal(oas, dim1=1, dim2=2)[full]
    want = (torch.diagonal(kept, dim1=1, dim2=2) + cp.shrink_shift[:, None])[full]
    ulp = torch.finfo(dtype).eps * diag.abs().amax(dim=1, keepdim=True)
    print(f"D={D} {dtype}: rho {cp.shrinkage[full].tolist()}, diagonal off by at most {((diag - want).abs() / ulp).max():.2f} ulp")
    assert ((diag - want).abs() <= 4 * ulp).all()
    # and the oracle's rho (float64: 1e-11; float32: 2e-5 times tr2 / (tr2 - tr^2 / D), the amplification of the ratio)
    for c in torch.nonzero(full).flatten().tolist():
        S = cso.sample_covariance(Xn[yn == c])
        tr, tr2, n = np.trace(S), np.sum(S * S), int(cp.counts[c])
        rho = min(((1 - 2 / D) * tr2 + tr * tr) / ((n + 1 - 2 / D) * (tr2 - tr * tr / D)), 1.0)
        bound = 1e-11 if dtype == torch.float64 else 2e-5 * tr2 / (tr2 - tr * tr / D)
        assert abs(float(cp.shrinkage[c]) - rho) < bound, (c, float(cp.shrinkage[c]), rho)
    if D == 5:   # three points in five dimensions: clamped
        assert float(cp.shrinkage[3]) == 1.0 and float(cp.shrink_keep[3]) == 0.0


# ---- values and dL/dF against the oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("D", [3, 5, 17, 63, 65, 100, 132])
def test_column_and_row_tails(D, dtype, tol, no_index_add):
    """Classes of 0, 1, 2, 3, 17, 70 and 129 points, every filter-block count and its tails, capped at D.  K = 64 puts the
    filter rows of the backward product over two chunks of 32 rows; D >= 65 has several stripes and off-diagonal tiles of
    the measuring SYRK."""
    name = f"tailsL{D}"
    Xn, yn, dense = reference(name, lambda: cpo.tails_with_long_class(D))
    cp = check_input(name, Xn, yn, dense, dtype, tol, sorted({min(K, D) for K in KS}))
    st = cp.feature_statistics(torch.tensor(cpo.filters(1, D), dtype=dtype, device=DEV), second_moments=True)
    assert torch.isnan(st["means"][0]).all() and torch.isfinite(st["means"][1:]).all()
    for k in ("covariances", "second_moments"):
        assert torch.isnan(st[k][:2]).all() and torch.isfinite(st[k][2:]).all()


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_last_row_group_and_classes_never_seen(dtype, tol, no_index_add):
    """C = 2, N = 600, D = 24: 19 row groups of the backward product with one stripe each, the class and filter rows at the
    end of the last group that has any; and the 37-class ragged input with n_classes = 40."""
    Xn, yn, dense = reference("few_long", cpo.few_long_classes)
    assert _native.point_backward_groups(600, 24) == 19
    check_input("few_long", Xn, yn, dense, dtype, tol, [5, 24])
    Xn, yn, dense = reference("ragged40", cso.ragged_small, n_classes=40)
    check_input("ragged40", Xn, yn, dense, dtype, tol, [4], n_classes=40)


# ---- exact symmetry, reproducibility ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name,make,K", [("tailsL65", lambda: cpo.tails_with_long_class(65), 17),
                                         ("tailsL65", lambda: cpo.tails_with_long_class(65), 64),
                                         ("few_long", cpo.few_long_classes, 24)])
def test_shrunk_outputs_symmetric_and_reproducible_bit_for_bit(name, make, K, dtype):
    Xn, yn, _ = reference(name, make)
    X, y = base.dev(Xn, yn, dtype)
    cp = ClassPoints(X, y, estimator="oas")
    F = torch.tensor(cpo.filters(K, Xn.shape[1]), dtype=dtype, device=DEV)
    A, b = (torch.tensor(t, dtype=dtype, device=DEV) for t in cpo.loss_terms(cp.n_classes, K, seed=3))
    runs = []
    for _ in range(2):
        zc, m, S, S2 = _native.class_feature_moments(cp, F, True, 0.25)
        partial = _native.class_feature_moments_backward(cp, zc, A, b, F)
        runs.append((zc, m, S, S2, partial))
    full = cp.counts >= 2
    for M in runs[0][2:4]:
        assert torch.isfinite(M[full]).all() and torch.equal(M[full], M[full].transpose(1, 2))
    for a, c in zip(*runs):
        assert torch.equal(nan_as(a), nan_as(c))
    assert torch.isfinite(runs[0][4]).all() and runs[0][4].abs().sum() > 0
    # the shrinkage is in there: not the empirical covariance
    plain = _native.class_feature_moments(ClassPoints(X, y), F, True, 0.25)[2]
    assert not torch.equal(plain[full], runs[0][2][full])


def test_backward_never_reads_what_it_skips():
    """NaN in G, keep and shift for the classes below two points and in g_means for the empty class: the same bits as zeros."""
    Xn, yn, _ = reference("tailsL17", lambda: cpo.tails_with_long_class(17))
    X, y = base.dev(Xn, yn, torch.float64)
    cp = ClassPoints(X, y, estimator="oas")
    assert torch.isnan(cp.shrink_keep[:2]).all() and torch.isnan(cp.shrink_shift[:2]).all()
    K = 5
    F = torch.tensor(cpo.filters(K, 17), device=DEV)
    A, b = (torch.tensor(t, device=DEV) for t in cpo.loss_terms(cp.n_classes, K, seed=3))
    zc = _native.class_feature_moments(cp, F, False, 0.0)[0]
    A[:2], b[0], cp.shrink_keep[:2], cp.shrink_shift[:2] = 0.0, 0.0, 0.0, 0.0
    clean = _native.class_feature_moments_backward(cp, zc, A, b, F)
    A[:2], b[0], cp.shrink_keep[:2], cp.shrink_shift[:2] = float("nan"), float("nan"), float("nan"), float("nan")
    assert torch.equal(clean, _native.class_feature_moments_backward(cp, zc, A, b, F)) and torch.isfinite(clean).all()
    # without the gradient of the means the class rows are zeros and the filter rows keep their place
    none = _native.class_feature_moments_backward(cp, zc, A, None, F)
    b[:] = 0.0
    assert torch.equal(none, _native.class_feature_moments_backward(cp, zc, A, b, F))


def test_one_dimension_propagates_nan_as_the_dense_statistics():
    """D = 1: tr2 = tr^2 and rho = 0 / 0 for every class, also those with two points and more; the dense OAS statistics are
    NaN there, and so are the shrunk feature covariances and dL/dF (the select leaves out the classes below two points only)."""
    Xn, yn = cso.tails(1)
    X, y = base.dev(Xn, yn, torch.float64)
    cp = ClassPoints(X, y, estimator="oas")
    assert torch.isnan(cp.shrinkage).all() and torch.isnan(cp.shrink_keep).all() and torch.isnan(cp.shrink_shift).all()
    assert torch.isnan(statistics.class_statistics(X, y, estimator="oas")["covariances"]).all()
    F = torch.ones(1, 1, dtype=torch.float64, device=DEV)
    zc, m, S, _ = _native.class_feature_moments(cp, F, False, 0.0)
    assert torch.isnan(S).all() and torch.isfinite(m[1:]).all()
    G, g = torch.ones(cp.n_classes, 1, 1, dtype=torch.float64, device=DEV), torch.ones(cp.n_classes, 1, dtype=torch.float64, device=DEV)
    assert torch.isnan(_native.class_feature_moments_backward(cp, zc, G, g, F).sum(dim=0)).all()


# ---- fallback -------------------------------------------------------------------------------------------------------------------

def test_switch_off_and_more_than_64_filters_take_the_torch_expression(monkeypatch):
    Xn, yn, dense = reference("tailsL100", lambda: cpo.tails_with_long_class(100))
    for dtype, tol in DTYPES:
        X, y = base.dev(Xn, yn, dtype)
        native = ClassPoints(X, y, estimator="oas")
        Fn = cpo.filters(65, 100)
        st = native.feature_statistics(torch.tensor(Fn, dtype=dtype, device=DEV), second_moments=True)   # 65 filters: torch
        cpo.check_values(st, cpo.feature_moments(Xn, yn, Fn, stats=dense), tol)
        with monkeypatch.context() as m:
            m.setattr(statistics, "NATIVE_CLASS_POINTS", False)
            m.setattr(_native, "class_shrinkage", None)                    # calling it would fail
            cp = ClassPoints(X, y, estimator="oas")
            Fn = cpo.filters(16, 100)
            F = torch.tensor(Fn, dtype=dtype, device=DEV)
            cpo.check_values(cp.feature_statistics(F, second_moments=True), cpo.feature_moments(Xn, yn, Fn, stats=dense), tol)
            A, b, g_ref, keep = reference_gradient("tailsL100", 16, True, seed=9)
            assert rel_err(base.loss_gradient(cp, F, A, b, keep, True).cpu().numpy(), g_ref) < tol
        full = cp.counts >= 2
        # float32: each side within 2e-5 x tr2 / (tr2 - tr^2 / D) of the oracle, and that factor is at most 8.3 on these inputs
        bound = 1e-11 if dtype == torch.float64 else 2 * 8.3 * 2e-5
        assert (cp.shrinkage[full] - native.shrinkage[full]).abs().max() < bound
        assert torch.isnan(cp.shrinkage[~full]).all()


# ---- models ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", base.VARIANTS)
@pytest.mark.parametrize("op", OAS_OPS)
def test_oas_points_closure_equals_dense_oas_closure(op, variant, no_index_add):
    """Loss and filter gradient of the fit's closure from ClassPoints(estimator="oas") against the dense OAS statistics:
    float64 within 1e-8; float32 within max(1e-5, 5 x the deviation of the dense float32 closure from the dense float64
    one).  The evaluator is the one the empirical points take."""
    Xn, yn = base.model_points()
    res = {}
    for dtype in (torch.float64, torch.float32):
        X, y = base.dev(Xn, yn, dtype)
        Wn = base.pair_weights(variant, dtype)
        for mode, data in (("dense", statistics.class_statistics(X, y, estimator="oas")),
                           ("points", ClassPoints(X, y, estimator="oas"))):
            res[mode, dtype] = base.closure(base.make(op, variant, dtype), data, Wn)
        assert res["points", dtype][2] == base.EVALUATOR[op]
    l64, g64, _ = res["dense", torch.float64]
    lp, gp, _ = res["points", torch.float64]
    print(f"oas {op} {variant} f64: loss {abs(lp - l64) / abs(l64):.2e} grad {rel_err(gp, g64):.2e}")
    assert abs(lp - l64) / abs(l64) < 1e-8 and rel_err(gp, g64) < 1e-8
    ld, gd, _ = res["dense", torch.float32]
    lp, gp, _ = res["points", torch.float32]
    dev_l, dev_g = abs(ld - l64) / abs(l64), rel_err(gd, g64)
    err_l, err_g = abs(lp - l64) / abs(l64), rel_err(gp, g64)
    print(f"oas {op} {variant} f32: loss {err_l:.2e} (dense {dev_l:.2e}) grad {err_g:.2e} (dense {dev_g:.2e})")
    assert err_l < max(1e-5, 5 * dev_l) and err_g < max(1e-5, 5 * dev_g)


def test_oas_points_fit_replays_its_graph_and_equals_the_eager_fit_bit_for_bit(monkeypatch):
    import sqfa_amd._optim as opt
    Xn, yn = base.model_points()
    X, y = base.dev(Xn, yn, torch.float64)
    monkeypatch.setattr(opt, "GRAPH_WARMUP_CLOSURES", 1)
    replays = [0]
    original_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays[0] += 1
        return original_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    runs = {}
    for use_graph in (False, True):
        monkeypatch.setattr(opt, "GRAPH_CLOSURE", use_graph)
        model = base.make("affine_invariant", "plain", torch.float64)
        loss, _ = model.fit(data_statistics=ClassPoints(X, y, estimator="oas"), max_epochs=4, show_progress=False,
                            return_loss=True)
        runs[use_graph] = loss
        if not use_graph:
            assert replays[0] == 0
    assert replays[0] >= 1, "the graph path was not taken"
    assert torch.equal(runs[True], runs[False])


# ---- nothing dense is formed ---------------------------------------------------------------------------------------------------

def test_an_oas_points_fit_forms_nothing_of_size_C_D_D(monkeypatch):
    """C = 64, D = 512, K = 8, N = 2048, float32 (one (C,D,D) tensor: 67 MB), the shape and the rule of
    test_a_points_fit_forms_nothing_of_size_C_D_D: over the construction of ClassPoints(estimator="oas") and a whole fit
    from it the peak of allocated memory rises by less than a quarter of one tensor beyond what the dense fit's closure
    itself needs, and that share is itself below the bound.  The coefficient pass: partials 36 KB, means workspace 128 KB."""
    C, D, K, N = 64, 512, 8, 2048
    one_tensor = C * D * D * 4
    rng = np.random.default_rng(21)
    yn = rng.permutation(np.arange(N) % C)
    Xn = (rng.standard_normal((N, D)) + 0.3 * rng.standard_normal((C, D))[yn]).astype(np.float32)
    X, y = torch.tensor(Xn, device=DEV), torch.tensor(yn, device=DEV)

    def fit_rise(data):
        torch.manual_seed(5)
        model = mc.make_model("smsqfa", D, K, 0.01, "sphere", torch.float32, DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, _ = model.fit(data_statistics=data(), max_epochs=3, show_progress=False, return_loss=True)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, loss

    dense = statistics.class_statistics(X, y, estimator="oas")["second_moments"]
    fit_rise(lambda: dense)
    closure_rise, dense_loss = fit_rise(lambda: dense)
    del dense
    assert closure_rise < one_tensor / 4

    def refuse(*a, **k):
        raise AssertionError("a dense statistic was formed")
    for owner, name in ((statistics, "class_statistics"), (model_module, "class_statistics"), (_native, "class_moments"),
                        (_native, "project_scatters"), (model_module, "conjugate_matrix"), (linalg, "conjugate_matrix")):
        monkeypatch.setattr(owner, name, refuse)
    rise, loss = fit_rise(lambda: ClassPoints(X, y, estimator="oas"))     # construction included
    print(f"peak rise: oas points fit {rise / 1e6:.2f} MB, dense closure {closure_rise / 1e6:.2f} MB, one (C,D,D) {one_tensor / 1e6:.1f} MB")
    assert rise - closure_rise < one_tensor / 4
    assert torch.isfinite(loss).all() and torch.isfinite(dense_loss).all() and len(loss) == len(dense_loss) == 3
