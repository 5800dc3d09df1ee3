"""GPU tests of the points mode (sqfa_class_means, sqfa_class_feature_moments, sqfa_class_feature_moments_backward,
statistics.ClassPoints, fit(statistics="points")) against the float64 oracle tests/class_points_oracle.py.
Bounds: the project's own for class statistics (tests/test_gpu_class_statistics.py), rel_err < 1e-11 in float64 and
< 2e-5 in float32, on values and on dL/dF; model level: the project's float64 gradient bound 1e-8 and the README's float32
rule.  Shapes are the smallest at which each mechanism can go wrong: the projection kernel takes 64 grouped rows per
workgroup and 64 (float32) / 32 (float64) columns per chunk, the backward product 32 rows per chunk and 64 columns per
stripe, 16 filters make one MFMA block."""
import numpy as np
import pytest
import torch

import class_points_oracle as cpo
import class_statistics_oracle as cso
import model_cases as mc
from conftest import rel_err
from sqfa_amd import _native, distances, linalg, model as model_module, statistics, transport
from sqfa_amd.statistics import ClassPoints

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-5)]
KS = [1, 2, 15, 16, 17, 33, 64]


@pytest.fixture
def no_index_add(monkeypatch):
    """The torch expression's index_add raises: whatever passes ran the native kernels."""
    def refuse(*a, **k):
        raise AssertionError("index_add called: the torch path ran")
    monkeypatch.setattr(torch, "index_add", refuse)
    monkeypatch.setattr(torch.Tensor, "index_add_", refuse)


_refs, _grads = {}, {}


def reference(name, make, n_classes=None):
    """(X, y, dense float64 oracle statistics) of a named input, computed once per session and shared."""
    if name not in _refs:
        X, y = make()
        _refs[name] = (X, y, cso.class_statistics(X, y, n_classes=n_classes))
    return _refs[name]


def reference_gradient(name, K, second, seed):
    """(A, b, dL/dF, keep) of the oracle loss on the named input and cpo.filters(K, D), once per session."""
    key = (name, K, second, seed)
    if key not in _grads:
        X, y, dense = _refs[name]
        A, b = cpo.loss_terms(dense["means"].shape[0], K, seed)
        _, g, keep = cpo.loss_gradient(X, y, cpo.filters(K, X.shape[1]), A, b, second_moments=second, stats=dense)
        _grads[key] = (A, b, g, keep)
    return _grads[key]


def dev(X, y, dtype):
    return torch.tensor(X, dtype=dtype, device=DEV), torch.tensor(y, device=DEV)


def loss_gradient(cp, F, A, b, keep, second):
    """dL/dF of the oracle's loss through ClassPoints.feature_statistics."""
    F = F.detach().clone().requires_grad_(True)
    st = cp.feature_statistics(F, second_moments=second)
    S = st["second_moments" if second else "covariances"]
    kp = torch.tensor(keep, device=DEV)
    L = (torch.tensor(A, dtype=F.dtype, device=DEV)[kp] * S[kp]).sum() + (torch.tensor(b, dtype=F.dtype, device=DEV)[kp] * st["means"][kp]).sum()
    L.backward()
    return F.grad


def check_input(name, Xn, yn, dense, dtype, tol, Ks, n_classes=None):
    X, y = dev(Xn, yn, dtype)
    cp = ClassPoints(X, y, n_classes=n_classes)
    D = Xn.shape[1]
    for K in Ks:
        Fn = cpo.filters(K, D)
        F = torch.tensor(Fn, dtype=dtype, device=DEV)
        st = cp.feature_statistics(F, second_moments=True)
        errs = cpo.check_values(st, cpo.feature_moments(Xn, yn, Fn, stats=dense), tol, what=(name, K))
        gerr = []
        for second in (False, True):
            A, b, g_ref, keep = reference_gradient(name, K, second, seed=7 * D + K)
            g = loss_gradient(cp, F, A, b, keep, second)
            gerr.append(rel_err(g.cpu().numpy(), g_ref))
        print(f"{name} K={K} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", grad {gerr[0]:.2e} / {gerr[1]:.2e}")
        assert max(gerr) < tol, (name, K, gerr)
    return cp


# ---- column and row tails, empty, singleton and ragged classes ----------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 5, 17, 63, 65, 100, 132])
def test_column_and_row_tails(D, dtype, tol, no_index_add):
    """Classes of 0, 1, 2, 3, 17, 70 and 129 points (longer than two row blocks and two row ranges), every filter-block
    count and its tails, capped at D.  D = 100 and 132 take the 16-byte loads, the others one element per load; 65, 100 and
    132 have several column chunks and stripes, the last one partial."""
    name = f"tailsL{D}"
    Xn, yn, dense = reference(name, lambda: cpo.tails_with_long_class(D))
    cp = check_input(name, Xn, yn, dense, dtype, tol, sorted({min(K, D) for K in KS}))
    # the NaN pattern: the empty class everywhere, the singleton in its matrices only
    st = cp.feature_statistics(torch.tensor(cpo.filters(1, D), dtype=dtype, device=DEV), second_moments=True)
    assert torch.isnan(st["means"][0]).all() and torch.isfinite(st["means"][1:]).all()
    for k in ("covariances", "second_moments"):
        assert torch.isnan(st[k][:2]).all() and torch.isfinite(st[k][2:]).all()


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_classes_split_over_workgroups_and_classes_never_seen(dtype, tol, no_index_add):
    """C = 2, N = 600: the Gram kernel splits each class into five shares, combined in a fixed order; and the 37-class ragged
    input with n_classes = 40 (three labels never occur, two more classes are empty)."""
    Xn, yn, dense = reference("few_long", cpo.few_long_classes)
    check_input("few_long", Xn, yn, dense, dtype, tol, [5, 24])
    Xn, yn, dense = reference("ragged40", cso.ragged_small, n_classes=40)
    check_input("ragged40", Xn, yn, dense, dtype, tol, [4], n_classes=40)


# ---- centring before the product ------------------------------------------------------------------------------------------------

def test_class_means_a_hundred_standard_deviations_out_f32(no_index_add):
    """Centring after the projection, or sum z z^T - n zbar zbar^T, loses about four digits of the covariance here."""
    Xn, yn, dense = reference("far", cso.far_means)
    X, y = dev(Xn, yn, torch.float32)
    Fn = cpo.filters(4, 20)
    st = ClassPoints(X, y).feature_statistics(torch.tensor(Fn, dtype=torch.float32, device=DEV), second_moments=True)
    errs = cpo.check_values(st, cpo.feature_moments(Xn, yn, Fn, stats=dense), 2e-5, what="far")
    print("far means:", errs)


# ---- exact symmetry, reproducibility --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name,make,K", [("tailsL65", lambda: cpo.tails_with_long_class(65), 17),
                                         ("tailsL65", lambda: cpo.tails_with_long_class(65), 64),
                                         ("few_long", cpo.few_long_classes, 24)])
def test_symmetric_and_reproducible_bit_for_bit(name, make, K, dtype):
    Xn, yn, dense = reference(name, make)
    X, y = dev(Xn, yn, dtype)
    cp = ClassPoints(X, y)
    F = torch.tensor(cpo.filters(K, Xn.shape[1]), dtype=dtype, device=DEV)
    A, b = (torch.tensor(t, dtype=dtype, device=DEV) for t in cpo.loss_terms(cp.n_classes, K, seed=3))
    runs = []
    for _ in range(2):
        zc, m, S, S2 = _native.class_feature_moments(cp, F, True, 0.25)
        partial = _native.class_feature_moments_backward(cp, zc, A, b)
        runs.append((zc, m, S, S2, partial))
    full = cp.counts >= 2
    for M in runs[0][2:4]:
        assert torch.isfinite(M[full]).all() and torch.equal(M[full], M[full].transpose(1, 2))
    for a, c in zip(*runs):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(c, nan=-7.0))
    assert torch.isfinite(runs[0][4]).all() and runs[0][4].abs().sum() > 0


def test_backward_never_reads_what_it_skips():
    """NaN in G for the classes below two points and in g_means for the empty class: the same bits as zeros there."""
    Xn, yn, _ = reference("tailsL17", lambda: cpo.tails_with_long_class(17))
    X, y = dev(Xn, yn, torch.float64)
    cp = ClassPoints(X, y)
    K = 5
    F = torch.tensor(cpo.filters(K, 17), device=DEV)
    A, b = (torch.tensor(t, device=DEV) for t in cpo.loss_terms(cp.n_classes, K, seed=3))
    A[:2], b[0] = 0.0, 0.0
    zc = _native.class_feature_moments(cp, F, False, 0.0)[0]
    clean = _native.class_feature_moments_backward(cp, zc, A, b)
    A[:2], b[0] = float("nan"), float("nan")
    assert torch.equal(clean, _native.class_feature_moments_backward(cp, zc, A, b)) and torch.isfinite(clean).all()


# ---- gather and alignment ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [17, 100])
def test_gather_grouped_and_unaligned_views_agree_bitwise(D, dtype):
    """Shuffled rows through `order`, the same rows grouped on the host with row_index NULL, the points as a view offset by
    one element (an unaligned base: one element per load) and unaligned filters: the same bits, values and gradient."""
    Xn, yn, _ = reference(f"tailsL{D}", lambda: cpo.tails_with_long_class(D))
    X, y = dev(Xn, yn, dtype)
    K = 16

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view_as(t)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0 and view.is_contiguous()
        return view

    F = torch.tensor(cpo.filters(K, D), dtype=dtype, device=DEV)
    base = ClassPoints(X, y)
    grouped = ClassPoints(X[base.order].contiguous(), base.row_class)
    grouped.order = None                                   # row_index NULL: the rows are already grouped
    A, b = (torch.tensor(t, dtype=dtype, device=DEV) for t in cpo.loss_terms(base.n_classes, K, seed=3))

    def run(cp, filters):
        zc, m, S, S2 = _native.class_feature_moments(cp, filters, True, 0.0)
        return zc, m, S, S2, _native.class_feature_moments_backward(cp, zc, A, b)

    want = run(base, F)
    for what, cp, filters in (("grouped", grouped, F), ("unaligned points", ClassPoints(shifted(X), y), F),
                              ("unaligned filters", base, shifted(F))):
        assert torch.equal(torch.nan_to_num(cp.means, nan=-7.0), torch.nan_to_num(base.means, nan=-7.0)), what
        for a, c in zip(want, run(cp, filters)):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(c, nan=-7.0)), what


# ---- means, switch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_means_equal_the_class_statistics_means(dtype, no_index_add):
    Xn, yn, _ = reference("tailsL100", lambda: cpo.tails_with_long_class(100))
    X, y = dev(Xn, yn, dtype)
    a, b = ClassPoints(X, y).means, statistics.class_statistics(X, y)["means"]
    assert torch.isnan(a[0]).all() and torch.equal(a[1:], b[1:]) and torch.isnan(b[0]).all()
    Xn, yn, _ = reference("ragged37", cso.ragged_small)
    X, y = dev(Xn, yn, dtype)
    assert torch.equal(torch.nan_to_num(ClassPoints(X, y).means, nan=-7.0),
                       torch.nan_to_num(statistics.class_statistics(X, y)["means"], nan=-7.0))


def test_switch_off_keeps_the_torch_expression(monkeypatch, no_index_add):
    Xn, yn, dense = reference("tailsL17", lambda: cpo.tails_with_long_class(17))
    X, y = dev(Xn, yn, torch.float64)
    F = torch.tensor(cpo.filters(4, 17), device=DEV)
    cp = ClassPoints(X, y)
    cp.feature_statistics(F)                              # native: the patch does not fire
    monkeypatch.setattr(statistics, "NATIVE_CLASS_POINTS", False)
    with pytest.raises(AssertionError, match="torch path ran"):
        cp.feature_statistics(F)
    with pytest.raises(AssertionError, match="torch path ran"):
        ClassPoints(X, y)


def test_more_than_64_filters_take_the_torch_expression():
    Xn, yn, dense = reference("tailsL100", lambda: cpo.tails_with_long_class(100))
    X, y = dev(Xn, yn, torch.float64)
    Fn = cpo.filters(65, 100)
    st = ClassPoints(X, y).feature_statistics(torch.tensor(Fn, device=DEV), second_moments=True)
    cpo.check_values(st, cpo.feature_moments(Xn, yn, Fn, stats=dense), 1e-11)


# ---- models --------------------------------------------------------------------------------------------------------------------------

MC, MD, MK = 8, 24, 4
OPS = {"affine_invariant": ("smsqfa", distances.affine_invariant), "log_euclidean": ("smsqfa", distances.log_euclidean),
       "bures_wasserstein": ("smsqfa", transport.bures_wasserstein),
       "fisher_rao_lower_bound": ("sqfa", distances.fisher_rao_lower_bound), "bhattacharyya": ("sqfa", distances.bhattacharyya)}
EVALUATOR = {"affine_invariant": "chain", "bures_wasserstein": "chain", "fisher_rao_lower_bound": "chain",
             "log_euclidean": "log_euclidean", "bhattacharyya": "gauss"}
VARIANTS = ["plain", "pair_weights", "orthogonal"]


def model_points():
    return reference("model", lambda: cso.ragged_small(C=MC, D=MD, empty=(), lo=30, hi=60))[:2]


def make(op, variant, dtype, seed=3):
    """The model of a case; float32 start values (filters, noise, the orthogonal map's base) whatever the dtype, so that
    the float32 and float64 models of a case are the same model."""
    kind, fn = OPS[op]
    torch.manual_seed(seed)
    model = mc.make_model(kind, MD, MK, 0.01, "orthogonal" if variant == "orthogonal" else "sphere", torch.float32, "cpu")
    model = (model.double() if dtype == torch.float64 else model).to(DEV)
    model.distance_fun = fn
    if variant == "orthogonal":
        par = model.parametrizations.filters[0]
        par.base = par.base.contiguous()
    return model


def pair_weights(variant, dtype):
    if variant != "pair_weights":
        return None
    W = torch.rand(MC, MC, generator=torch.Generator().manual_seed(11), dtype=torch.float64) + 0.1
    return _native.normalized_pair_weights(W + W.T, MC, dtype, DEV)


def closure(model, data, Wn):
    """One closure evaluation as the fitting loop does it: (loss, gradient of the raw parameter, evaluator)."""
    prepared = model._prepare_statistics(data)
    model.zero_grad()
    model._pair_weights = Wn
    try:
        plan = model._closure_plan(prepared)
        loss, flags = model._fused_closure_loss(prepared)
        assert flags.tolist() == [0, 0]
        loss.backward()
    finally:
        model._pair_weights = None
    (param,) = list(model.parameters())
    return float(loss.detach()), param.grad.detach().cpu().numpy().copy(), plan.evaluator


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("op", sorted(OPS))
def test_points_closure_equals_dense_closure(op, variant, no_index_add):
    """Loss and filter gradient of the fit's closure from the points against the dense statistics: float64 within the
    project's gradient bound 1e-8; float32 within max(1e-5, 5 x the deviation of the dense float32 closure from the dense
    float64 one)."""
    Xn, yn = model_points()
    res = {}
    for dtype in (torch.float64, torch.float32):
        X, y = dev(Xn, yn, dtype)
        Wn = pair_weights(variant, dtype)
        for mode, data in (("dense", statistics.class_statistics(X, y)), ("points", ClassPoints(X, y))):
            res[mode, dtype] = closure(make(op, variant, dtype), data, Wn)
        assert res["points", dtype][2] == EVALUATOR[op]
    l64, g64, _ = res["dense", torch.float64]
    lp, gp, _ = res["points", torch.float64]
    print(f"{op} {variant} f64: loss {abs(lp - l64) / abs(l64):.2e} grad {rel_err(gp, g64):.2e}")
    assert abs(lp - l64) / abs(l64) < 1e-8 and rel_err(gp, g64) < 1e-8
    ld, gd, _ = res["dense", torch.float32]
    lp, gp, _ = res["points", torch.float32]
    dev_l, dev_g = abs(ld - l64) / abs(l64), rel_err(gd, g64)
    err_l, err_g = abs(lp - l64) / abs(l64), rel_err(gp, g64)
    print(f"{op} {variant} f32: loss {err_l:.2e} (dense {dev_l:.2e}) grad {err_g:.2e} (dense {dev_g:.2e})")
    assert err_l < max(1e-5, 5 * dev_l) and err_g < max(1e-5, 5 * dev_g)


@pytest.mark.parametrize("op", sorted(OPS))
def test_class_distances_from_points(op):
    Xn, yn = model_points()
    X, y = dev(Xn, yn, torch.float64)
    model = make(op, "plain", torch.float64)
    with torch.no_grad():
        for reg in (False, True):
            a = model.get_class_distances(ClassPoints(X, y), regularized=reg)
            b = model.get_class_distances(statistics.class_statistics(X, y), regularized=reg)
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-8


@pytest.mark.parametrize("kind,pairwise", [("smsqfa", False), ("sqfa", False), ("smsqfa", True)])
def test_short_fit_from_points_follows_the_dense_fit(kind, pairwise):
    """3 epochs from the same start, float64: filters within 1e-5, loss histories within 1e-8; pairwise=True holds the
    first pair with FixedFilters while it learns the second (K = 4)."""
    Xn, yn = model_points()
    X, y = dev(Xn, yn, torch.float64)
    runs = {}
    for mode in ("dense", "points"):
        torch.manual_seed(5)
        model = mc.make_model(kind, MD, MK, 0.01, "sphere", torch.float64, DEV)
        loss, _ = model.fit(X=X, y=y, statistics=mode, max_epochs=3, show_progress=False, return_loss=True, pairwise=pairwise)
        runs[mode] = (loss.numpy(), model.filters.detach().cpu().numpy())
    assert len(runs["points"][0]) == (6 if pairwise else 3)
    assert np.abs(runs["points"][0] - runs["dense"][0]).max() < 1e-8
    assert rel_err(runs["points"][1], runs["dense"][1]) < 1e-5


# ---- nothing dense is formed ----------------------------------------------------------------------------------------------------------

def test_a_points_fit_forms_nothing_of_size_C_D_D(monkeypatch):
    """C = 64, D = 512, K = 8, N = 2048, float32: one (C,D,D) tensor is 67 MB.  Over a whole points fit the peak of
    allocated memory rises by less than a quarter of that beyond what the dense fit's closure itself needs (the pair
    workspaces, measured on a dense fit from ready statistics; that share must itself stay below the bound, or subtracting
    it would prove nothing): centred features 64 KB, partial sums 1 MB, means 128 KB."""
    C, D, K, N = 64, 512, 8, 2048
    one_tensor = C * D * D * 4
    rng = np.random.default_rng(21)
    yn = rng.permutation(np.arange(N) % C)
    Xn = (rng.standard_normal((N, D)) + 0.3 * rng.standard_normal((C, D))[yn]).astype(np.float32)
    X, y = torch.tensor(Xn, device=DEV), torch.tensor(yn, device=DEV)

    def fit_rise(**kw):
        torch.manual_seed(5)
        model = mc.make_model("smsqfa", D, K, 0.01, "sphere", torch.float32, DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss, _ = model.fit(max_epochs=3, show_progress=False, return_loss=True, **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, loss

    # the dense fit twice from the same tensor: the first one also checks the symmetry of the (C,D,D) statistics (temporaries
    # of their size); the second one allocates what a closure itself needs
    dense = statistics.class_statistics(X, y)["second_moments"]
    fit_rise(data_statistics=dense)
    closure_rise, dense_loss = fit_rise(data_statistics=dense)
    del dense
    assert closure_rise < one_tensor / 4

    def refuse(*a, **k):
        raise AssertionError("a dense statistic was formed")
    for owner, name in ((statistics, "class_statistics"), (model_module, "class_statistics"), (_native, "class_moments"),
                        (_native, "project_scatters"), (model_module, "conjugate_matrix"), (linalg, "conjugate_matrix")):
        monkeypatch.setattr(owner, name, refuse)
    rise, loss = fit_rise(X=X, y=y, statistics="points")
    print(f"peak rise: points fit {rise / 1e6:.2f} MB, dense closure {closure_rise / 1e6:.2f} MB, one (C,D,D) {one_tensor / 1e6:.1f} MB")
    assert rise - closure_rise < one_tensor / 4
    assert torch.isfinite(loss).all() and torch.isfinite(dense_loss).all() and len(loss) == len(dense_loss) == 3


# ---- graph ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["affine_invariant", "bhattacharyya", "log_euclidean"])
def test_points_fit_replays_its_graph_and_equals_the_eager_fit_bit_for_bit(op, monkeypatch):
    import sqfa_amd._optim as opt
    Xn, yn = model_points()
    X, y = dev(Xn, yn, torch.float64)
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
        model = make(op, "plain", torch.float64)
        loss, _ = model.fit(X=X, y=y, statistics="points", max_epochs=4, show_progress=False, return_loss=True)
        runs[use_graph] = loss
        if not use_graph:
            assert replays[0] == 0
    assert replays[0] >= 1, "the graph path was not taken"
    assert torch.equal(runs[True], runs[False])
