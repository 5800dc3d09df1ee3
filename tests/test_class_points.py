"""CPU checks of the points mode: ClassPoints' torch expression against the float64 oracle tests/class_points_oracle.py
(values and gradient), its bookkeeping, the refusals, the argument checks of the C ABI (fake non-null pointers: nothing
is launched) and that statistics="dense" is the path of an omitted `statistics`."""
import ctypes

import numpy as np
import pytest
import torch

import class_points_oracle as cpo
import class_statistics_oracle as cso
import model_cases as mc
from conftest import rel_err
from sqfa_amd import _lib, _native, model as model_module, statistics
from sqfa_amd.statistics import ClassPoints

Z, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(4096)


# ---- the torch expression against the oracle -----------------------------------------------------------------------------

INPUTS = {"ragged_small": lambda: cso.ragged_small(), "tails17": lambda: cso.tails(17)}


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 2e-5)])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_torch_expression_against_the_oracle(name, dtype, tol):
    Xn, yn = INPUTS[name]()
    D, K = Xn.shape[1], 4
    Fn = cpo.filters(K, D)
    cp = ClassPoints(torch.tensor(Xn, dtype=dtype), torch.tensor(yn))
    C = cp.n_classes
    dense = cso.class_statistics(Xn, yn)
    F = torch.tensor(Fn, dtype=dtype, requires_grad=True)
    stats = cp.feature_statistics(F, second_moments=True)
    errs = cpo.check_values(stats, cpo.feature_moments(Xn, yn, Fn, stats=dense), tol, what=name)
    print(name, dtype, errs)
    assert rel_err(cp.means[cp.counts > 0].numpy(), dense["means"][cp.counts.numpy() > 0]) < tol
    A, b = cpo.loss_terms(C, K, seed=5)
    for second in (False, True):
        L_ref, g_ref, keep = cpo.loss_gradient(Xn, yn, Fn, A, b, second_moments=second, stats=dense)
        F.grad = None
        st = cp.feature_statistics(F, second_moments=second)
        S = st["second_moments" if second else "covariances"]
        kp = torch.tensor(keep)
        L = (torch.tensor(A, dtype=dtype)[kp] * S[kp]).sum() + (torch.tensor(b, dtype=dtype)[kp] * st["means"][kp]).sum()
        L.backward()
        assert rel_err(F.grad.numpy(), g_ref) < tol, (name, second)


def test_noise_goes_on_the_diagonal_only():
    Xn, yn = cso.ragged_small(C=5, D=7, empty=())
    cp = ClassPoints(torch.tensor(Xn), torch.tensor(yn))
    F = torch.tensor(cpo.filters(3, 7))
    a, b = cp.feature_statistics(F, second_moments=True), cp.feature_statistics(F, second_moments=True, noise=0.25)
    assert torch.equal(a["means"], b["means"])
    for k in ("covariances", "second_moments"):
        assert torch.allclose(b[k] - a[k], 0.25 * torch.eye(3, dtype=torch.float64).expand(5, 3, 3), atol=1e-14)


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------

def test_bookkeeping_float_labels_extra_classes_and_nan_pattern():
    Xn, yn = cso.tails(5)                       # class sizes 0, 1, 2, 3, 17, 70
    X = torch.tensor(Xn, dtype=torch.float32)
    cp = ClassPoints(X, torch.tensor(yn, dtype=torch.float32), n_classes=8)   # float labels; classes 6 and 7 never occur
    assert cp.n_classes == 8 and cp.n_dim == 5 and cp.points.data_ptr() == X.data_ptr()   # no copy of the points
    assert cp.counts.tolist() == cso.TAIL_SIZES + [0, 0]
    assert cp.class_start.tolist() == np.concatenate([[0], np.cumsum(cso.TAIL_SIZES + [0, 0])]).tolist()
    assert torch.equal(cp.row_class, torch.sort(torch.tensor(yn)).values)
    assert torch.equal(torch.tensor(yn)[cp.order], cp.row_class)
    empty = [0, 6, 7]
    assert torch.isnan(cp.means[empty]).all() and torch.isfinite(cp.means[1:6]).all()
    st = cp.feature_statistics(torch.tensor(cpo.filters(2, 5), dtype=torch.float32), second_moments=True)
    assert torch.isnan(st["means"][empty]).all() and torch.isfinite(st["means"][1:6]).all()
    for k in ("covariances", "second_moments"):
        assert torch.isnan(st[k][empty + [1]]).all() and torch.isfinite(st[k][2:6]).all()   # the singleton: NaN matrices
    dense = cp.class_statistics()
    assert dense["covariances"].shape == (8, 5, 5) and torch.isnan(dense["means"][empty]).all()
    assert torch.equal(dense["means"][1:6], statistics.class_statistics(X, torch.tensor(yn))["means"][1:6])
    # without n_classes the largest label decides
    assert ClassPoints(X, torch.tensor(yn)).n_classes == 6


def test_bad_inputs():
    X = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="labels must lie in"):
        ClassPoints(X, torch.tensor([0, 1, 2, 3]), n_classes=3)
    with pytest.raises(ValueError, match="shape"):
        ClassPoints(X, torch.tensor([0, 1, 2]))
    with pytest.raises(TypeError):
        ClassPoints(torch.zeros(4, 3, dtype=torch.int64), torch.tensor([0, 1, 2, 3]))
    assert "ClassPoints" in statistics.__all__


# ---- refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
def test_refusals(model_name):
    Xn, yn = cso.ragged_small(C=4, D=6, empty=(), lo=5, hi=9)
    X, y = torch.tensor(Xn, dtype=torch.float32), torch.tensor(yn)
    model = mc.make_model(model_name, 6, 2, 0.01, "sphere", torch.float32, "cpu")
    with pytest.raises(ValueError, match="empirical"):
        model.fit(X=X, y=y, statistics="points", estimator="oas", show_progress=False)
    with pytest.raises(ValueError, match="'dense' or 'points'"):
        model.fit(X=X, y=y, statistics="auto", show_progress=False)
    cp = ClassPoints(X, y)
    with pytest.raises(TypeError, match="X="):
        model.fit_pca(data_statistics=cp)
    model.class_shard = object()
    with pytest.raises(NotImplementedError, match="class_shard"):
        model.fit(X=X, y=y, statistics="points", show_progress=False)
    with pytest.raises(NotImplementedError, match="class_shard"):
        model.fit(data_statistics=cp, show_progress=False)


def test_models_accept_class_points_on_the_cpu():
    """The plan and the feature statistics of both models from a ClassPoints equal those from the dense dict (float64, CPU:
    the torch expression; distances that run on the CPU)."""
    from sqfa_amd import distances
    Xn, yn = cso.ragged_small(C=5, D=8, empty=(), lo=10, hi=20)
    X, y = torch.tensor(Xn), torch.tensor(yn)
    cp, dense = ClassPoints(X, y), statistics.class_statistics(X, y)
    sm = mc.make_model("smsqfa", 8, 3, 0.01, "sphere", torch.float64, "cpu")
    sq = mc.make_model("sqfa", 8, 3, 0.01, "sphere", torch.float64, "cpu")
    assert rel_err(sm._feature_scatters(cp, True).detach(), sm._feature_scatters(dense, True).detach()) < 1e-12
    a, b = sq._feature_statistics(cp, True), sq._feature_statistics(dense, True)
    assert rel_err(a["means"].detach(), b["means"].detach()) < 1e-12
    assert rel_err(a["covariances"].detach(), b["covariances"].detach()) < 1e-12
    for m in (sm, sq):
        assert m._n_classes_total(cp) == 5 and m._prepare_statistics(cp) is cp
        assert m._closure_plan(cp).evaluator == "chain" and m._single_node_inputs(cp) is None
    sq.distance_fun = distances.bhattacharyya
    assert sq._closure_plan(cp) is None           # CPU points: the generic closure
    assert rel_err(sq.get_class_distances(cp).detach(), sq.get_class_distances(dense).detach()) < 1e-10
    sq.fit(data_statistics=cp, max_epochs=1, show_progress=False)   # the generic closure runs on the CPU


# ---- dense stays the default ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
def test_dense_and_an_omitted_statistics_take_the_same_path(model_name, monkeypatch):
    calls = []

    class Stop(Exception):
        pass

    def spy(X, y, estimator="empirical"):
        calls.append(estimator)
        raise Stop

    monkeypatch.setattr(model_module, "class_statistics", spy)
    monkeypatch.setattr(model_module, "ClassPoints", None)     # building one would fail
    X, y = torch.zeros(6, 4), torch.tensor([0, 0, 0, 1, 1, 1])
    model = mc.make_model(model_name, 4, 2, 0.01, "sphere", torch.float32, "cpu")
    for kw in ({}, {"statistics": "dense"}, {"statistics": "dense", "estimator": "oas"}):
        with pytest.raises(Stop):
            model.fit(X=X, y=y, show_progress=False, **kw)
    assert calls == ["empirical", "empirical", "oas"]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def means(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_means(g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("class_start", FAKE),
                                        g("C", 3), g("dtype", 0), g("means", FAKE), Z)


def forward(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_feature_moments(
        g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("row_class", FAKE), g("class_start", FAKE), g("C", 3),
        g("means", FAKE), g("F", FAKE), g("K", 2), g("dtype", 0), 0.0, g("zc", FAKE), g("means_f", FAKE), g("cov_f", FAKE),
        g("second_f", Z), g("ws", FAKE), g("nbytes", 1 << 30), Z)


def backward(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_feature_moments_backward(
        g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("row_class", FAKE), g("class_start", FAKE), g("C", 3),
        g("means", FAKE), g("zc", FAKE), g("G", FAKE), g("ldg", 2), g("g_means", Z), g("K", 2), g("dtype", 0),
        g("n_groups", 4), g("partial", FAKE), g("ws", FAKE), g("nbytes", 1 << 30), Z)


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(dtype):
    query = _lib.load().sqfa_class_feature_moments_workspace_bytes
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for N, C, D, K in ((1, 1, 1, 1), (222, 7, 17, 16), (60000, 1000, 784, 16), (60000, 1000, 2048, 32), (50000, 100, 3072, 64),
                       (60000, 10, 784, 16), (1 << 32, 10, 3, 2)):
        nbytes = query(N, C, D, K, dtype)
        assert nbytes >= (N + C) * K * esz and nbytes >= C * K * K * esz    # the backward weights; one Gram per class
        assert nbytes <= max((N + C) * K, 32 * C * K * K) * esz + 16        # never anything of size D
    assert query(10, 3, 5, 65, dtype) == 0                                  # K > 64
    assert query(10, 3, 5, 2, 7) == 0                                       # bad dtype
    assert query(-1, 3, 5, 2, dtype) == 0 and query(10, 0, 5, 2, dtype) == 0
    assert query(10, 3, 0, 2, dtype) == 0 and query(10, 3, 5, 0, dtype) == 0
    assert query(10, 1 << 20, 5, 2, dtype) == 0                             # beyond the grid limits
    assert query(0, 3, 5, 2, dtype) > 0                                     # no point at all is a valid shape


def test_class_means_argument_checks():
    for bad in (dict(points=Z), dict(class_start=Z), dict(means=Z), dict(N=-1), dict(C=0), dict(D=0), dict(dtype=2),
                dict(dtype=-1)):
        assert means(**bad) == -1, bad
    assert means(C=1 << 20) == -2
    assert means(C=1 << 20, dtype=5) == -1


def test_feature_moments_argument_checks():
    for bad in (dict(points=Z), dict(row_class=Z), dict(class_start=Z), dict(means=Z), dict(F=Z), dict(zc=Z), dict(means_f=Z),
                dict(cov_f=Z), dict(N=-1), dict(C=0), dict(D=0), dict(K=0), dict(dtype=2), dict(dtype=-1)):
        assert forward(**bad) == -1, bad
    assert forward(K=65) == -2 and forward(C=1 << 20) == -2
    assert forward(ws=Z) == -3 and forward(nbytes=8) == -3
    # in this order: a bad argument wins over an unsupported shape, which wins over a short workspace
    assert forward(dtype=9, K=65, ws=Z) == -1 and forward(F=Z, nbytes=8) == -1 and forward(K=65, ws=Z) == -2


def test_feature_moments_backward_argument_checks():
    for bad in (dict(points=Z), dict(row_class=Z), dict(class_start=Z), dict(means=Z), dict(zc=Z), dict(G=Z), dict(partial=Z),
                dict(N=-1), dict(C=0), dict(D=0), dict(K=0), dict(ldg=1), dict(n_groups=0), dict(dtype=2)):
        assert backward(**bad) == -1, bad
    assert backward(K=65, ldg=65) == -2 and backward(C=1 << 20) == -2
    assert backward(ws=Z) == -3 and backward(nbytes=8) == -3
    assert backward(dtype=9, K=65, ldg=65, ws=Z) == -1 and backward(K=65, ldg=65, ws=Z) == -2


def test_backward_groups_fill_the_chip_and_stay_small():
    """groups x 64-column stripes: about four workgroups per CU at the c3 and c5 shapes, partial sums of a few MB."""
    for N, D, K in ((60000, 784, 16), (50000, 3072, 16), (60000, 2048, 32)):
        groups = _native.point_backward_groups(N, D)
        assert 512 <= groups * -(-D // 64) <= 1100 and groups * K * D * 4 <= 10 << 20
    assert _native.point_backward_groups(10, 5) == 1 and _native.point_backward_groups(2048, 512) == 64
