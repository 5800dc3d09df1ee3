"""CPU tests of the per-pair class weights (fit(pair_weights=W): loss = -sum_{i>j} W_ij D_ij / sum_{i>j} W_ij): the two new
C-ABI entry points (exported, bound, argument validation before any HIP call), the host-side validation of the weights, the
closure plan, and the plumbing from fit() down to the pair backend with the float64 oracle as the backend (C=5, D=6, K=2)."""
import ctypes
import os

import pytest
import torch

import sqfa_amd
from oracle_backend import oracle_pair_backend
from pair_weight_cases import make_weights, normalized, weighted_loss
from sqfa_amd import _lib, _native, distances

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
# fit() hands its loss record back as a float32 tensor: a float64 loss read from it carries one float32 rounding
# (relative 2^-24), on top of the 1e-9 the closure itself is held to
RECORD = 1e-9 + 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture
def oracle_backend(monkeypatch):
    def backend(A, B, metric="airm", **kw):
        return oracle_pair_backend(A, B, **kw)

    monkeypatch.setattr(_native, "_pair_backend", backend)


# ---------------------------------------------------------------------------------------------------------------
# C ABI


def test_symbols_exported_and_bound(lib):
    for name, n_args in (("sqfa_gauss_pairwise_loss_weighted", 17), ("sqfa_log_euclidean_pairwise_loss_weighted", 15)):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is ctypes.c_int
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        # the old signature with one pointer in front of uniform_weight
        old = _lib.PROTOTYPES[name[:-len("_weighted")]][1]
        pos = 7 if "gauss" in name else 6
        assert _lib.PROTOTYPES[name][1] == old[:pos] + [ctypes.c_void_p] + old[pos:]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "sqfa_gauss_pairwise_loss_weighted(" in header and "sqfa_log_euclidean_pairwise_loss_weighted(" in header
    assert "sqfa_gauss_pairwise_loss(" in header and "sqfa_log_euclidean_pairwise_loss(" in header
    assert "MUST BE SYMMETRIC" in header


def _gauss(lib, mu=1, cov=1, n=4, m=8, dtype=_lib.SQFA_F32, kind=0, W=1, gmu=1, gcov=1, ws=1, ws_bytes=1 << 24):
    return lib.sqfa_gauss_pairwise_loss_weighted(FAKE if mu else NULL, FAKE if cov else NULL, n, m, dtype, kind, 1e-6,
                                                 FAKE if W else NULL, -1.0, FAKE, FAKE if gmu else NULL,
                                                 FAKE if gcov else NULL, NULL, NULL, FAKE if ws else NULL, ws_bytes, NULL)


def _logeuc(lib, S=1, n=4, m=8, dtype=_lib.SQFA_F32, sqrt_mode=1, W=1, grad=1, ws=1, ws_bytes=1 << 24):
    return lib.sqfa_log_euclidean_pairwise_loss_weighted(FAKE if S else NULL, n, m, dtype, sqrt_mode, 1e-6,
                                                         FAKE if W else NULL, -1.0, FAKE, FAKE if grad else NULL, NULL, NULL,
                                                         FAKE if ws else NULL, ws_bytes, NULL)


@pytest.mark.parametrize("W", [0, 1])
def test_gauss_argument_validation(lib, W):
    assert _gauss(lib, W=W, mu=0) == -1
    assert _gauss(lib, W=W, cov=0) == -1
    assert _gauss(lib, W=W, n=1) == -1
    assert _gauss(lib, W=W, n=0) == -1
    assert _gauss(lib, W=W, m=0) == -1
    assert _gauss(lib, W=W, dtype=7) == -1
    assert _gauss(lib, W=W, kind=-1) == -1
    assert _gauss(lib, W=W, kind=4) == -1
    assert _gauss(lib, W=W, gmu=0) == -1               # exactly one of the two gradient outputs
    assert _gauss(lib, W=W, gcov=0) == -1
    assert _gauss(lib, W=W, m=65) == -2                # SQFA_ERR_UNSUPPORTED_M
    assert _gauss(lib, W=W, ws_bytes=16) == -3         # SQFA_ERR_WORKSPACE
    assert _gauss(lib, W=W, ws=0) == -3
    assert _gauss(lib, W=W, m=64, ws_bytes=16) == -3
    assert _gauss(lib, W=W, gmu=0, gcov=0, ws_bytes=16) == -3   # forward only passes the argument checks
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):       # the workspace query is the unweighted one
        need = lib.sqfa_gauss_pairwise_workspace_bytes(4, 8, dtype)
        assert _gauss(lib, W=W, dtype=dtype, ws_bytes=need - 1) == -3


@pytest.mark.parametrize("W", [0, 1])
def test_log_euclidean_argument_validation(lib, W):
    assert _logeuc(lib, W=W, S=0) == -1
    assert _logeuc(lib, W=W, n=1) == -1
    assert _logeuc(lib, W=W, n=0) == -1
    assert _logeuc(lib, W=W, m=0) == -1
    assert _logeuc(lib, W=W, dtype=7) == -1
    assert _logeuc(lib, W=W, dtype=-1) == -1
    assert _logeuc(lib, W=W, sqrt_mode=2) == -1
    assert _logeuc(lib, W=W, sqrt_mode=-1) == -1
    assert _logeuc(lib, W=W, m=65) == -2
    assert _logeuc(lib, W=W, m=128) == -2
    assert _logeuc(lib, W=W, ws_bytes=16) == -3
    assert _logeuc(lib, W=W, ws=0) == -3
    assert _logeuc(lib, W=W, m=64, ws_bytes=16) == -3
    assert _logeuc(lib, W=W, sqrt_mode=0, grad=0, ws_bytes=16) == -3
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):
        need = lib.sqfa_log_euclidean_workspace_bytes(4, 8, dtype)
        assert _logeuc(lib, W=W, dtype=dtype, ws_bytes=need - 1) == -3


def test_native_calls_refuse_cpu_tensors_with_weights():
    S = torch.eye(2, dtype=torch.float64).repeat(3, 1, 1)
    W = torch.ones(3, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.hip_log_euclidean_pairwise_loss(S, True, 1e-6, -0.1, pair_weights=W)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.hip_gauss_pairwise_loss(torch.zeros(3, 2, dtype=torch.float64), S, 0, 1e-6, -0.1, pair_weights=W)


# ---------------------------------------------------------------------------------------------------------------
# statistics and models of the host tests: C = 5, D = 6, K = 2, float64, CPU

C, D, K = 5, 6, 2


def _stats():
    g = torch.Generator().manual_seed(3)
    A = torch.randn(C, D, 4 * D, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2) / (4 * D) + 0.1 * torch.eye(D, dtype=torch.float64)
    cov = 0.5 * (cov + cov.transpose(1, 2))
    return {"means": 0.5 * torch.randn(C, D, generator=g, dtype=torch.float64), "covariances": cov}


def _model(kind, distance_fun=None, n_filters=K, constraint="sphere"):
    torch.manual_seed(11)
    cls = sqfa_amd.model.SQFA if kind == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    return cls(n_dim=D, n_filters=n_filters, feature_noise=0.01, distance_fun=distance_fun, constraint=constraint).double()


def _data(kind):
    stats = _stats()
    return stats if kind == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]


# ---------------------------------------------------------------------------------------------------------------
# validation, one condition at a time


def _fit(model, data, W, **kw):
    return model.fit(data_statistics=data, max_epochs=2, show_progress=False, return_loss=True, pair_weights=W, **kw)


@pytest.mark.parametrize("kind", ["smsqfa", "sqfa"])
def test_validation_of_the_weights(kind, oracle_backend):
    model, data = _model(kind), _data(kind)
    good = make_weights(C, 1)
    with pytest.raises(ValueError, match="shape"):
        _fit(model, data, good[:4, :4])
    with pytest.raises(ValueError, match="shape"):
        _fit(model, data, good[0])
    with pytest.raises(ValueError, match="shape"):
        _fit(model, data, torch.ones(C, C + 1, dtype=torch.float64))
    for bad_value in (float("nan"), float("inf")):
        bad = good.clone()
        bad[3, 1] = bad[1, 3] = bad_value
        with pytest.raises(ValueError, match="finite"):
            _fit(model, data, bad)
    bad = good.clone()
    bad[2, 0] = bad[0, 2] = -0.5
    with pytest.raises(ValueError, match="non-negative"):
        _fit(model, data, bad)
    bad = good.clone()
    bad[4, 1] = bad[4, 1] + 1e-12
    with pytest.raises(ValueError, match="symmetric"):
        _fit(model, data, bad)
    with pytest.raises(ValueError, match="positive sum"):
        _fit(model, data, torch.zeros(C, C, dtype=torch.float64))
    with pytest.raises(ValueError, match="positive sum"):
        _fit(model, data, torch.eye(C, dtype=torch.float64))   # the diagonal does not count
    assert model._pair_weights is None                          # nothing of a failed fit stays on the model
    # tensor-likes are accepted, the diagonal is ignored
    W = good.clone()
    W.fill_diagonal_(7.0)
    loss_a, _ = _fit(_model(kind), data, W.tolist())
    loss_b, _ = _fit(_model(kind), data, good.numpy())
    assert torch.equal(loss_a, loss_b)


def test_normalized_pair_weights():
    W = make_weights(C, 2)
    W.fill_diagonal_(3.0)
    Wn = _native.normalized_pair_weights(W, C, torch.float32, "cpu")
    assert Wn.dtype == torch.float32 and Wn.is_contiguous() and tuple(Wn.shape) == (C, C)
    assert torch.equal(Wn, normalized(W).float())
    assert bool((Wn.diagonal() == 0).all())
    assert abs(float(torch.tril(Wn.double(), -1).sum()) + 1.0) < 1e-6
    assert _native.normalized_pair_weights(None, C, torch.float32, "cpu") is None
    ones = _native.normalized_pair_weights(torch.ones(C, C), C, torch.float64, "cpu")
    assert torch.allclose(ones[1, 0], torch.tensor(-1.0 / (C * (C - 1) // 2), dtype=torch.float64), rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------
# the plan


def _record_plans(model, monkeypatch):
    plans = []
    original = model._closure_plan

    def recording(prepared=None, staged=False):
        plan = original(prepared, staged)
        if prepared is not None:
            plans.append(plan)
        return plan

    monkeypatch.setattr(model, "_closure_plan", recording)
    return plans


@pytest.mark.parametrize("kind", ["smsqfa", "sqfa"])
def test_fit_without_weights_takes_todays_plan(kind, oracle_backend, monkeypatch):
    model, data = _model(kind), _data(kind)
    today = model._closure_plan(model._prepare_statistics(data))
    assert today.pair_weights is None and today.evaluator == "chain" and today.weight == -1.0 / 10
    plans = _record_plans(model, monkeypatch)
    _fit(model, data, None)
    assert len(plans) > 0 and all(p == today for p in plans)
    # the eight-field construction still works and means "no weights"
    assert sqfa_amd.model.ClosurePlan(*today[:8]) == today
    # with weights: the same plan but for the weights, which are the normalised matrix; cleared after the fit
    W = make_weights(C, 5)
    plans.clear()
    _fit(model, data, W)
    assert len(plans) > 0
    for p in plans:
        assert p[:8] == today[:8] and torch.equal(p.pair_weights, normalized(W))
    assert all(p.pair_weights is plans[0].pair_weights for p in plans)    # one static tensor for the whole fit
    assert model._pair_weights is None


def test_lbfgs_keywords_still_fall_through(oracle_backend):
    model, data = _model("smsqfa"), _data("smsqfa")
    _fit(model, data, make_weights(C, 5), history_size=5)
    with pytest.raises(TypeError):
        _fit(model, data, make_weights(C, 5), no_such_lbfgs_option=1)


# ---------------------------------------------------------------------------------------------------------------
# plumbing: weighted closure loss and filter gradient against float64 autograd of -sum tril(W D) / sum tril(W)


def _reference(model, data, W):
    raw = model.parametrizations.filters.original
    raw.grad = None
    Dm = model.get_class_distances(data, regularized=True)
    loss = weighted_loss(W, Dm)
    (grad,) = torch.autograd.grad(loss, raw)
    return loss.detach(), grad


@pytest.mark.parametrize("kind,fn", [("smsqfa", "affine_invariant"), ("sqfa", "fisher_rao_lower_bound")])
@pytest.mark.parametrize("constraint", ["sphere", "none"])
def test_weighted_closure_matches_autograd(kind, fn, constraint, oracle_backend):
    model, data = _model(kind, getattr(distances, fn), constraint=constraint), _data(kind)
    W = make_weights(C, 7)
    ref_loss, ref_grad = _reference(model, data, W)
    uni_loss, _ = _reference(model, data, torch.ones(C, C, dtype=torch.float64))
    assert abs(float(ref_loss - uni_loss)) > 1e-3 * abs(float(uni_loss))      # the weights matter in this case
    prepared = model._prepare_statistics(data)
    raw = model.parametrizations.filters.original
    model._pair_weights = _native.normalized_pair_weights(W, C, raw.dtype, raw.device)
    try:
        plan = model._closure_plan(prepared)
        assert plan.evaluator == "chain" and plan.pair_weights is model._pair_weights
        raw.grad = None
        loss, flags = model._fused_closure_loss(prepared)
        loss.backward()
    finally:
        model._pair_weights = None
    assert flags.tolist() == [0, 0]
    assert abs(float(loss.detach() - ref_loss)) <= 1e-9 * abs(float(ref_loss))
    assert float((raw.grad - ref_grad).norm()) <= 1e-8 * float(ref_grad.norm())
    # the same through fit(): the loss recorded for the first epoch is the one at the initial filters
    losses, _ = _fit(model, data, W)
    assert abs(float(losses[0] - ref_loss)) <= RECORD * abs(float(ref_loss))
    assert losses[-1] < losses[0]
    # W = ones gives the present loss to rounding
    model2 = _model(kind, getattr(distances, fn), constraint=constraint)
    l_ones, _ = _fit(model2, data, torch.ones(C, C, dtype=torch.float64))
    model3 = _model(kind, getattr(distances, fn), constraint=constraint)
    l_none, _ = _fit(model3, data, None)
    assert abs(float(l_ones[0] - l_none[0])) <= RECORD * abs(float(l_none[0]))
    assert abs(float(l_none[0] - uni_loss)) <= RECORD * abs(float(uni_loss))


def test_generic_closure_takes_the_weights(oracle_backend):
    """A custom distance_fun has no fused closure: the fitting loop's own expression carries the weights."""
    fn = lambda A, B: distances.affine_invariant(A, B)   # noqa: E731
    model, data = _model("smsqfa", fn), _data("smsqfa")
    assert not model._has_fused_closure()
    W = make_weights(C, 9)
    ref_loss, _ = _reference(model, data, W)
    losses, _ = _fit(model, data, W)
    assert abs(float(losses[0] - ref_loss)) <= RECORD * abs(float(ref_loss))
    assert losses[-1] < losses[0]
    # and agrees with the fused closure of the same operator
    fused = _model("smsqfa", distances.affine_invariant)
    losses_fused, _ = _fit(fused, data, W)
    assert abs(float(losses_fused[0] - losses[0])) <= RECORD * abs(float(losses[0]))
    # torch-only operators on CPU tensors (log_euclidean declines its fused closure there)
    model = _model("smsqfa", distances.log_euclidean)
    ref_loss, _ = _reference(model, data, W)
    losses, _ = _fit(model, data, W)
    assert abs(float(losses[0] - ref_loss)) <= RECORD * abs(float(ref_loss))


def test_a_zero_weight_removes_the_pair(oracle_backend):
    """Only the weighted pair drives the loss: with one pair weighted, the loss is -D of that pair."""
    model, data = _model("smsqfa"), _data("smsqfa")
    W = torch.zeros(C, C, dtype=torch.float64)
    W[3, 1] = W[1, 3] = 2.5
    Dm = model.get_class_distances(data, regularized=True).detach()
    losses, _ = _fit(model, data, W)
    assert abs(float(losses[0] + Dm[3, 1])) <= RECORD * float(Dm[3, 1])


@pytest.mark.parametrize("kind", ["smsqfa", "sqfa"])
def test_pairwise_fit_with_weights(kind, oracle_backend):
    model, data = _model(kind, n_filters=4), _data(kind)
    W = make_weights(C, 13)
    losses, times = model.fit(data_statistics=data, max_epochs=4, show_progress=False, return_loss=True, pairwise=True,
                              pair_weights=W)
    assert torch.isfinite(losses).all() and losses[-1] < losses[0] and len(losses) == len(times)
    assert model._pair_weights is None
    # every stage used the weights: the first epoch of the first stage is the weighted loss of the first two filters
    ref_model = _model(kind, n_filters=4)
    first_two = _model(kind, n_filters=2)
    first_two._replace_filters(ref_model.filters.detach()[:2].clone())
    ref_loss, _ = _reference(first_two, data, W)
    assert abs(float(losses[0] - ref_loss)) <= RECORD * abs(float(ref_loss))
