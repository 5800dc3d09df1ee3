"""GPU tests of the native orthogonal constraint (sqfa_orthogonal_forward / _backward, _native.OrthogonalFilters,
constraints.Orthogonal): kernel parity with torch's _Orthogonal, the golden closures and fits with torch's
householder_product made to raise, the single-node and graph-captured closures, and the NATIVE_ORTHOGONAL switch."""
import gc

import numpy as np
import pytest
import torch

import model_cases as mc
import orthogonal_oracle as oo
from conftest import rel_err
from sqfa_amd._optim import _no_gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# one reflector; the golden's shape; both sides of the 16 / 32 / 64 boundaries; K = 64 with few rows below the triangle;
# D spanning several row blocks with a ragged last one; the c3 filter shape
SHAPES = [(1, 4), (3, 8), (16, 64), (17, 68), (33, 132), (64, 68), (64, 256), (5, 1040), (16, 784)]
_reference = {}


def _case(K, D, signs):
    """Inputs and the CPU float64 / float32 results of torch's own parametrization, computed once per case."""
    key = (K, D, signs)
    if key not in _reference:
        X, base, R = oo.make_case(K, D, signs)
        _reference[key] = (X, base, R, oo.torch_reference(X, base, R, torch.float64), oo.torch_reference(X, base, R, torch.float32))
    return _reference[key]


def _native_result(X, base, R, dtype):
    from sqfa_amd import _native
    Xt = torch.tensor(X, dtype=dtype, device=DEV, requires_grad=True)
    Bt = torch.tensor(base, dtype=dtype, device=DEV)
    assert _native.orthogonal_supported(Xt, Bt)
    F = _native.OrthogonalFilters.apply(Xt, Bt)
    (F * torch.tensor(R, dtype=dtype, device=DEV)).sum().backward()
    return F.detach().cpu().numpy(), Xt.grad.cpu().numpy()


@pytest.fixture
def no_householder_product(monkeypatch):
    """torch's own Householder map raises on GPU tensors: whatever passes under this fixture ran the native kernels.
    (CPU calls pass through: registering the parametrization orthogonalises the initial filters with it on the host,
    torch's right_inverse, before the model moves to the device.)"""
    original = torch.linalg.householder_product

    def refuse(A, *a, **k):
        if A.is_cuda:
            raise AssertionError("torch.linalg.householder_product was called: the native orthogonal map was not taken")
        return original(A, *a, **k)
    monkeypatch.setattr(torch.linalg, "householder_product", refuse)


@pytest.mark.parametrize("signs", oo.SIGNS)
@pytest.mark.parametrize("K,D", SHAPES)
def test_kernels_match_torch_f64(K, D, signs, record_property):
    X, base, R, (F_ref, g_ref), _ = _case(K, D, signs)
    F, g = _native_result(X, base, R, torch.float64)
    err_f, err_g = rel_err(F, F_ref), rel_err(g, g_ref)
    record_property("forward_rel_err", err_f)
    record_property("grad_rel_err", err_g)
    print(f"orthogonal f64 K={K} D={D} {signs}: forward {err_f:.2e}, gradient {err_g:.2e}")
    assert err_f <= 1e-12 and err_g <= 1e-10
    assert (g[np.tril_indices(K, 0, D)] == 0).all()
    F2, g2 = _native_result(X, base, R, torch.float64)
    assert np.array_equal(F, F2) and np.array_equal(g, g2)


@pytest.mark.parametrize("signs", oo.SIGNS)
@pytest.mark.parametrize("K,D", SHAPES)
def test_kernels_match_torch_f32(K, D, signs, record_property):
    """Bound: max(1e-5, 5 x the deviation of torch's own float32 result from its float64 result on the same input)."""
    X, base, R, (F_ref, g_ref), (F_t32, g_t32) = _case(K, D, signs)
    F, g = _native_result(X, base, R, torch.float32)
    err_f, err_g = rel_err(F, F_ref), rel_err(g, g_ref)
    own_f, own_g = rel_err(F_t32, F_ref), rel_err(g_t32, g_ref)
    for name, v in (("forward_rel_err", err_f), ("grad_rel_err", err_g), ("torch_f32_forward", own_f), ("torch_f32_grad", own_g)):
        record_property(name, v)
    print(f"orthogonal f32 K={K} D={D} {signs}: forward {err_f:.2e} (torch f32 {own_f:.2e}), gradient {err_g:.2e} (torch f32 {own_g:.2e})")
    assert err_f <= max(1e-5, 5 * own_f) and err_g <= max(1e-5, 5 * own_g)
    assert (g[np.tril_indices(K, 0, D)] == 0).all()
    F2, g2 = _native_result(X, base, R, torch.float32)
    assert np.array_equal(F, F2) and np.array_equal(g, g2)


@pytest.mark.parametrize("key", mc.G3O_KEYS)
def test_golden_closures_take_the_native_map_f64(key, no_householder_product):
    mc.check_closure(key, torch.float64, DEV, tol_loss=1e-10, tol_grad=1e-7, tol_dist=1e-9, G3=mc.G3O)


@pytest.mark.parametrize("key", mc.G3O_KEYS_F32)
def test_golden_closures_take_the_native_map_f32(key, no_householder_product):
    ref_dev = rel_err(mc.G3O[f"{key}_grad_f32"], mc.G3O[f"{key}_grad_f64"])
    mc.check_closure(key, torch.float32, DEV, tol_loss=1e-5, tol_grad=max(3e-5, 5 * ref_dev), tol_dist=2e-5, G3=mc.G3O)


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
def test_fit_takes_the_native_map(model_name, no_householder_product):
    mc.check_orthogonal_fit(model_name, DEV)


def _orthogonal_model(model_name, C, D, K, dtype):
    stats = {k: v.to(dtype).to(DEV) for k, v in mc.c2_statistics(C=C, D=D).items()}
    inp = stats if model_name == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
    model = mc.make_model(model_name, D, K, 0.01, "orthogonal", dtype, DEV)
    X, base, _ = oo.make_case(K, D, "mixed")
    mc.set_orthogonal_base(model, base)
    with torch.no_grad():
        model.parametrizations.filters.original.copy_(torch.tensor(X, dtype=dtype))
    return model, model._prepare_statistics(inp)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model_name,C,D,K", [("smsqfa", 24, 96, 4), ("sqfa", 12, 64, 9), ("smsqfa", 9, 72, 17), ("sqfa", 40, 48, 1)])
def test_single_node_closure_matches_autograd_chain(model_name, C, D, K, dtype, monkeypatch):
    """_native.FusedClosure with the orthogonal map as its parametrization stage against the chain of autograd nodes with
    torch's own _Orthogonal.forward in front (NATIVE_ORTHOGONAL off): same loss, flags and raw-parameter gradient, to the
    tolerances of tests/test_gpu_model.py::test_single_node_closure_matches_autograd_chain."""
    from sqfa_amd import constraints
    model, prepared = _orthogonal_model(model_name, C, D, K, dtype)
    results = []
    for native in (True, False):
        monkeypatch.setattr(constraints, "NATIVE_ORTHOGONAL", native)
        assert (model._single_node_inputs(prepared) is not None) == native
        model.zero_grad()
        loss, flags = model._fused_closure_loss(prepared)
        (3.0 * loss).backward()                      # a non-unit incoming gradient
        results.append((loss.item(), flags.tolist(), model.parametrizations.filters.original.grad.clone()))
    (l1, f1, g1), (l0, f0, g0) = results
    assert f1 == f0 == [0, 0]
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    assert abs(l1 - l0) <= tol * abs(l0)
    assert rel_err(g1.cpu(), g0.cpu()) <= (1e-10 if dtype == torch.float64 else 2e-4)
    assert (g1.cpu().numpy()[np.tril_indices(K, 0, D)] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_single_node_closure_replays_in_a_graph(dtype, no_householder_product):
    """Forward + backward of the single-node closure captured in a HIP graph; the raw parameter changes in place; the
    replay equals an eager evaluation at the new point bit for bit."""
    model, prepared = _orthogonal_model("sqfa", 12, 64, 9, dtype)
    raw = model.parametrizations.filters.original
    assert model._single_node_inputs(prepared) is not None and model._noise_scalar() is not None

    def evaluate():
        raw.grad = None
        loss, flags = model._fused_closure_loss(prepared)
        loss.backward()
        return loss.detach(), flags, raw.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            evaluate()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    # torch no longer collects garbage before a capture, and a cyclic collection inside one that finalises device
    # tensors or an older graph aborts the process (_optim._no_gc): collect now, none while the stream captures
    gc.collect()
    with _no_gc(), torch.cuda.graph(graph):
        g_loss, g_flags, g_grad = evaluate()
    step = torch.tensor(oo.make_case(9, 64, "negative", seed=7)[0], dtype=dtype, device=DEV)
    with torch.no_grad():
        raw.add_(0.05 * step)
    graph.replay()
    torch.cuda.synchronize()
    replayed = (g_loss.clone(), g_flags.clone(), g_grad.clone())
    loss, flags, grad = evaluate()
    assert flags.tolist() == [0, 0] and torch.isfinite(loss)
    assert torch.equal(replayed[0], loss) and torch.equal(replayed[1], flags) and torch.equal(replayed[2], grad)


def test_switch_restores_torchs_map(monkeypatch):
    from sqfa_amd import constraints
    model, prepared = _orthogonal_model("smsqfa", 24, 96, 4, torch.float64)
    calls = []
    original = torch.linalg.householder_product
    monkeypatch.setattr(torch.linalg, "householder_product", lambda *a, **k: calls.append(1) or original(*a, **k))
    native = model.filters.detach().clone()
    assert not calls and model._single_node_inputs(prepared) is not None
    monkeypatch.setattr(constraints, "NATIVE_ORTHOGONAL", False)
    assert model._single_node_inputs(prepared) is None
    assert rel_err(model.filters.detach().cpu(), native.cpu()) < 1e-12
    assert calls
