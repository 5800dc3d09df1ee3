"""GPU tests of the affine-invariant family at matrix sizes 65..128 (the LDS pair kernel) against the float64 numpy
oracle (oracle/closed_form.py) and the torch expression of the reference (oracle/reference_path.py).

Tolerances as in test_gpu_parity: float64 loss 1e-11, distances 1e-10, gradients 1e-8; float32 loss 1e-5,
distances 2e-5, gradients max(1e-5, 5 x the reference's own float32 deviation on the same matrices) -- the rule of
test_gpu_parity._tols, with the deviation measured here by running the reference's torch expression
(oracle/reference_path.py) in float32 on the GPU.  float32 runs are compared with the oracle evaluated on the inputs as
the kernel receives them (rounded to float32)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import closed_form, reference_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = dict(loss=1e-11, dist=1e-10, grad=1e-8)
F32 = dict(loss=1e-5, dist=2e-5, grad=1e-5)
DTYPES = [torch.float64, torch.float32]


def _tol(dtype):
    return F64 if dtype == torch.float64 else F32


def _spd(C, m, seed, ridge=0.02):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((C, 3 * m, m))
    return np.einsum("cnm,cnk->cmk", X, X) / (3 * m) + ridge * np.eye(m)


def _rounded(X, dtype):
    """the float64 values of X as the kernel of `dtype` receives them"""
    return np.asarray(X, dtype=np.float32).astype(np.float64) if dtype == torch.float32 else np.asarray(X)


def _f32_grad_bound(S):
    """max(1e-5, 5 x the float32 deviation of the reference's own closure gradient) on the classes S (float64 numpy)"""
    _, g_ref, _ = closed_form.closure_loss_and_grad(S)
    _, g32, _ = reference_path.pairwise_loss_and_grad(torch.tensor(S, dtype=torch.float32, device=DEV))
    return max(1e-5, 5 * rel_err(g32.double().cpu(), g_ref))


def _grad_tol(dtype, S):
    return F64["grad"] if dtype == torch.float64 else _f32_grad_bound(S)


def _fused(S, scale=1.0, sqrt_mode=True, shard=(0, 1)):
    from sqfa_amd import _native, distances
    C = S.shape[0]
    P = C * (C - 1) // 2
    S = S.clone().requires_grad_(True)
    loss, flags = _native.PairwiseLoss.apply(S, scale, distances.EPSILON, sqrt_mode, -1.0 / P, shard, None)
    loss.backward()
    return loss.detach(), S.grad, flags


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,m", [(5, 65), (4, 72), (6, 80), (3, 96), (4, 127), (3, 128), (12, 100)])
def test_fused_loss_and_grad_vs_oracle(C, m, dtype):
    from sqfa_amd import distances
    S = _rounded(_spd(C, m, C * 1000 + m), dtype)
    loss_ref, grad_ref, D_ref = closed_form.closure_loss_and_grad(S)
    St = torch.tensor(S, dtype=dtype, device=DEV)
    loss, grad, flags = _fused(St)
    tol = _tol(dtype)
    assert flags.tolist() == [0, 0]
    assert abs(loss.item() - loss_ref) <= tol["loss"] * abs(loss_ref)
    assert rel_err(grad.cpu(), grad_ref) <= _grad_tol(dtype, S)
    D = distances.affine_invariant(St, St).cpu().numpy()
    assert np.abs(D - D_ref).max() <= tol["dist"] * max(1.0, np.abs(D_ref).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [65, 101])
def test_distance_functions_and_autograd(m, dtype):
    """affine_invariant[_sq] (cross mode, nA != nB) and fisher_rao_lower_bound[_sq] on embeddings of size m = K + 1:
    values and autograd gradients for a random upstream gradient."""
    from sqfa_amd import distances
    tol = _tol(dtype)
    A, B = _rounded(_spd(4, m, 7 + m), dtype), _rounded(_spd(3, m, 8 + m), dtype)
    G = np.random.default_rng(m).standard_normal((4, 3))
    gtol = _grad_tol(dtype, np.concatenate([A, B]))
    for fn, sqrt_mode in ((distances.affine_invariant, True), (distances.affine_invariant_sq, False)):
        At = torch.tensor(A, dtype=dtype, device=DEV, requires_grad=True)
        Bt = torch.tensor(B, dtype=dtype, device=DEV, requires_grad=True)
        D = fn(At, Bt)
        (D * torch.tensor(G, dtype=dtype, device=DEV)).sum().backward()
        D_ref, gA_ref, gB_ref = closed_form.pairwise(A, B, G, 1.0, sqrt_mode)
        assert np.abs(D.detach().cpu().numpy() - D_ref).max() <= tol["dist"] * max(1.0, np.abs(D_ref).max())
        assert rel_err(At.grad.cpu(), gA_ref) <= gtol
        assert rel_err(Bt.grad.cpu(), gB_ref) <= gtol
    # Fisher-Rao lower bound: K = m - 1 filters, embeddings of size m
    K = m - 1
    rng = np.random.default_rng(K)
    cov, mu = _rounded(_spd(5, K, 99 + K), dtype), _rounded(0.3 * rng.standard_normal((5, K)), dtype)
    E = _rounded(closed_form.embed_gaussian(mu, cov), dtype)
    C = 5
    W = np.tril(rng.standard_normal((C, C)), -1)
    gtol = _grad_tol(dtype, E)
    for fn, sqrt_mode in ((distances.fisher_rao_lower_bound, True), (distances.fisher_rao_lower_bound_sq, False)):
        stats = {"means": torch.tensor(mu, dtype=dtype, device=DEV, requires_grad=True),
                 "covariances": torch.tensor(cov, dtype=dtype, device=DEV, requires_grad=True)}
        D = fn(stats, stats)
        (D * torch.tensor(W, dtype=dtype, device=DEV)).sum().backward()
        D_ref, gE_ref, _ = closed_form.pairwise(E, None, W, 0.5, sqrt_mode)
        assert np.abs(D.detach().cpu().numpy() - D_ref).max() <= tol["dist"] * max(1.0, np.abs(D_ref).max())
        # gradient wrt the covariances: the top-left block of the embedding's gradient
        assert rel_err(stats["covariances"].grad.cpu(), gE_ref[:, :K, :K]) <= gtol


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_mode_with_pair_weights(dtype):
    from sqfa_amd import _native
    tol = _tol(dtype)
    A, B = _rounded(_spd(5, 88, 1), dtype), _rounded(_spd(3, 88, 2), dtype)
    Wn = np.random.default_rng(3).standard_normal((5, 3))
    At, Bt = torch.tensor(A, dtype=dtype, device=DEV), torch.tensor(B, dtype=dtype, device=DEV)
    out = _native.hip_pair_backend(At, Bt, scale=1.0, eps=1e-6, sqrt_mode=True,
                                   weights=torch.tensor(Wn, dtype=dtype, device=DEV), uniform_weight=0.0, shard=(0, 1),
                                   want_loss=True, want_grad=True, want_dist=True, want_eig=False)
    D_ref, gA_ref, gB_ref = closed_form.pairwise(A, B, Wn)
    loss_ref = (Wn * D_ref).sum()
    assert out["nonfinite"].tolist() == [0, 0]
    assert abs(out["loss"].item() - loss_ref) <= tol["loss"] * np.abs(Wn * D_ref).sum()
    assert np.abs(out["dist"].cpu().numpy() - D_ref).max() <= tol["dist"] * np.abs(D_ref).max()
    gtol = _grad_tol(dtype, np.concatenate([A, B]))
    assert rel_err(out["gradA"].cpu(), gA_ref) <= gtol
    assert rel_err(out["gradB"].cpu(), gB_ref) <= gtol


@pytest.mark.parametrize("dtype", DTYPES)
def test_generalized_eigenvalues_and_backward(dtype):
    from sqfa_amd import linalg
    A, B = _rounded(_spd(3, 70, 11), dtype), _rounded(_spd(2, 70, 12), dtype)
    At = torch.tensor(A, dtype=dtype, device=DEV, requires_grad=True)
    Bt = torch.tensor(B, dtype=dtype, device=DEV, requires_grad=True)
    lam = linalg.generalized_eigenvalues(At, Bt)
    ref = closed_form.generalized_eigenvalues(A, B)
    assert rel_err(lam.detach().cpu(), ref) <= (1e-11 if dtype == torch.float64 else 2e-5)  # test_gpu_parity's bounds
    gtol = _grad_tol(dtype, np.concatenate([A, B]))
    Wk = np.random.default_rng(5).standard_normal(ref.shape)
    (lam * torch.tensor(Wk, dtype=dtype, device=DEV)).sum().backward()
    gA_ref, gB_ref = closed_form.eigenvalue_weight_gradient(A, B, Wk)
    assert rel_err(At.grad.cpu(), gA_ref) <= gtol
    assert rel_err(Bt.grad.cpu(), gB_ref) <= gtol
    # self case: the mirrored 1/lambda entries carry their own derivative
    Ct = torch.tensor(A, dtype=dtype, device=DEV, requires_grad=True)
    lam_s = linalg.generalized_eigenvalues(Ct, Ct)
    Ws = np.random.default_rng(6).standard_normal(lam_s.shape)
    (lam_s * torch.tensor(Ws, dtype=dtype, device=DEV)).sum().backward()
    gA_s, gB_s = closed_form.eigenvalue_weight_gradient(A, A, Ws)
    assert rel_err(Ct.grad.cpu(), gA_s + gB_s) <= 10 * gtol


@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_sum_to_the_whole(dtype):
    from sqfa_amd import _native
    S = torch.tensor(_spd(23, 72, 21), dtype=dtype, device=DEV)
    P = 23 * 22 // 2

    def run(shard):
        return _native.hip_pair_backend(S, None, scale=1.0, eps=1e-6, sqrt_mode=True, weights=None,
                                        uniform_weight=-1.0 / P, shard=shard, want_loss=True, want_grad=True,
                                        want_dist=True, want_eig=False)
    whole = run((0, 1))
    rtol = 1e-12 if dtype == torch.float64 else 1e-5
    for n in (2, 3):
        parts = [run((r, n)) for r in range(n)]
        loss = sum(p["loss"].item() for p in parts)
        grad = sum(p["gradA"] for p in parts)
        assert abs(loss - whole["loss"].item()) <= rtol * abs(whole["loss"].item())
        assert rel_err(grad.cpu(), whole["gradA"].cpu()) <= rtol
        # every off-diagonal entry is written by exactly one shard, and there with the unsharded value
        written = sum((p["dist"] != 0).to(torch.int32) for p in parts)
        off = ~torch.eye(23, dtype=torch.bool, device=DEV)
        assert (written[off] == 1).all()
        assert torch.equal(sum(p["dist"] * off for p in parts), whole["dist"] * off)


def test_bitwise_reproducible():
    for dtype in DTYPES:
        S = torch.tensor(_spd(9, 104, 31), dtype=dtype, device=DEV)
        l0, g0, _ = _fused(S)
        l1, g1, _ = _fused(S)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_sampled_c200_m72_f32():
    from sqfa_amd import _native
    C, m = 200, 72
    S = _rounded(_spd(C, m, 200), torch.float32)
    P = C * (C - 1) // 2
    St = torch.tensor(S, dtype=torch.float32, device=DEV)
    out = _native.hip_pair_backend(St, None, scale=1.0, eps=1e-6, sqrt_mode=True, weights=None,
                                   uniform_weight=-1.0 / P, shard=(0, 1), want_loss=True, want_grad=True,
                                   want_dist=True, want_eig=False)
    assert out["nonfinite"].tolist() == [0, 0]
    D = out["dist"].cpu().numpy()
    rng = np.random.default_rng(7)
    Linv = np.linalg.inv(np.linalg.cholesky(S))
    for _ in range(200):
        i, j = rng.choice(C, 2, replace=False)
        lam, _ = closed_form._pair_terms(S[i], Linv[j])
        d = np.sqrt(np.sum(np.log(lam) ** 2) + 1e-6)
        assert abs(D[i, j] - d) <= 2e-5 * max(1.0, d)
    g = out["gradA"].cpu().numpy()
    for c in (0, 137):
        # the distance is symmetric: class c's gradient row is the A side of c against every other class
        others = np.delete(S, c, axis=0)
        _, gref, _ = closed_form.pairwise(S[c:c + 1], others, np.full((1, C - 1), -1.0 / P))
        assert rel_err(g[c], gref[0]) <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_inputs(dtype):
    from sqfa_amd import distances
    m = 76
    S = _spd(3, m, 41)
    # identical classes: d = sqrt(eps), finite zero-ish gradient
    Si = np.stack([S[0], S[0], S[1]])
    St = torch.tensor(Si, dtype=dtype, device=DEV)
    D = distances.affine_invariant(St, St)
    assert abs(D[1, 0].item() - 1e-3) <= (1e-12 if dtype == torch.float64 else 1e-6)
    loss, grad, flags = _fused(St)
    assert flags.tolist() == [0, 0] and torch.isfinite(grad).all()
    if dtype == torch.float64:  # (float32: log(lambda) of the identical pair is rounding noise, amplified by 1/d)
        loss_ref, grad_ref, _ = closed_form.closure_loss_and_grad(Si)
        assert rel_err(grad.cpu(), grad_ref) <= 10 * F64["grad"]
    # repeated eigenvalues: B = 2 A except on a 3-dimensional subspace
    Q = np.linalg.qr(np.random.default_rng(2).standard_normal((m, m)))[0]
    ev = np.full(m, 2.0)
    ev[:3] = (3.0, 0.5, 0.7)
    Sr = np.stack([S[0], Q.T @ np.diag(1.0 / ev) @ Q, S[2]])
    Sr[1] = np.linalg.cholesky(S[0]) @ Sr[1] @ np.linalg.cholesky(S[0]).T
    Sr[1] = 0.5 * (Sr[1] + Sr[1].T)
    Sr = _rounded(Sr, dtype)
    loss, grad, flags = _fused(torch.tensor(Sr, dtype=dtype, device=DEV))
    loss_ref, grad_ref, _ = closed_form.closure_loss_and_grad(Sr)
    assert flags.tolist() == [0, 0]
    assert abs(loss.item() - loss_ref) <= _tol(dtype)["loss"] * abs(loss_ref)
    assert rel_err(grad.cpu(), grad_ref) <= 10 * _grad_tol(dtype, Sr)


def test_anisotropic_class_f64():
    m = 90
    S = _spd(4, m, 51)
    Q = np.linalg.qr(np.random.default_rng(3).standard_normal((m, m)))[0]
    S[2] = Q @ np.diag(np.logspace(0, 4, m)) @ Q.T  # condition number 1e4
    S[2] = 0.5 * (S[2] + S[2].T)
    loss, grad, flags = _fused(torch.tensor(S, dtype=torch.float64, device=DEV))
    loss_ref, grad_ref, _ = closed_form.closure_loss_and_grad(S)
    assert flags.tolist() == [0, 0]
    assert abs(loss.item() - loss_ref) <= F64["loss"] * abs(loss_ref)
    assert rel_err(grad.cpu(), grad_ref) <= F64["grad"]


def test_non_spd_class_reports_nonfinite():
    import sqfa_amd
    from sqfa_amd import _native
    m = 80
    S = torch.tensor(_spd(5, m, 61), dtype=torch.float64, device=DEV)
    S[3] = -S[3]
    out = _native.hip_pair_backend(S, None, scale=1.0, eps=1e-6, sqrt_mode=True, weights=None, uniform_weight=-0.1,
                                   shard=(0, 1), want_loss=True, want_grad=True, want_dist=True, want_eig=False)
    torch.cuda.synchronize()
    assert sum(out["nonfinite"].tolist()) > 0
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=m, feature_noise=0.0, n_filters=m).double().to(DEV)
    with pytest.raises(ValueError, match="NaN"):
        model.fit(data_statistics=S, max_epochs=2, show_progress=False)


def _reference_closure(model, stats, kind, noise):
    """loss and gradient wrt the raw filter parameter through the reference's torch expression (float64, CPU)."""
    X = model.parametrizations.filters.original.detach().cpu().double().requires_grad_(True)
    F = X / X.norm(dim=1, keepdim=True)
    K = F.shape[0]
    cov = stats["covariances"].cpu().double()
    mu = stats["means"].cpu().double()
    if kind == "sqfa":
        C_f = F @ cov @ F.T + noise * torch.eye(K, dtype=torch.float64)
        m_f = mu @ F.T
        E = torch.empty(cov.shape[0], K + 1, K + 1, dtype=torch.float64)
        E[:, :K, :K] = C_f + m_f[:, :, None] * m_f[:, None, :]
        E[:, :K, K] = m_f
        E[:, K, :K] = m_f
        E[:, K, K] = 1.0
        S, scale = E, 0.5
    else:
        second = cov + mu[:, :, None] * mu[:, None, :]
        S, scale = F @ second @ F.T + noise * torch.eye(K, dtype=torch.float64), 1.0
    loss, gS, _ = reference_path.pairwise_loss_and_grad(S.detach(), scale=scale)
    (gX,) = torch.autograd.grad((S * gS).sum(), X)
    return loss.item(), gX


@pytest.mark.parametrize("kind,K", [("sqfa", 64), ("smsqfa", 96)])
def test_model_closure_vs_reference_f64(kind, K):
    import model_cases as mc
    stats = {k: v.to(DEV) for k, v in mc.c2_statistics(C=6, D=160).items()}
    model = mc.make_model(kind, 160, K, 0.01, "sphere", torch.float64, DEV)
    inp = stats if kind == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
    prepared = model._prepare_statistics(inp)
    model.zero_grad()
    loss, flags = model._fused_closure_loss(prepared)
    loss.backward()
    assert flags.tolist() == [0, 0]
    noise = float(torch.tensor(0.01, dtype=torch.float32))  # the model keeps its noise matrix in float32
    loss_ref, g_ref = _reference_closure(model, stats, kind, noise)
    assert abs(loss.item() - loss_ref) <= 1e-10 * abs(loss_ref)
    assert rel_err(model.parametrizations.filters.original.grad.cpu(), g_ref) <= 1e-7


@pytest.mark.parametrize("kind,K", [("sqfa", 64), ("smsqfa", 96)])
def test_fit_three_epochs_lowers_the_loss(kind, K):
    import model_cases as mc
    stats = {k: v.to(DEV) for k, v in mc.c2_statistics(C=6, D=160).items()}
    model = mc.make_model(kind, 160, K, 0.01, "sphere", torch.float64, DEV)
    inp = stats if kind == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
    loss, _ = model.fit(data_statistics=inp, max_epochs=3, show_progress=False, return_loss=True)
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]


def test_boundary_64_and_65():
    """m = 64 keeps the register kernel (its geometry and its results), m = 65 runs on the LDS path: both agree with the
    oracle."""
    import ctypes
    from sqfa_amd import _lib
    lib = _lib.load()
    out = [ctypes.c_int() for _ in range(5)]
    assert lib.sqfa_airm_tiling(10, 0, 64, _lib.SQFA_F64, *[ctypes.byref(v) for v in out]) == 0
    assert out[4].value == 64 and 64 % out[0].value == 0
    for m in (64, 65):
        S = _spd(5, m, 300 + m)
        loss_ref, grad_ref, _ = closed_form.closure_loss_and_grad(S)
        loss, grad, flags = _fused(torch.tensor(S, dtype=torch.float64, device=DEV))
        assert flags.tolist() == [0, 0]
        assert abs(loss.item() - loss_ref) <= F64["loss"] * abs(loss_ref)
        assert rel_err(grad.cpu(), grad_ref) <= F64["grad"]
