"""Pins tests/projection_oracle.py (the float64 definition the GPU tests of the projection-side kernels compare with)
without a GPU: against the reference's own outputs (golden G3b), against oracle/reference_path.embed_gaussian, every
hand-written backward formula against torch autograd, and -- on the input families of tests/test_gpu_projection_kernels.py --
the same expressions evaluated in float32 numpy against the float32 bound those tests hold the kernels to."""
import numpy as np
import pytest
import torch

import model_cases as mc
import orthogonal_oracle
import projection_oracle as po
from conftest import load_golden, rel_err
from oracle import reference_path

F32 = np.float32


@pytest.mark.parametrize("C,D,K", [(3, 784, 16), (2, 2048, 32), (4, 132, 8)])
def test_stage_reproduces_the_reference_transform(C, D, K):
    """Golden G3b: the reference's transform_scatters / transform (sphere constraint, no noise) and the gradient of
    sum(W * S) with respect to the raw filters, W a general (non-symmetric) weight."""
    G3B = load_golden("g3b_transform_scatters.npz")
    key = f"C{C}_D{D}_K{K}"
    stats = mc.c2_statistics(C=C, D=D)
    cov = stats["covariances"].numpy()
    assert np.allclose(cov[0, :3, :3], G3B[f"{key}_check"], rtol=1e-12)
    st = po.stage(G3B[f"{key}_raw"], cov, None, 0.0, "sphere", G3B[f"{key}_W"], 1.0)
    assert rel_err(st["out"].value, G3B[f"{key}_S_f64"]) < 1e-13
    assert rel_err(st["dX_autograd"], G3B[f"{key}_grad_f64"]) < 1e-12
    assert rel_err(st["dX"].value, G3B[f"{key}_grad_f64"]) < 1e-12
    assert rel_err(stats["means"].numpy() @ st["F"].T, G3B[f"{key}_Z_f64"]) < 1e-13
    # the parts the stage is made of
    T = po.project(cov, st["F"])
    assert rel_err(po.feature_scatters(st["F"], T.value, 0.0).value, G3B[f"{key}_S_f64"]) < 1e-13
    F, norms = po.sphere_forward(G3B[f"{key}_raw"])
    assert np.array_equal(F.value, st["F"]) and np.abs(np.linalg.norm(F.value, axis=1) - 1).max() < 1e-15
    assert np.allclose(norms.value, np.linalg.norm(G3B[f"{key}_raw"], axis=1), rtol=1e-15)


@pytest.mark.parametrize("C,K,D", [(1, 1, 4), (3, 5, 12), (2, 17, 20)])
def test_embedding_layout_is_the_reference_path(C, K, D):
    c = po.case_forward(C, D, K, np.float64)
    fs = po.feature_scatters(c["F"], c["T"], 0.01, c["m"])
    S = po.feature_scatters(c["F"], c["T"], 0.01).value
    E = reference_path.embed_gaussian(torch.tensor(c["m"]), torch.tensor(S)).numpy()
    assert fs.value.shape == (C, K + 1, K + 1) and np.abs(fs.value - E).max() <= 1e-15 * np.abs(E).max()
    assert (fs.mag >= np.abs(fs.value)).all() and (fs.value[:, K, K] == 1).all()
    assert np.array_equal(fs.value[:, :K, K], c["m"]) and np.array_equal(fs.value[:, K, :K], c["m"])


@pytest.mark.parametrize("C,D,K,ldg,n_groups", [(3, 8, 2, 2, 1), (5, 12, 5, 6, 3), (3, 20, 17, 18, 5), (2, 4, 1, 1, 2)])
def test_backward_product_formula_vs_autograd(C, D, K, ldg, n_groups):
    """sum_g P_g = d/dF sum(G[:K,:K] * F Psi F^T) for symmetric Psi and a general G; groups partition the classes."""
    rng = po.rng_for(11, C, D, K)
    Psi = po.symmetric_scatters(rng, C, D, np.float64)
    F = rng.standard_normal((K, D))
    G = rng.standard_normal((C, ldg, ldg))
    Ft = torch.tensor(F, requires_grad=True)
    S = Ft.unsqueeze(0) @ torch.tensor(Psi) @ Ft.T.unsqueeze(0)
    (torch.tensor(G[:, :K, :K]) * S).sum().backward()
    T = po.project(Psi, F).value
    P = po.backward_partials(G, T, n_groups)
    assert P.value.shape == (n_groups, K, D)
    assert rel_err(P.value.sum(0), Ft.grad.numpy()) < 1e-13
    counts = po.group_counts(C, n_groups)
    assert counts.sum() == C and np.array_equal(np.ravel(P.n), 2 * K * counts)
    for g in range(n_groups):
        alone = po.backward_partials(G[g::n_groups], T[g::n_groups], 1) if counts[g] else None
        if alone is None:
            assert not P.value[g].any() and not P.mag[g].any()
        else:
            assert np.allclose(P.value[g], alone.value[0], rtol=1e-13, atol=1e-13)
    assert (P.mag >= np.abs(P.value) * (1 - 1e-12)).all()


@pytest.mark.parametrize("C,K", [(1, 1), (3, 5), (4, 16)])
def test_embed_backward_means_formula_vs_autograd(C, K):
    c = po.case_embed(C, K, np.float64)
    rng = po.rng_for(12, C, K)
    S = rng.standard_normal((C, K, K))
    mt = torch.tensor(c["m"], requires_grad=True)
    (torch.tensor(c["gE"]) * reference_path.embed_gaussian(mt, torch.tensor(S))).sum().backward()
    gm = po.embed_backward_means(c["gE"], c["m"])
    assert rel_err(gm.value, mt.grad.numpy()) < 1e-14
    assert (gm.mag >= np.abs(gm.value) * (1 - 1e-12)).all()


@pytest.mark.parametrize("K,D,n_groups", [(1, 1, 0), (1, 4, 1), (3, 257, 5), (3, 12, 0)])
@pytest.mark.parametrize("with_norms", [True, False])
def test_sphere_backward_formula_vs_autograd(K, D, n_groups, with_norms):
    c = po.case_sphere(K, D, n_groups, np.float64)
    Xt = torch.tensor(c["X"], requires_grad=True)
    Ft = Xt / torch.linalg.norm(Xt, dim=1, keepdim=True) if with_norms else Xt
    gF = c["extra"] + (c["partials"].sum(0) if n_groups else 0.0)
    (c["gloss"] * (torch.tensor(gF) * Ft).sum()).backward()
    sb = po.sphere_backward(c["X"], c["norms"] if with_norms else None, c["partials"], c["extra"], c["gloss"])
    # (D = 1 cancels to zero: the comparison is against the magnitude, i.e. the float64 bound itself)
    assert po.ratio(Xt.grad.numpy(), sb, np.float64) <= po.C_FACTOR
    assert (sb.mag >= np.abs(sb.value) * (1 - 1e-12)).all()
    none = po.sphere_backward(c["X"], c["norms"] if with_norms else None, None, None, None)
    assert not none.value.any() and not none.mag.any()


@pytest.mark.parametrize("K,D", [(1, 8), (5, 12), (17, 68)])
def test_orthogonal_restatement_in_torch(K, D):
    X, base, R = orthogonal_oracle.make_case(K, D, "mixed", seed=3)
    Xt = torch.tensor(X, requires_grad=True)
    F = po.orthogonal_forward_torch(Xt, torch.tensor(base))
    (F * torch.tensor(R)).sum().backward()
    assert rel_err(F.detach().numpy(), orthogonal_oracle.forward(X, base)) < 1e-13
    assert rel_err(Xt.grad.numpy(), orthogonal_oracle.backward(X, base, R)) < 1e-12


CHAIN_SHAPES = [(1, 8), (17, 68), (33, 132), (64, 132)]


@pytest.mark.parametrize("with_means", [False, True])
@pytest.mark.parametrize("kind", po.CHAIN_KINDS)
@pytest.mark.parametrize("K,D", CHAIN_SHAPES[:3])
def test_stage_formulas_vs_autograd(K, D, kind, with_means):
    """The hand-written backward chain and autograd on the plain expression agree, for every parametrization, with and
    without the means path; the float64 values are far inside their own float64 bound."""
    c = po.case_chain(K, D, 3, kind, with_means, np.float64)
    st = po.stage(c["X"], c["Psi"], c["means"], c["noise"], c["base"] if kind == "orthogonal" else kind, c["gS"], c["gloss"])
    m = K + 1 if with_means else K
    assert st["out"].value.shape == (3, m, m)
    assert rel_err(st["dX"].value, st["dX_autograd"]) < 1e-11
    assert po.ratio(st["dX_autograd"], st["dX"], np.float64) <= po.C_FACTOR
    assert (st["dX"].mag >= np.abs(st["dX"].value) * (1 - 1e-9)).all()
    assert (st["out"].mag >= np.abs(st["out"].value) * (1 - 1e-9)).all()


# ---- the float32 evaluation of the oracle's own expressions stays inside the float32 bound ---------------------------


@pytest.mark.parametrize("C,D,K", [(2, 4, 1), (3, 12, 3), (2, 68, 17), (2, 132, 49), (2, 64, 64), (2, 1028, 20), (2, 2052, 4)])
def test_float32_project_inside_bound(C, D, K):
    c = po.case_project(C, D, K, F32)
    ref = po.project(c["Psi"], c["F"])
    assert po.ratio(po.project(c["Psi"], c["F"], F32).value, ref, F32) <= po.C_FACTOR
    assert po.ratio(ref.value, ref, F32) == 0.0


@pytest.mark.parametrize("C,D,K", [(1, 4, 1), (3, 28, 15), (3, 132, 33), (1, 144, 64)])
@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("with_means", [False, True])
def test_float32_feature_scatters_inside_bound(C, D, K, noise, with_means):
    c = po.case_forward(C, D, K, F32)
    noise = float(po.rounded(noise, F32))
    m = c["m"] if with_means else None
    ref = po.feature_scatters(c["F"], c["T"], noise, m)
    assert po.ratio(po.feature_scatters(c["F"], c["T"], noise, m, F32).value, ref, F32) <= po.C_FACTOR


@pytest.mark.parametrize("C,D,K,ldg", [(2, 4, 1, 1), (3, 16, 17, 18), (3, 40, 48, 48), (2, 132, 64, 65)])
@pytest.mark.parametrize("symmetric", [False, True])
def test_float32_backward_partials_inside_bound(C, D, K, ldg, symmetric):
    c = po.case_backward(C, D, K, ldg, symmetric, F32)
    for n_groups in (1, 3, C, C + 2):
        ref = po.backward_partials(c["G"], c["T"], n_groups)
        got = po.backward_partials(c["G"], c["T"], n_groups, F32)
        assert po.ratio(got.value, ref, F32) <= po.C_FACTOR
        assert not got.value[C:].any()


@pytest.mark.parametrize("K,D,n_groups", [(1, 1, 0), (3, 4, 1), (1, 255, 3), (3, 257, 7), (1, 784, 64)])
def test_float32_sphere_inside_bound(K, D, n_groups):
    c = po.case_sphere(K, D, n_groups, F32)
    F, norms = po.sphere_forward(c["X"])
    F32v, norms32 = po.sphere_forward(c["X"], F32)
    assert po.ratio(F32v.value, F, F32) <= po.C_FACTOR and po.ratio(norms32.value, norms, F32) <= po.C_FACTOR
    for nrm in (c["norms"], None):
        for extra in (c["extra"], None):
            for gloss in (c["gloss"], None):
                ref = po.sphere_backward(c["X"], nrm, c["partials"], extra, gloss)
                got = po.sphere_backward(c["X"], nrm, c["partials"], extra, gloss, F32)
                assert po.ratio(got.value, ref, F32) <= po.C_FACTOR


@pytest.mark.parametrize("C,K", [(1, 1), (3, 5), (70, 16), (3, 64)])
def test_float32_embed_backward_means_inside_bound(C, K):
    c = po.case_embed(C, K, F32)
    ref = po.embed_backward_means(c["gE"], c["m"])
    assert po.ratio(po.embed_backward_means(c["gE"], c["m"], F32).value, ref, F32) <= po.C_FACTOR


def _stage_float32(c, kind):
    """The chain in float32 torch-CPU arithmetic (sphere / identity): forward values and autograd gradient."""
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    X = t(c["X"]).requires_grad_(True)
    F = X / torch.linalg.norm(X, dim=1, keepdim=True) if kind == "sphere" else X
    T = t(c["Psi"]) @ F.T
    S = F.unsqueeze(0) @ T + np.float32(c["noise"]) * torch.eye(X.shape[0])
    out = S if c["means"] is None else reference_path.embed_gaussian(t(c["means"]) @ F.T, S)
    (np.float32(c["gloss"]) * (t(c["gS"]) * out).sum()).backward()
    return out.detach().numpy(), X.grad.numpy()


@pytest.mark.parametrize("with_means", [False, True])
@pytest.mark.parametrize("kind", ["sphere", "identity"])
@pytest.mark.parametrize("K,D", CHAIN_SHAPES)
def test_float32_chain_inside_bound(K, D, kind, with_means):
    """(The orthogonal map's float32 evaluation is the business of tests/test_gpu_orthogonal.py and its oracle: the
    kernels compute its K x K quantities in double whatever the dtype, which a float32 numpy restatement would not.)"""
    c = po.case_chain(K, D, 3, kind, with_means, F32)
    st = po.stage(c["X"], c["Psi"], c["means"], c["noise"], kind, c["gS"], c["gloss"])
    out32, dX32 = _stage_float32(c, kind)
    assert po.ratio(out32, st["out"], F32) <= po.C_FACTOR
    assert po.ratio(dX32, st["dX"], F32) <= po.C_FACTOR
