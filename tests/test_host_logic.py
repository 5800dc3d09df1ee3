"""CPU tests of the host side (model shell, fitting loop, statistics, constraints, torch-only
distance operators) with the float64 ORACLE installed as pair backend, against the goldens
captured from the reference (G3 closure, G4 fit trajectories, G5 quirks) and the
reference's error contract (its tests/test_training.py)."""
import numpy as np
import pytest
import torch

import model_cases as mc
from conftest import rel_err
from oracle_backend import oracle_eigenvalues_backward, oracle_pair_backend


@pytest.fixture(autouse=True)
def _oracle_backend():
    from sqfa_amd import _native
    saved = _native._pair_backend
    saved_eig = _native._eig_backward_backend
    _native._pair_backend = oracle_pair_backend   # test-only substitution of the module attribute
    _native._eig_backward_backend = oracle_eigenvalues_backward
    yield
    _native._pair_backend = saved
    _native._eig_backward_backend = saved_eig


CPU = torch.device("cpu")


@pytest.mark.parametrize("key", mc.G3_KEYS)
def test_closure_matches_reference(key):
    mc.check_closure(key, torch.float64, CPU, tol_loss=1e-10, tol_grad=1e-7, tol_dist=1e-9)


@pytest.mark.parametrize("key", mc.G3O_KEYS)
def test_orthogonal_closure_matches_reference(key):
    """constraint="orthogonal" (reference src/sqfa/model.py:416-431) with the parametrization's stored `base`."""
    mc.check_closure(key, torch.float64, CPU, tol_loss=1e-10, tol_grad=1e-7, tol_dist=1e-9, G3=mc.G3O)


def test_c1_config_early_epochs_filters_match_reference():
    """BASELINE config 1 shape, five epochs: learned filters to 1e-5 (host logic + oracle backend)."""
    mc.check_early_epochs("g6c_fit_c1_early.npz", 10, 784, 4, 5, CPU)


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
def test_orthogonal_fit_matches_reference(model_name):
    mc.check_orthogonal_fit(model_name, CPU)


@pytest.mark.parametrize("dname", ["rot", "syn"])
@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
@pytest.mark.parametrize("K,noise", [(2, 1e-3), (4, 1e-2)])
@pytest.mark.parametrize("epochs", [1, 3])
def test_short_fit_trajectories(dname, model_name, K, noise, epochs):
    # losses come back as a float32 tensor (default dtype, like the reference) -> 1e-6.
    # rot/K=4 sits on the flat orbit F -> G F of the AIRM loss (SURVEY.md 7 "hard parts"; the
    # reference's own float32 run diverges there): bounds = 2 x the reference's own spread under
    # rounding-level perturbations at that point (golden G4D).
    tol_loss, tol_filters = 1e-6, 1e-7
    if dname == "rot" and K == 4 and epochs > 1:
        spread_f, spread_l = mc.rot_k4_spread(model_name)
        tol_loss, tol_filters = max(1e-6, 2 * spread_l), max(1e-7, 2 * spread_f)
    mc.check_fit(dname, model_name, K, noise, epochs, CPU, tol_loss=tol_loss, tol_filters=tol_filters)


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
def test_full_fit_to_convergence_rot(model_name):
    # stopping rule, epoch count and learned filters of a converged float64 fit
    mc.check_fit("rot", model_name, 2, 1e-3, 300, CPU, tol_loss=1e-6, tol_filters=1e-5)


def test_pairwise_fit_syn():
    # flat-orbit case (see tests/test_gpu_model.py::test_full_fit_flat_orbit_case_f64)
    stats = mc.fit_stats("syn", torch.float64, CPU)
    model = mc.make_model("smsqfa", 50, 4, 1e-2, "sphere", torch.float64, CPU)
    model.fit_pca(data_statistics=stats)
    loss, t = model.fit(data_statistics=stats, max_epochs=300, show_progress=False, return_loss=True, pairwise=True)
    ref = mc.G4["syn_smsqfa_pairwise_K4_loss"]
    assert abs(loss[-1].item() - ref[-1]) <= 1e-5 * abs(ref[-1])
    assert rel_err(model.filters.detach(), mc.G4["syn_smsqfa_pairwise_K4_filters"]) <= 5e-3


# ---------------------------------------------------------------- error contract (reference tests/test_training.py)
def _rot_cov():
    return torch.tensor(mc.G4["rotated_cov"], dtype=torch.float32)


def test_sqfa_rejects_tensor_statistics():
    import sqfa_amd
    model = sqfa_amd.model.SQFA(n_dim=8, feature_noise=0.001, n_filters=2)
    with pytest.raises(TypeError):
        sqfa_amd._optim.fitting_loop(model=model, data_statistics=_rot_cov(), max_epochs=2, show_progress=False)
    with pytest.raises(TypeError):
        model.fit(data_statistics=_rot_cov(), max_epochs=2, show_progress=False)
    with pytest.raises(TypeError):
        model.get_class_distances(_rot_cov())


def test_fit_argument_errors():
    import sqfa_amd
    m3 = sqfa_amd.model.SecondMomentsSQFA(n_dim=8, feature_noise=0.001, n_filters=3)
    with pytest.raises(ValueError, match="even"):
        m3.fit(data_statistics=_rot_cov(), pairwise=True, max_epochs=2, show_progress=False)
    m2 = sqfa_amd.model.SecondMomentsSQFA(n_dim=8, n_filters=2)
    with pytest.raises(ValueError):
        m2.fit(max_epochs=2)
    with pytest.raises(ValueError):
        m2.fit_pca()
    with pytest.raises(TypeError):
        m2.fit(data_statistics=[1, 2, 3], max_epochs=2)
    with pytest.raises(ValueError):
        m2.fit(data_statistics={"means": torch.zeros(5, 8)}, max_epochs=2)
    with pytest.raises(ValueError):
        sqfa_amd.model.SecondMomentsSQFA(n_dim=3, n_filters=5)


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
@pytest.mark.parametrize("n_filters", [1, 2, 4])
@pytest.mark.parametrize("pairwise", [False, True])
def test_fit_runs_float32(model_name, n_filters, pairwise):
    import sqfa_amd
    torch.manual_seed(1)
    cov = _rot_cov()
    stats = {"means": torch.zeros(5, 8), "covariances": cov}
    cls = sqfa_amd.model.SQFA if model_name == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    model = cls(n_dim=8, feature_noise=0.01, n_filters=n_filters)
    if pairwise and n_filters % 2:
        with pytest.raises(ValueError):
            model.fit(data_statistics=stats, pairwise=True, max_epochs=3, show_progress=False)
        return
    loss, t = model.fit(data_statistics=stats, pairwise=pairwise, max_epochs=4, show_progress=False, return_loss=True)
    assert torch.isfinite(loss).all() and model.filters.shape == (n_filters, 8)
    assert sorted(model.state_dict()) == ["noise_mat", "parametrizations.filters.original"]
    assert model.transform(torch.randn(7, 8)).shape == (7, n_filters)
    assert model.transform_scatters(cov).shape == (5, n_filters, n_filters)


def test_orthogonal_constraint_keeps_filters_orthonormal():
    import sqfa_amd
    torch.manual_seed(3)
    stats = mc.fit_stats("syn", torch.float64, CPU)
    with mc.default_dtype(torch.float64):
        model = sqfa_amd.model.SQFA(n_dim=50, feature_noise=0.01, n_filters=3, constraint="orthogonal").double()
    loss, _ = model.fit(data_statistics=stats, max_epochs=3, show_progress=False, return_loss=True)
    F = model.filters.detach()
    assert torch.allclose(F @ F.T, torch.eye(3, dtype=torch.float64), atol=1e-10)
    assert loss[-1] <= loss[0]


def test_fit_from_points_and_nan_guard():
    import sqfa_amd
    g5 = mc.G5
    X = torch.tensor(g5["pts_X"], dtype=torch.float32)
    y = torch.tensor(g5["pts_y"])
    model = sqfa_amd.model.SQFA(n_dim=6, feature_noise=0.01, n_filters=2)
    model.fit_pca(X=X)
    assert rel_err(model.filters.detach(), sqfa_amd.statistics.pca(X, 2)) < 1e-6
    loss, _ = model.fit(X=X, y=y, max_epochs=3, show_progress=False, return_loss=True)
    assert torch.isfinite(loss).all()
    bad = sqfa_amd.model.SecondMomentsSQFA(n_dim=6, feature_noise=0.0, n_filters=2)
    S = torch.eye(6).repeat(4, 1, 1)
    S[1] = -S[1]
    with pytest.raises(ValueError, match="NaN"):
        bad.fit(data_statistics=S, max_epochs=2, show_progress=False)


# ---------------------------------------------------------------- statistics / linalg / other distances (G5)
def test_statistics_match_reference():
    from sqfa_amd import statistics
    g5 = mc.G5
    X = torch.tensor(g5["pts_X"])
    y = torch.tensor(g5["pts_y"])
    for est in ("empirical", "oas"):
        st = statistics.class_statistics(X, y, estimator=est)
        assert sorted(st) == ["covariances", "means", "second_moments"]
        for k, v in st.items():
            assert rel_err(v, g5[f"class_stats_{est}_{k}"]) < 1e-12
    assert rel_err(statistics.pca(X, 3), g5["pca_X_K3"]) < 1e-10
    assert rel_err(statistics.oas_covariance(X), g5["oas_cov"]) < 1e-12
    assert rel_err(statistics.sample_covariance(X), g5["sample_cov"]) < 1e-12
    rot = torch.tensor(g5["rotated_cov"])
    for K in (1, 2, 4, 8):
        assert rel_err(statistics.pca_from_scatter(rot, K), g5[f"pca_from_scatter_K{K}"]) < 1e-10
    with pytest.raises(ValueError):
        statistics.pca(X, 7)
    with pytest.raises(ValueError):
        statistics.pca_from_scatter(rot, 9)


@pytest.mark.parametrize("estimator", ["empirical", "oas"])
@pytest.mark.parametrize("batch_elements", [1 << 27, 4000])
def test_class_statistics_ragged_classes(estimator, batch_elements, monkeypatch):
    """Ragged class sizes through the padded-batch path (one or many groups) against the
    per-class definition (reference: statistics.py:8-54): centre, X^T X / (n-1), optional OAS."""
    from sqfa_amd import statistics
    monkeypatch.setattr(statistics, "_BATCH_ELEMENTS", batch_elements)
    g = torch.Generator().manual_seed(3)
    sizes = [5, 17, 200, 33, 2, 64, 65, 31, 400, 8]
    d = 12
    y = torch.cat([torch.full((n,), c) for c, n in enumerate(sizes)])
    X = torch.randn(len(y), d, generator=g, dtype=torch.float64) * 2.0 + torch.randn(d, generator=g, dtype=torch.float64)
    perm = torch.randperm(len(y), generator=g)
    X, y = X[perm], y[perm]
    st = statistics.class_statistics(X, y, estimator=estimator)
    for c in range(len(sizes)):
        pts = X[y == c]
        cov = statistics.sample_covariance(pts) if estimator == "empirical" else statistics.oas_covariance(pts)
        assert rel_err(st["means"][c], pts.mean(dim=0)) < 1e-13
        assert rel_err(st["covariances"][c], cov) < 1e-12
        assert rel_err(st["second_moments"][c], cov + torch.outer(pts.mean(dim=0), pts.mean(dim=0))) < 1e-12
    with pytest.raises(ValueError):
        statistics.class_statistics(X, y, estimator="ledoit")


def test_linalg_helpers_and_shapes():
    from sqfa_amd import distances, linalg
    g5 = mc.G5
    spd = torch.tensor(g5["spd"])
    assert rel_err(linalg.spd_sqrt(spd), g5["spd_sqrt"]) < 1e-12
    assert rel_err(linalg.spd_log(spd), g5["spd_log"]) < 1e-12
    W = linalg.spd_inv_sqrt(spd)
    assert rel_err(W @ spd @ W.transpose(1, 2), g5["spd_inv_sqrt_whitened"]) < 1e-10
    gv, ge = linalg.generalized_eigenvectors(spd[:3], spd[1:4])
    assert rel_err(ge, g5["gen_eigval"]) < 1e-10
    for i in range(3):
        for j in range(3):
            A, B, V, lam = spd[i], spd[1 + j], gv[i, j], ge[i, j]
            # defining properties for every pair: A v = lambda B v, unit-norm columns
            assert rel_err(A @ V, (B @ V) * lam) < 1e-9
            assert torch.allclose(torch.linalg.norm(V, dim=0), torch.ones(3, dtype=V.dtype), atol=1e-12)
            if i != 1 + j:  # (A_i == B_j gives a fully degenerate pencil: any basis is an answer)
                assert rel_err(V.abs(), g5["gen_eigvec_abs"][i, j]) < 1e-8
    for nA, nB, nd_d, nd_l in g5["squeeze_shapes"]:
        A, B = spd[:nA], spd[:nB]
        assert distances.affine_invariant_sq(A, B).dim() == nd_d
        assert linalg.generalized_eigenvalues(A, B).dim() == nd_l
    assert tuple(distances.affine_invariant_sq(spd[0], spd[:4]).shape) == tuple(g5["squeeze_2d_A"])
    with pytest.raises(ValueError):
        linalg.conjugate_matrix(spd, torch.ones(3))
    F = torch.randn(2, 3, dtype=torch.float64)
    assert linalg.conjugate_matrix(spd, F).shape == (4, 2, 2)
    assert linalg.conjugate_matrix(spd[0], F).shape == (2, 2)
    assert linalg.conjugate_matrix(spd, torch.stack([F, F])).shape == (4, 2, 2, 2)


def test_other_distance_operators():
    from sqfa_amd import distances
    g5 = mc.G5
    st = {"means": torch.tensor(g5["dist_mu"]), "covariances": torch.tensor(g5["dist_cov"])}
    assert rel_err(distances.log_euclidean_sq(st["covariances"], st["covariances"]), g5["log_euclidean_sq"]) < 1e-10
    assert rel_err(distances.log_euclidean(st["covariances"], st["covariances"]), g5["log_euclidean"]) < 1e-10
    for name in ("bhattacharyya", "mahalanobis_sq", "mahalanobis", "hellinger", "fisher_rao_same_cov"):
        # G5 was generated under a float64 default dtype; the reference's fisher_rao_same_cov takes
        # sqrt(2) from a DEFAULT-dtype tensor, so under this test's float32 default it is 1.7e-8 off
        assert rel_err(getattr(distances, name)(st, st), g5[name]) < (3e-8 if name == "fisher_rao_same_cov" else 1e-9), name
    assert sorted(distances.__all__) == sorted(
        ["affine_invariant_sq", "affine_invariant", "log_euclidean_sq", "log_euclidean", "fisher_rao_lower_bound",
         "fisher_rao_lower_bound_sq", "bhattacharyya", "mahalanobis_sq", "mahalanobis", "hellinger",
         "fisher_rao_same_cov"])


def test_custom_distance_fun_uses_generic_closure():
    import sqfa_amd
    from oracle import reference_path
    cov = torch.tensor(mc.G4["rotated_cov"], dtype=torch.float64)
    with mc.default_dtype(torch.float64):
        model = sqfa_amd.model.SecondMomentsSQFA(n_dim=8, n_filters=2, feature_noise=1e-3,
                                                 distance_fun=reference_path.affine_invariant).double()
    assert model._fused_closure_loss(cov) is None
    loss, _ = model.fit(data_statistics=cov, max_epochs=2, show_progress=False, return_loss=True)
    assert torch.isfinite(loss).all()


def test_usable_cpus_is_positive_and_bounded():
    import os
    from sqfa_amd.statistics import usable_cpus
    n = usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_generalized_eigenvalues_is_differentiable():
    """The reference's generalized_eigenvalues is autograd-transparent (src/sqfa/linalg.py:48-70) and
    the tutorial builds distance_funs on it (docs/source/tutorials/distances.md:127-178): the
    autograd plumbing (sort permutation, scatter of the upstream gradient, squeeze rules) against
    the reference's gradients of a weighted sum of eigenvalues (golden G1x)."""
    from conftest import load_golden, rel_err
    from sqfa_amd import linalg
    G1X = load_golden("g1x_airm_cross.npz")
    for nA, nB, m in [tuple(c) for c in G1X["cases"]]:
        key = f"A{nA}_B{nB}_m{m}"
        A = torch.tensor(G1X[f"{key}_A"], requires_grad=True)
        B = torch.tensor(G1X[f"{key}_B"], requires_grad=True)
        lam = linalg.generalized_eigenvalues(A, B)
        assert tuple(lam.shape) == G1X[f"{key}_lam_f64"].shape
        loss = (torch.tensor(G1X[f"{key}_Wlam"]) * lam).sum()
        gA, gB = torch.autograd.grad(loss, (A, B))
        assert rel_err(gA, G1X[f"{key}_gA_lam_f64"]) < 1e-8
        assert rel_err(gB, G1X[f"{key}_gB_lam_f64"]) < 1e-8


def test_other_operators_values_and_gradients_cpu_branch():
    """CPU tensors keep the torch expressions of the non-default operators: values and gradients
    against the reference (golden G5b) -- the GPU branch (native pair kernel) has the same test in
    tests/test_gpu_other_operators.py."""
    from conftest import load_golden
    from sqfa_amd import distances
    G5B = load_golden("g5b_other_operators.npz")
    for nA, nB, K in [tuple(int(v) for v in c) for c in G5B["cases"]][:4]:
        key = f"A{nA}_B{nB}_K{K}"
        for name in ("bhattacharyya", "mahalanobis", "fisher_rao_same_cov", "log_euclidean"):
            a = {"means": torch.tensor(G5B[f"{key}_muA"], requires_grad=True),
                 "covariances": torch.tensor(G5B[f"{key}_covA"], requires_grad=True)}
            b = a if not nB else {"means": torch.tensor(G5B[f"{key}_muB"], requires_grad=True),
                                  "covariances": torch.tensor(G5B[f"{key}_covB"], requires_grad=True)}
            fn = getattr(distances, name)
            D = fn(a["covariances"], b["covariances"]) if name.startswith("log_") else fn(a, b)
            assert rel_err(D.detach(), G5B[f"{key}_{name}_f64"]) < 1e-9, (key, name)
            loss = (torch.tensor(G5B[f"{key}_W"]).reshape(D.shape) * D).sum()
            (g,) = torch.autograd.grad(loss, [a["covariances"]])
            refg = G5B[f"{key}_{name}_gcovA_f64"]
            if np.isnan(refg).any():   # the reference's own gradient is NaN (acosh'(1) on the self-pair diagonal)
                assert torch.isnan(g).any()
                continue
            assert rel_err(g, refg) < 1e-7, (key, name)


def test_class_statistics_vs_reference_ragged_1000_classes():
    mc.check_class_statistics_vs_reference("cpu")


def test_dict_statistics_second_moments_are_formed_once():
    """_stats_to_scatter hands out the SAME tensor for the same (covariances, means) tensors and versions (the reference
    rebuilds cov + mu mu^T inside every call; a fresh tensor per call also re-ran the symmetry check of the
    native projection on every get_class_distances / transform_scatters call), and notices in-place edits."""
    from sqfa_amd import model as M
    g = torch.Generator().manual_seed(0)
    A = torch.randn(4, 6, 9, generator=g)
    stats = {"means": torch.randn(4, 6, generator=g), "covariances": A @ A.transpose(1, 2)}
    a = M._stats_to_scatter(stats)
    b = M._stats_to_scatter(dict(stats))              # another dict, the same tensors
    assert a is b
    assert torch.equal(a, stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :])
    stats["means"].mul_(2.0)                          # in-place edit: version changes, the sum is rebuilt
    c = M._stats_to_scatter(stats)
    assert c is not a and torch.equal(c, stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :])
    raw = torch.eye(3).repeat(2, 1, 1)
    assert M._stats_to_scatter(raw) is raw            # tensors pass through
    tracked = {"means": stats["means"].clone().requires_grad_(), "covariances": stats["covariances"]}
    assert M._stats_to_scatter(tracked).requires_grad  # autograd-tracked inputs are never cached


def test_sharded_closure_eager_pass_does_not_disturb_the_captured_graphs():
    """ShardedClosure.run(eager=True) after the capture (bench.py's profiling pass) must leave the box bound to the tensors
    the captured graphs write (it returned and all-reduced the stale eager tensors afterwards).  The stage /
    graph mechanics with stand-ins for the HIP graphs: a 'graph' re-runs its stage's arithmetic INTO the tensors that were
    bound when it was captured, exactly what a replay does."""
    from sqfa_amd._optim import GraphRunner, ShardedClosure
    sc = ShardedClosure.__new__(ShardedClosure)
    x = torch.zeros(3)
    box = {}

    def compute():                 # like stage_backward: binds a fresh tensor
        box["grad"] = x * 2.0

    def collective():              # like reduce_grad: reads the box at call time
        box["grad"] += 1.0

    def pack():
        box["packed"] = box["grad"] + 0.0

    class FakeGraph:
        """Captured at construction: reads the tensors bound THEN (`reads`), writes into the tensors it produced THEN."""

        def __init__(self, fn, reads, writes):
            self.reads = {n: box[n] for n in reads}
            fn()
            self.bound = {n: box[n] for n in writes}
            self.fn = fn

        def replay(self):            # like a HIP graph: fixed addresses in, fixed addresses out, the box is not touched
            saved = dict(box)
            box.update(self.reads)
            self.fn()
            for n, t in self.bound.items():
                t.copy_(box[n])
            box.clear()
            box.update(saved)

    sc.runner = GraphRunner([compute, collective, pack], box, eager_stages=(1,))
    sc.runner.calls = 99
    x.fill_(1.0)
    graphs = [FakeGraph(compute, [], ["grad"]), None]
    collective()
    graphs.append(FakeGraph(pack, ["grad"], ["packed"]))
    sc.runner.graphs, sc.runner.state = graphs, "on"
    packed, grad = sc.run()
    assert packed.tolist() == [3.0] * 3
    x.fill_(5.0)
    e_packed, e_grad = sc.run(eager=True)
    assert e_packed.tolist() == [11.0] * 3
    assert box["grad"] is graphs[0].bound["grad"] and box["packed"] is graphs[2].bound["packed"]   # the capture-time tensors again
    x.fill_(7.0)
    packed, grad = sc.run()
    assert packed.tolist() == [15.0] * 3 and grad.tolist() == [15.0] * 3
    assert packed is graphs[2].bound["packed"]
