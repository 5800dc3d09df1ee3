"""CPU tests of sqfa_amd.logdet: the module's names, the direct calls (plain torch expressions) against the generalised-
eigenvalue route of tests/stein_oracle.py in float64, autograd against the oracle's closed-form gradient, the closure plan
of both models, and a CPU fit through the generic closure."""
import itertools

import numpy as np
import pytest
import torch

import stein_oracle as so

NAMES = ["stein", "stein_root"]


def _classes(n, m, seed):
    return torch.from_numpy(so.make_classes(n, m, seed))


def test_module_names():
    import sqfa_amd
    from sqfa_amd import _native, distances, divergences, logdet, transport
    assert logdet.__all__ == NAMES
    assert "logdet" in sqfa_amd.__all__ and sqfa_amd.logdet is logdet
    for name in NAMES:
        fn = getattr(logdet, name)
        assert name not in distances.__all__ and name not in transport.__all__ and name not in divergences.__all__
        assert distances.fused_spec(fn) is None and fn not in distances._FUSED          # no pair-kernel operators
        assert distances.class_fused_spec(fn) is None and divergences.fused_spec(fn) is None
    assert logdet.STEIN_FUSED_CLOSURE is True
    assert distances.class_pair_spec(logdet.stein) == ("stein", "spd", False)
    assert distances.class_pair_spec(logdet.stein_root) == ("stein", "spd", True)
    assert logdet.fused_spec(logdet.stein) == ("spd", False) and logdet.fused_spec(logdet.stein_root) == ("spd", True)
    assert logdet.fused_spec(distances.log_euclidean) is None and logdet.fused_spec(lambda A, B: None) is None
    fam = _native.pair_family("stein")
    assert _native.STEIN_MAX_DIM == fam.limit == 64 and fam.means is False
    assert fam.entry == fam.name == "sqfa_stein_pairwise_loss" and fam.query == "sqfa_stein_workspace_bytes"
    assert "Stein" in fam.size_error.format(m=65, limit=64)
    assert _native.pair_family("jeffreys") is _native.PAIR_FAMILIES["jeffreys"]


def test_direct_calls_match_the_oracle():
    from sqfa_amd import distances, logdet
    S = _classes(5, 4, seed=11)
    want = so.stein_eigenvalues(S.numpy(), S.numpy())
    D = logdet.stein(S, S)
    assert D.shape == (5, 5) and D.dtype == torch.float64
    assert np.abs(D.numpy() - want).max() <= 1e-12
    assert np.abs(D.numpy() - so.three_logdets(S.numpy(), S.numpy())).max() <= 1e-12
    assert D.min() >= -1e-12
    assert (D - D.t()).abs().max() <= 1e-12
    assert torch.equal(D.diagonal(), torch.zeros(5, dtype=torch.float64))           # (S + S)/2 is S: the same factor
    # twice the Bhattacharyya distance of the zero-mean Gaussians
    zero = {"means": torch.zeros(5, 4, dtype=torch.float64), "covariances": S}
    assert (D - 2 * distances.bhattacharyya(zero, zero)).abs().max() <= 1e-12
    R = logdet.stein_root(S, S)
    assert np.abs(R.numpy() - np.sqrt(np.abs(want) + 1e-6)).max() <= 1e-12
    assert torch.equal(R, torch.sqrt(torch.abs(D) + 1e-6))
    assert torch.equal(R.diagonal(), torch.full((5,), 1e-6, dtype=torch.float64).sqrt())
    # the cross case, and walking A in chunks gives the same values
    B = _classes(3, 4, seed=12)
    Dc = logdet.stein(S, B)
    assert Dc.shape == (5, 3)
    assert np.abs(Dc.numpy() - so.stein_eigenvalues(S.numpy(), B.numpy())).max() <= 1e-12
    old = logdet._CHUNK_ELEMENTS
    try:
        logdet._CHUNK_ELEMENTS = 2 * 3 * 16      # two rows of A at a time
        assert torch.equal(logdet.stein(S, B), Dc)
        assert torch.equal(logdet.stein_root(S, B), torch.sqrt(torch.abs(Dc) + 1e-6))
    finally:
        logdet._CHUNK_ELEMENTS = old


def test_squeeze_shapes_and_dtypes():
    from sqfa_amd import logdet
    S = _classes(4, 3, seed=5)
    for fn in (logdet.stein, logdet.stein_root):
        assert fn(S, S).shape == (4, 4)
        assert fn(S[0], S).shape == (4,)
        assert fn(S, S[:1]).shape == (4,)
        assert fn(S[1], S[2]).shape == ()
        assert fn(S, S).dtype == torch.float64 and fn(S.float(), S.float()).dtype == torch.float32


def test_indefinite_matrix_gives_nan():
    from sqfa_amd import logdet
    S = _classes(3, 3, seed=6)
    S[1] = torch.diag(torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64))
    D = logdet.stein(S, S)
    assert torch.isnan(D[1]).all() and torch.isnan(D[:, 1]).all()
    assert torch.isfinite(D[0, 2]) and torch.isfinite(D[2, 0])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_autograd_matches_the_closed_form(name, weighted):
    from sqfa_amd import logdet
    n, m = 5, 4
    S = _classes(n, m, seed=21)
    W = so.make_weights(n, seed=3) if weighted else None
    weight = -1.0 / (n * (n - 1) // 2)
    want = so.loss_and_gradient(S.numpy(), name == "stein_root", weight, W)
    Sv = S.clone().requires_grad_(True)
    D = getattr(logdet, name)(Sv, Sv)
    r, c = torch.tril_indices(n, n, offset=-1)
    w = torch.from_numpy(W)[r, c] if weighted else weight
    loss = (w * D[r, c]).sum()
    (g,) = torch.autograd.grad(loss, Sv)
    g = 0.5 * (g + g.transpose(1, 2))
    assert abs(loss.item() - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"]))
    assert so.max_rel(g.numpy(), want["grad"]) <= 1e-11
    # the oracle's closed form against central differences of its own loss
    h, E = 1e-6, np.zeros((n, m, m))
    E[2, 1, 3] = E[2, 3, 1] = 1.0
    up = so.loss_and_gradient(S.numpy() + h * E, name == "stein_root", weight, W)["loss"]
    dn = so.loss_and_gradient(S.numpy() - h * E, name == "stein_root", weight, W)["loss"]
    assert abs((up - dn) / (2 * h) - 2 * want["grad"][2, 1, 3]) <= 1e-7 * max(1.0, abs(want["grad"]).max())


def test_float32_yardstick_is_close_to_the_oracle():
    S = so.make_classes(6, 8, seed=4).astype(np.float32)
    want = so.loss_and_gradient(S.astype(np.float64), True, -0.1)
    yard = so.loss_and_gradient(S, True, -0.1, dtype=np.float32)
    assert yard["dist"].dtype == np.float32 and yard["grad"].dtype == np.float32
    for name in ("loss", "dist", "grad"):
        assert 0 < so.max_rel(yard[name], want[name]) <= 1e-4, name


# ---------------------------------------------------------------------------------------------------------------------
class OneRankClassShard:
    """sqfa_amd.parallel.ClassShard of a one-rank group, without a process group."""
    rank, world_size, offset, counts, n_classes, group = 0, 1, 0, [3], 3, None

    def gather(self, S_local):
        return S_local

    def reduce_gradients(self, parameters):
        pass


def _tiny_statistics():
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 4, 6, generator=g)
    return {"means": 0.3 * torch.randn(3, 4, generator=g), "covariances": A @ A.transpose(1, 2) / 6 + 0.1 * torch.eye(4)}


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
@pytest.mark.parametrize("fn_name", NAMES)
def test_closure_plan(model_name, fn_name, monkeypatch):
    import sqfa_amd
    from sqfa_amd import logdet
    from sqfa_amd.parallel import PairShard
    stats = _tiny_statistics()
    cls = sqfa_amd.model.SQFA if model_name == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    torch.manual_seed(1)
    model = cls(n_dim=4, n_filters=2, feature_noise=0.01, distance_fun=getattr(logdet, fn_name))
    prepared = model._prepare_statistics(stats if model_name == "sqfa" else stats["covariances"])
    for pair_sharded, class_sharded, switch in itertools.product((False, True), repeat=3):
        case = (model_name, fn_name, pair_sharded, class_sharded, switch)
        model.pair_shard = PairShard(rank=0, world_size=1) if pair_sharded else None
        model.class_shard = OneRankClassShard() if class_sharded else None
        monkeypatch.setattr(logdet, "STEIN_FUSED_CLOSURE", switch)
        bare, full = model._closure_plan(), model._closure_plan(prepared)
        assert model._has_fused_closure() == (bare is not None), case
        if model_name == "smsqfa" and switch and not pair_sharded and not class_sharded:
            assert bare is not None and bare.evaluator == "stein", case
            assert bare.sqrt_mode is (fn_name == "stein_root"), case
            assert bare.weight is None and bare.inputs is None and bare.metric is None, case
        else:
            assert bare is None, case               # SQFA takes dict statistics: these are SPD-batch operators
        assert full is None, case                   # CPU statistics: the generic closure
        assert model._fused_closure_loss(prepared) is None, case


def test_limits_of_the_plan():
    import sqfa_amd
    from sqfa_amd import logdet
    SM = sqfa_amd.model.SecondMomentsSQFA
    assert SM(n_dim=80, n_filters=64, distance_fun=logdet.stein)._has_fused_closure()
    assert SM(n_dim=80, n_filters=64, distance_fun=logdet.stein_root).double()._has_fused_closure()
    assert not SM(n_dim=80, n_filters=65, distance_fun=logdet.stein)._has_fused_closure()
    assert not SM(n_dim=80, n_filters=65, distance_fun=logdet.stein_root)._has_fused_closure()
    assert not SM(n_dim=6, n_filters=2, distance_fun=logdet.stein).half()._has_fused_closure()
    assert SM(n_dim=6, n_filters=2, distance_fun=logdet.stein, constraint="orthogonal")._has_fused_closure()


def test_other_families_are_untouched_by_the_stein_switch(monkeypatch):
    import sqfa_amd
    from sqfa_amd import distances, divergences, logdet, transport
    SM, SQ = sqfa_amd.model.SecondMomentsSQFA, sqfa_amd.model.SQFA
    models = [SM(n_dim=6, n_filters=2, distance_fun=fn) for fn in
              (distances.affine_invariant, distances.log_euclidean, divergences.jeffreys_spd, transport.bures_wasserstein)]
    models += [SQ(n_dim=6, n_filters=2, distance_fun=fn) for fn in
               (distances.fisher_rao_lower_bound, distances.bhattacharyya, divergences.jeffreys_root)]
    before = [m._closure_plan() for m in models]
    assert all(plan is not None for plan in before)
    monkeypatch.setattr(logdet, "STEIN_FUSED_CLOSURE", False)
    assert [m._closure_plan() for m in models] == before
    assert distances.class_pair_spec(logdet.stein) is None and distances.class_pair_spec(logdet.stein_root) is None
    assert distances.class_pair_spec(divergences.jeffreys) == ("jeffreys", "gaussian", False)


def test_native_call_refuses_cpu_tensors():
    from sqfa_amd import _native
    S = _classes(3, 2, seed=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.hip_stein_pairwise_loss(S, False, 1e-6, -0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.ClassPairLoss.apply(None, S, "stein", True, 1e-6, -0.1)


@pytest.mark.parametrize("fn_name", NAMES)
def test_cpu_fit_runs_the_generic_closure(fn_name):
    import sqfa_amd
    from sqfa_amd import logdet
    stats = _tiny_statistics()
    torch.manual_seed(4)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=4, n_filters=2, feature_noise=0.01, distance_fun=getattr(logdet, fn_name))
    loss, _ = model.fit(data_statistics=stats["covariances"], max_epochs=2, show_progress=False, return_loss=True)
    assert loss.shape == (2,) and torch.isfinite(loss).all() and loss[-1] < loss[0]
    D = model.get_class_distances(stats["covariances"])
    assert D.shape == (3, 3) and torch.isfinite(D).all()
