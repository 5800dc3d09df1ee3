"""CPU tests of sqfa_amd.divergences: the module's names, the direct calls (plain torch expressions in the explicit-difference
form) against the textbook form of tests/jeffreys_oracle.py in float64, the closure plan of both models, and a CPU fit
through the generic closure."""
import itertools

import pytest
import torch

import jeffreys_oracle as jo

NAMES = ["jeffreys", "jeffreys_root", "jeffreys_spd", "jeffreys_spd_root"]


def test_module_names():
    import sqfa_amd
    from sqfa_amd import distances, divergences, transport
    assert divergences.__all__ == NAMES
    assert "divergences" in sqfa_amd.__all__
    for name in NAMES:
        assert name not in distances.__all__ and name not in transport.__all__
        assert distances.fused_spec(getattr(divergences, name)) is None           # no pair-kernel operators
        assert distances.class_fused_spec(getattr(divergences, name)) is None
        assert getattr(divergences, name) not in distances._FUSED.values() and name not in distances._FUSED
    assert divergences.JEFFREYS_FUSED_CLOSURE is True
    assert divergences.fused_spec(divergences.jeffreys) == ("gaussian", False)
    assert divergences.fused_spec(divergences.jeffreys_root) == ("gaussian", True)
    assert divergences.fused_spec(divergences.jeffreys_spd) == ("spd", False)
    assert divergences.fused_spec(divergences.jeffreys_spd_root) == ("spd", True)
    assert divergences.fused_spec(distances.bhattacharyya) is None
    assert divergences.fused_spec(lambda A, B: None) is None


def test_direct_calls_match_the_textbook_form():
    from sqfa_amd import divergences
    mu, cov = jo.make_classes(5, 4, seed=11)
    stats = {"means": mu, "covariances": cov}
    want = jo.textbook(mu, cov, mu, cov)
    J = divergences.jeffreys(stats, stats)
    assert J.shape == (5, 5) and J.dtype == torch.float64
    assert (J - want).abs().max() <= 1e-12
    assert J.min() >= -1e-12
    assert (J - J.t()).abs().max() <= 1e-12
    assert torch.equal(J.diagonal(), torch.zeros(5, dtype=torch.float64))         # differences of a class with itself
    R = divergences.jeffreys_root(stats, stats)
    assert (R - torch.sqrt(want + 1e-6)).abs().max() <= 1e-12
    assert torch.equal(R.diagonal(), torch.full((5,), 1e-6, dtype=torch.float64).sqrt())
    # the means-free operators are the Gaussian ones with zero means
    zero = {"means": torch.zeros_like(mu), "covariances": cov}
    assert (divergences.jeffreys_spd(cov, cov) - divergences.jeffreys(zero, zero)).abs().max() <= 1e-12
    assert (divergences.jeffreys_spd(cov, cov) - jo.textbook(None, cov, None, cov)).abs().max() <= 1e-12
    assert (divergences.jeffreys_spd_root(cov, cov) - divergences.jeffreys_root(zero, zero)).abs().max() <= 1e-12
    # the cross case, and walking A in chunks gives the same values
    sB = {"means": mu[:2] + 0.1, "covariances": cov[3:]}
    Jc = divergences.jeffreys(stats, sB)
    assert Jc.shape == (5, 2)
    assert (Jc - jo.textbook(mu, cov, sB["means"], sB["covariances"])).abs().max() <= 1e-12
    old = divergences._CHUNK_ELEMENTS
    try:
        divergences._CHUNK_ELEMENTS = 2 * 2 * 16      # two rows of A at a time
        assert torch.equal(divergences.jeffreys(stats, sB), Jc)
    finally:
        divergences._CHUNK_ELEMENTS = old


def test_squeeze_shapes():
    from sqfa_amd import divergences
    mu, cov = jo.make_classes(4, 3, seed=5)
    stats = {"means": mu, "covariances": cov}
    one = {"means": mu[0], "covariances": cov[0]}
    for fn in (divergences.jeffreys, divergences.jeffreys_root):
        assert fn(stats, stats).shape == (4, 4)
        assert fn(one, stats).shape == (4,)
        assert fn(stats, one).shape == (4,)
        assert fn(one, one).shape == ()
    for fn in (divergences.jeffreys_spd, divergences.jeffreys_spd_root):
        assert fn(cov, cov).shape == (4, 4)
        assert fn(cov[0], cov).shape == (4,)
        assert fn(cov, cov[:1]).shape == (4,)
        assert fn(cov[1], cov[2]).shape == ()
    assert divergences.jeffreys(stats, stats).dtype == torch.float64
    assert divergences.jeffreys_spd(cov.float(), cov.float()).dtype == torch.float32


def test_gradcheck():
    from sqfa_amd import divergences
    mu, cov = jo.make_classes(3, 3, seed=2)
    mu.requires_grad_(True)
    cov.requires_grad_(True)
    for fn in (divergences.jeffreys, divergences.jeffreys_root):
        def f(mu_, cov_):
            s = {"means": mu_, "covariances": cov_}
            D = fn(s, s)
            r, c = torch.tril_indices(3, 3, offset=-1)
            return D[r, c]            # the diagonal of the root form sits at sqrt(eps): its slope is not what a fit uses
        assert torch.autograd.gradcheck(f, (mu, cov))
    for fn in (divergences.jeffreys_spd, divergences.jeffreys_spd_root):
        def g(cov_):
            D = fn(cov_, cov_)
            r, c = torch.tril_indices(3, 3, offset=-1)
            return D[r, c]
        assert torch.autograd.gradcheck(g, (cov,))


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
    from sqfa_amd import divergences
    from sqfa_amd.parallel import PairShard
    stats = _tiny_statistics()
    cls = sqfa_amd.model.SQFA if model_name == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    torch.manual_seed(1)
    model = cls(n_dim=4, n_filters=2, feature_noise=0.01, distance_fun=getattr(divergences, fn_name))
    prepared = model._prepare_statistics(stats if model_name == "sqfa" else stats["covariances"])
    matched = (model_name == "sqfa") == (fn_name in ("jeffreys", "jeffreys_root"))
    for pair_sharded, class_sharded, switch in itertools.product((False, True), repeat=3):
        case = (model_name, fn_name, pair_sharded, class_sharded, switch)
        model.pair_shard = PairShard(rank=0, world_size=1) if pair_sharded else None
        model.class_shard = OneRankClassShard() if class_sharded else None
        monkeypatch.setattr(divergences, "JEFFREYS_FUSED_CLOSURE", switch)
        bare, full = model._closure_plan(), model._closure_plan(prepared)
        assert model._has_fused_closure() == (bare is not None), case
        if matched and switch and not pair_sharded and not class_sharded:
            assert bare is not None and bare.evaluator == "jeffreys", case
            assert bare.sqrt_mode is fn_name.endswith("_root"), case
            assert bare.weight is None and bare.inputs is None, case
        else:
            assert bare is None, case
        assert full is None, case                   # CPU statistics: the generic closure
        assert model._fused_closure_loss(prepared) is None, case


def test_limits_of_the_plan():
    import sqfa_amd
    from sqfa_amd import _native, divergences
    SM, SQ = sqfa_amd.model.SecondMomentsSQFA, sqfa_amd.model.SQFA
    assert _native.JEFFREYS_MAX_DIM == 64
    assert SQ(n_dim=80, n_filters=64, distance_fun=divergences.jeffreys)._has_fused_closure()
    assert not SQ(n_dim=80, n_filters=65, distance_fun=divergences.jeffreys)._has_fused_closure()
    assert SM(n_dim=80, n_filters=64, distance_fun=divergences.jeffreys_spd_root).double()._has_fused_closure()
    assert not SM(n_dim=80, n_filters=65, distance_fun=divergences.jeffreys_spd)._has_fused_closure()
    assert not SM(n_dim=6, n_filters=2, distance_fun=divergences.jeffreys_spd).half()._has_fused_closure()
    assert SQ(n_dim=6, n_filters=2, distance_fun=divergences.jeffreys, constraint="orthogonal")._has_fused_closure()


def test_native_call_refuses_cpu_tensors():
    from sqfa_amd import _native
    mu, cov = jo.make_classes(3, 2, seed=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.hip_jeffreys_pairwise_loss(mu, cov, False, 1e-6, -0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.ClassPairLoss.apply(None, cov, "jeffreys", True, 1e-6, -0.1)


@pytest.mark.parametrize("fn_name", NAMES)
def test_cpu_fit_runs_the_generic_closure(fn_name):
    import sqfa_amd
    from sqfa_amd import divergences
    stats = _tiny_statistics()
    torch.manual_seed(4)
    gaussian = fn_name in ("jeffreys", "jeffreys_root")
    cls = sqfa_amd.model.SQFA if gaussian else sqfa_amd.model.SecondMomentsSQFA
    model = cls(n_dim=4, n_filters=2, feature_noise=0.01, distance_fun=getattr(divergences, fn_name))
    loss, _ = model.fit(data_statistics=stats if gaussian else stats["covariances"], max_epochs=2, show_progress=False,
                        return_loss=True)
    assert loss.shape == (2,) and torch.isfinite(loss).all() and loss[-1] < loss[0]
    D = model.get_class_distances(stats if gaussian else stats["covariances"])
    assert D.shape == (3, 3) and torch.isfinite(D).all()
