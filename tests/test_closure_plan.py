"""CPU tests of the closure plan (model._closure_plan): the ONE decision of which fused evaluator a model's closure runs.
Whatever arms the graph capture (_has_fused_closure) is the plan without statistics; whatever the plan with statistics
names, _fused_closure_loss evaluates.  Tiny CPU statistics (C=3, D=4, K=2) with the oracle as pair backend."""
import itertools

import pytest
import torch

from oracle_backend import oracle_pair_backend


@pytest.fixture(autouse=True)
def _oracle_backend(monkeypatch):
    from sqfa_amd import _native

    def backend(A, B, metric="airm", **kw):   # the oracle knows the affine-invariant metric only: enough for "a pair comes back"
        return oracle_pair_backend(A, B, **kw)

    monkeypatch.setattr(_native, "_pair_backend", backend)


def _operators():
    from sqfa_amd import distances, divergences, transport
    ops = {name: getattr(distances, name) for name in distances.__all__}
    ops.update({name: getattr(transport, name) for name in transport.__all__})
    ops.update({name: getattr(divergences, name) for name in divergences.__all__})
    ops["custom"] = lambda A, B: distances.affine_invariant(A, B)
    return ops


OPERATORS = ["affine_invariant_sq", "affine_invariant", "log_euclidean_sq", "log_euclidean", "fisher_rao_lower_bound",
             "fisher_rao_lower_bound_sq", "bhattacharyya", "mahalanobis_sq", "mahalanobis", "hellinger", "fisher_rao_same_cov",
             "bures_wasserstein_sq", "bures_wasserstein", "wasserstein_sq", "wasserstein", "jeffreys", "jeffreys_root",
             "jeffreys_spd", "jeffreys_spd_root", "custom"]

# (model, distance_fun) -> (evaluator of the plan without statistics, with these CPU statistics), unsharded, every switch
# on; every pair that is not listed has no fused closure.  The class-pair evaluators (Gaussian, log-Euclidean, Jeffreys) are
# GPU-only: on CPU tensors the plan with statistics is None (the generic closure), while the pair kernels' chain reaches
# _pair_backend.
PLANS = {
    ("smsqfa", "affine_invariant_sq"): ("chain", "chain"),
    ("smsqfa", "affine_invariant"): ("chain", "chain"),
    ("smsqfa", "bures_wasserstein_sq"): ("chain", "chain"),
    ("smsqfa", "bures_wasserstein"): ("chain", "chain"),
    ("smsqfa", "log_euclidean_sq"): ("log_euclidean", None),
    ("smsqfa", "log_euclidean"): ("log_euclidean", None),
    ("sqfa", "fisher_rao_lower_bound_sq"): ("chain", "chain"),
    ("sqfa", "fisher_rao_lower_bound"): ("chain", "chain"),
    ("sqfa", "bhattacharyya"): ("gauss", None),
    ("sqfa", "mahalanobis_sq"): ("gauss", None),
    ("sqfa", "mahalanobis"): ("gauss", None),
    ("sqfa", "hellinger"): ("gauss", None),
    ("sqfa", "jeffreys"): ("jeffreys", None),
    ("sqfa", "jeffreys_root"): ("jeffreys", None),
    ("smsqfa", "jeffreys_spd"): ("jeffreys", None),
    ("smsqfa", "jeffreys_spd_root"): ("jeffreys", None),
}
SINGLE_PROCESS_ONLY = {"gauss": "GAUSS_FUSED_CLOSURE", "log_euclidean": "LOG_EUCLIDEAN_FUSED_CLOSURE",
                       "jeffreys": "JEFFREYS_FUSED_CLOSURE"}   # evaluator -> its switch


class OneRankClassShard:
    """sqfa_amd.parallel.ClassShard of a one-rank group, without a process group."""
    rank, world_size, offset, counts, n_classes, group = 0, 1, 0, [3], 3, None

    def gather(self, S_local):
        return S_local

    def reduce_gradients(self, parameters):
        pass


def test_the_operator_list_is_complete():
    assert sorted(OPERATORS) == sorted(_operators())


@pytest.mark.parametrize("model_name", ["smsqfa", "sqfa"])
@pytest.mark.parametrize("fn_name", OPERATORS)
def test_plan_arms_and_evaluates_consistently(model_name, fn_name, monkeypatch):
    import sqfa_amd
    from sqfa_amd import distances, divergences
    from sqfa_amd.parallel import PairShard
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 4, 6, generator=g)
    stats = {"means": 0.3 * torch.randn(3, 4, generator=g), "covariances": A @ A.transpose(1, 2) / 6 + 0.1 * torch.eye(4)}
    cls = sqfa_amd.model.SQFA if model_name == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    torch.manual_seed(1)
    model = cls(n_dim=4, n_filters=2, feature_noise=0.01, distance_fun=_operators()[fn_name])
    prepared = model._prepare_statistics(stats if model_name == "sqfa" else stats["covariances"])
    for pair_sharded, class_sharded, gauss_on, log_on, jeffreys_on in itertools.product((False, True), repeat=5):
        case = (model_name, fn_name, pair_sharded, class_sharded, gauss_on, log_on, jeffreys_on)
        model.pair_shard = PairShard(rank=0, world_size=1) if pair_sharded else None
        model.class_shard = OneRankClassShard() if class_sharded else None
        monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", gauss_on)
        monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", log_on)
        monkeypatch.setattr(divergences, "JEFFREYS_FUSED_CLOSURE", jeffreys_on)
        bare, full = model._closure_plan(), model._closure_plan(prepared)
        assert model._has_fused_closure() == (bare is not None), case
        assert full is None or bare is not None, case          # statistics only ever take a fused closure away
        out = model._fused_closure_loss(prepared)
        if full is None:
            assert out is None, case
        else:
            loss, flags = out
            assert loss.dim() == 0 and torch.isfinite(loss) and flags.tolist() == [0, 0], case
            assert full.weight == -1.0 / 3 and full.shard == (0, 1), case
        expected = PLANS.get((model_name, fn_name), (None, None))
        switch = SINGLE_PROCESS_ONLY.get(expected[0])
        if switch is not None and (pair_sharded or class_sharded or not {"GAUSS_FUSED_CLOSURE": gauss_on,
                                                                         "LOG_EUCLIDEAN_FUSED_CLOSURE": log_on,
                                                                         "JEFFREYS_FUSED_CLOSURE": jeffreys_on}[switch]):
            expected = (None, None)
        assert (bare and bare.evaluator, full and full.evaluator) == expected, case
        if bare is not None and bare.evaluator == "jeffreys":
            assert bare.sqrt_mode is fn_name.endswith("_root"), case
            assert bare.weight is None and bare.inputs is None, case


def test_cpu_models_keep_the_chain():
    """A CPU model with a native distance_fun evaluates through PairwiseLoss and _pair_backend, never the single node."""
    import sqfa_amd
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=4, n_filters=2, feature_noise=0.01)
    S = torch.eye(4).repeat(3, 1, 1) * torch.tensor([1.0, 2.0, 3.0])[:, None, None]
    plan = model._closure_plan(S)
    assert plan.evaluator == "chain" and plan.inputs is None and plan.metric == "airm" and plan.sqrt_mode is True


# operator -> (family, input kind, mode) of distances.class_pair_spec, and the module and switch of each family
def _class_pair_table():
    from sqfa_amd import _lib, distances, divergences
    return {
        distances.bhattacharyya: ("gauss", "gaussian", _lib.SQFA_GAUSS_BHATTACHARYYA),
        distances.hellinger: ("gauss", "gaussian", _lib.SQFA_GAUSS_HELLINGER),
        distances.mahalanobis_sq: ("gauss", "gaussian", _lib.SQFA_GAUSS_MAHALANOBIS_SQ),
        distances.mahalanobis: ("gauss", "gaussian", _lib.SQFA_GAUSS_MAHALANOBIS),
        distances.log_euclidean: ("log_euclidean", "spd", True),
        distances.log_euclidean_sq: ("log_euclidean", "spd", False),
        divergences.jeffreys: ("jeffreys", "gaussian", False),
        divergences.jeffreys_root: ("jeffreys", "gaussian", True),
        divergences.jeffreys_spd: ("jeffreys", "spd", False),
        divergences.jeffreys_spd_root: ("jeffreys", "spd", True),
    }


def _old_lookups(fn):
    """What the three per-family lookups returned before class_pair_spec existed, with every switch on."""
    from sqfa_amd import distances, divergences
    return (distances.fused_spec(fn), distances.class_fused_spec(fn), divergences.fused_spec(fn))


def test_class_pair_spec_is_the_one_registry(monkeypatch):
    from sqfa_amd import _native, distances, divergences
    table = _class_pair_table()
    switches = {"gauss": (distances, "GAUSS_FUSED_CLOSURE"), "log_euclidean": (distances, "LOG_EUCLIDEAN_FUSED_CLOSURE"),
                "jeffreys": (divergences, "JEFFREYS_FUSED_CLOSURE")}
    assert set(switches) == set(_native.PAIR_FAMILIES) == {family for family, _, _ in table.values()}
    # every operator one of the three old lookups knows maps to exactly one family, with the documented (kind, mode) ...
    for name, fn in _operators().items():
        gauss, log_euclidean, jeffreys = _old_lookups(fn)
        known = [gauss is not None and gauss[3] == "gauss", log_euclidean is not None, jeffreys is not None]
        assert sum(known) == (1 if fn in table else 0), name
        assert distances.class_pair_spec(fn) == table.get(fn), name
        spec = distances.class_pair_spec(fn)
        assert spec is None or (type(spec[2]) is bool) == (spec[0] != "gauss"), name
    assert distances.class_pair_spec(lambda A, B: None) is None
    # ... and the old lookups return today's tuples
    sqrt_mode = {distances.bhattacharyya: False, distances.hellinger: True, distances.mahalanobis_sq: False,
                 distances.mahalanobis: True}
    for fn, (family, kind, mode) in table.items():
        expected = {"gauss": ((kind, mode, sqrt_mode.get(fn), "gauss"), None, None), "log_euclidean": (None, (kind, mode), None),
                    "jeffreys": (None, None, (kind, mode))}[family]
        assert _old_lookups(fn) == expected, fn.__name__
    assert distances.fused_spec(distances.affine_invariant) == ("spd", 1.0, True, "airm")
    assert distances.fused_spec(distances.fisher_rao_lower_bound_sq) == ("gaussian", 0.5, False, "airm")
    # each switch turned off removes its family and no other, from the new lookup and from the old ones
    for off, (module, attribute) in switches.items():
        with monkeypatch.context() as patch:
            patch.setattr(module, attribute, False)
            for fn, spec in table.items():
                gone = spec[0] == off
                assert distances.class_pair_spec(fn) == (None if gone else spec), (off, fn.__name__)
                assert any(v is not None for v in _old_lookups(fn)) == (not gone), (off, fn.__name__)
            assert distances.fused_spec(distances.affine_invariant) == ("spd", 1.0, True, "airm")
        assert all(distances.class_pair_spec(fn) == spec for fn, spec in table.items())
