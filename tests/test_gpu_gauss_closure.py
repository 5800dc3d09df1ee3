"""GPU tests of the fused Gaussian pair closure: sqfa_gauss_pairwise_loss (fused mode of the Gaussian pair kernels),
_native.ClassPairLoss (family "gauss") and SQFA's closure with bhattacharyya / hellinger / mahalanobis_sq / mahalanobis as
distance_fun, against the reference's values (golden G8, tests/golden/make_golden_gauss_closure.py) and a float64 torch
expression of the definitions (tests/gauss_oracle.py).

Tolerances (the rule of tests/test_gpu_other_operators.py): float64 1e-9 (values) / 1e-8 (gradients; Hellinger
gradients 1e-6); float32 max(1e-5, 5 x the reference's own float32-vs-float64 deviation on that case, G8's f32 keys).

5-epoch float64 loss trajectory (test_fit_trajectory_vs_reference): the fused path may deviate from the golden by
5 x the generic path's own deviation, with a floor of 1e-8 relative; both are measured in the test and printed."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from gauss_oracle import _full_expression, _rows_D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G8 = load_golden("g8_gauss_closure.npz")
CASES = [tuple(int(v) for v in c) for c in G8["cases"]]
NOISE = {c: float(n) for c, n in zip(CASES, G8["noise"])}
OPS = {"bhattacharyya": 0, "hellinger": 1, "mahalanobis_sq": 2, "mahalanobis": 3}
DTYPES = [torch.float64, torch.float32]
EPS = 1e-6


def _key(C, D, K):
    return f"C{C}_D{D}_K{K}"


def _tol(key, op, what, dtype, floor64):
    if dtype == torch.float64:
        return floor64
    return max(1e-5, 5 * rel_err(G8[f"{key}_{op}_{what}_f32"], G8[f"{key}_{op}_{what}_f64"]))


def _grad_floor(op):
    return 1e-6 if op == "hellinger" else 1e-8


def _native_call(mu, cov, kind, weight, want_grad=True, want_dist=True):
    from sqfa_amd import _native
    out = _native.hip_gauss_pairwise_loss(mu, cov, kind, EPS, weight, want_grad=want_grad, want_dist=want_dist)
    torch.cuda.synchronize()
    return out


def _feature_stats(key, dtype):
    return (torch.tensor(G8[f"{key}_fmu"], dtype=dtype, device=DEV), torch.tensor(G8[f"{key}_fcov"], dtype=dtype, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("C,D,K", CASES)
def test_cabi_parity_golden_cases(C, D, K, op, dtype):
    key, kind = _key(C, D, K), OPS[op]
    mu, cov = _feature_stats(key, dtype)
    weight = -1.0 / (C * (C - 1) // 2)
    # the expression written here (on the unrounded float64 inputs) is pinned to what the reference computed
    loss_e, gmu_e, gcov_e, D_e = _full_expression(*_feature_stats(key, torch.float64), kind, weight)
    assert rel_err(D_e.cpu(), G8[f"{key}_{op}_D_f64"]) < 1e-10
    assert rel_err(loss_e.cpu(), G8[f"{key}_{op}_loss_f64"]) < 1e-10
    assert rel_err(gmu_e.cpu(), G8[f"{key}_{op}_gmu_f64"]) < 1e-7
    assert rel_err(gcov_e.cpu(), G8[f"{key}_{op}_gcov_f64"]) < 1e-7
    out = _native_call(mu, cov, kind, weight)
    assert out["nonfinite"].tolist() == [0, 0]
    errs = {"loss": rel_err(out["loss"].cpu(), G8[f"{key}_{op}_loss_f64"]),
            "D": rel_err(out["dist"].cpu(), G8[f"{key}_{op}_D_f64"]),
            "gmu": rel_err(out["gmu"].cpu(), G8[f"{key}_{op}_gmu_f64"]),
            "gcov": rel_err(out["gcov"].cpu(), G8[f"{key}_{op}_gcov_f64"])}
    print(key, op, dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["loss"] <= _tol(key, op, "loss", dtype, 1e-9)
    assert errs["D"] <= _tol(key, op, "D", dtype, 1e-9)
    assert errs["gmu"] <= _tol(key, op, "gmu", dtype, _grad_floor(op))
    assert errs["gcov"] <= _tol(key, op, "gcov", dtype, _grad_floor(op))
    assert torch.equal(out["gcov"], out["gcov"].transpose(1, 2))         # full symmetric matrices
    diag = out["dist"].diagonal()
    assert torch.allclose(diag, torch.full_like(diag, 0.0 if kind in (0, 2) else EPS ** 0.5), rtol=1e-6, atol=0)
    fwd = _native_call(mu, cov, kind, weight, want_grad=False, want_dist=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["gmu"] is None and fwd["dist"] is None


def _large_inputs(dtype):
    g = torch.Generator().manual_seed(11)
    C, K = 1000, 16
    common = torch.randn(K, 4 * K, generator=g, dtype=torch.float64)
    common = common @ common.T / (4 * K)
    A = torch.randn(C, K, 4 * K, generator=g, dtype=torch.float64)
    cov = 0.7 * common + 0.3 * (A @ A.transpose(1, 2) / (4 * K))
    mu = 0.3 * torch.randn(C, K, generator=g, dtype=torch.float64)
    # the float32 run sees float32-rounded inputs; the float64 expression is evaluated on the same rounded values
    return mu.to(dtype).to(DEV), cov.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
def test_cabi_parity_c1000_k16_sampled_rows(op, dtype):
    kind = OPS[op]
    mu, cov = _large_inputs(dtype)
    C = mu.shape[0]
    weight = -1.0 / (C * (C - 1) // 2)
    out = _native_call(mu, cov, kind, weight)
    assert out["nonfinite"].tolist() == [0, 0]
    mu64, cov64 = mu.double(), cov.double()
    # the loss over all pairs, in row chunks (nothing of size (C,C,K,K) at once)
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    with torch.no_grad():
        for r0 in range(0, C, 100):
            Dr = _rows_D(mu64[r0:r0 + 100], cov64[r0:r0 + 100], mu64, cov64, kind)
            mask = torch.arange(C, device=DEV)[None, :] < torch.arange(r0, r0 + 100, device=DEV)[:, None]
            total += (Dr * mask).sum()
    rows = torch.tensor([0, 1, 63, 64, 255, 256, 500, 777, 998, 999], device=DEV)
    mu_r = mu64[rows].clone().requires_grad_(True)
    cov_r = cov64[rows].clone().requires_grad_(True)
    Dr = _rows_D(mu_r, cov_r, mu64, cov64, kind)
    off = torch.ones_like(Dr, dtype=torch.bool)
    off[torch.arange(len(rows)), rows] = False
    # class i sees each of its pairs from its own side: row i of the gradient is d/d(class i) of weight * sum_{j != i} D_ij
    gmu_e, gcov_e = torch.autograd.grad(weight * (Dr * off).sum(), (mu_r, cov_r))
    D_e = Dr.detach().clone()
    D_e[torch.arange(len(rows)), rows] = 0.0 if kind in (0, 2) else EPS ** 0.5
    # float32: the reference was not run at this size; its own float32 deviation on the golden case of the same K and
    # the same family of inputs (C10_D24_K16) is the yardstick, by the same rule as on the golden cases
    k16 = _key(*CASES[3])
    tol_v = max(_tol(k16, op, "loss", dtype, 1e-9), _tol(k16, op, "D", dtype, 1e-9))
    tol_g = max(_tol(k16, op, "gmu", dtype, _grad_floor(op)), _tol(k16, op, "gcov", dtype, _grad_floor(op)))
    errs = {"loss": rel_err(out["loss"].cpu(), (weight * total).cpu()), "D": rel_err(out["dist"][rows].cpu(), D_e.cpu()),
            "gmu": rel_err(out["gmu"][rows].cpu(), gmu_e.cpu()), "gcov": rel_err(out["gcov"][rows].cpu(), gcov_e.cpu())}
    print("C=1000 K=16", op, dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["loss"] <= tol_v and errs["D"] <= tol_v
    assert errs["gmu"] <= tol_g and errs["gcov"] <= tol_g


# ---------------------------------------------------------------------------------------------------------------------
def _model(C, D, K, op, dtype, constraint="sphere"):
    import sqfa_amd
    from sqfa_amd import distances
    key = _key(C, D, K)
    model = sqfa_amd.model.SQFA(n_dim=D, n_filters=K, feature_noise=NOISE[(C, D, K)], distance_fun=getattr(distances, op),
                                constraint=constraint)
    if dtype == torch.float64:
        model = model.double()
    model = model.to(DEV)
    if constraint == "sphere":   # other constraints keep their (seeded) random initial filters
        with torch.no_grad():
            model.parametrizations.filters.original.copy_(torch.tensor(G8[f"{key}_raw"], dtype=dtype))
    stats = {"means": torch.tensor(G8[f"{key}_mu"], dtype=dtype, device=DEV),
             "covariances": torch.tensor(G8[f"{key}_cov"], dtype=dtype, device=DEV)}
    return model, stats


def _closure(model, stats):
    """One closure evaluation as the fitting loop does it: (loss, gradient of the single raw parameter, fused?)."""
    from sqfa_amd import _optim
    prepared = model._prepare_statistics(stats)
    model.zero_grad()
    fused = model._fused_closure_loss(prepared)
    if fused is not None:
        loss, flags = fused
        assert flags.tolist() == [0, 0]
    else:
        Dm = model.get_class_distances(prepared, regularized=True)
        _optim.check_distances_valid(Dm)
        C = Dm.shape[0]
        rows, cols = torch.tril_indices(C, C, offset=-1)
        loss = -Dm[rows.to(DEV), cols.to(DEV)].mean()
    loss.backward()
    (param,) = list(model.parameters())
    return loss.detach(), param.grad.detach().clone(), fused is not None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("C,D,K", CASES)
def test_closure_vs_reference(C, D, K, op, dtype, monkeypatch):
    from sqfa_amd import _native
    key = _key(C, D, K)

    def refuse(*a, **k):
        raise AssertionError("the generic pair-terms node was used by the fused closure")

    monkeypatch.setattr(_native.GaussPairTerms, "apply", refuse)
    model, stats = _model(C, D, K, op, dtype)
    loss, grad, fused = _closure(model, stats)
    assert fused
    e_l, e_g = rel_err(loss.cpu(), G8[f"{key}_{op}_loss_f64"]), rel_err(grad.cpu(), G8[f"{key}_{op}_grad_f64"])
    print(key, op, dtype, f"loss {e_l:.2e} grad {e_g:.2e}")
    assert e_l <= _tol(key, op, "loss", dtype, 1e-9)
    assert e_g <= _tol(key, op, "grad", dtype, _grad_floor(op))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("constraint", ["sphere", "orthogonal"])
@pytest.mark.parametrize("op", list(OPS))
def test_fused_equals_generic_closure(op, constraint, dtype, monkeypatch):
    from sqfa_amd import distances
    for C, D, K in (CASES[1], CASES[3], CASES[4]):
        key = _key(C, D, K)
        res = {}
        for switch in (True, False):
            monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", switch)
            torch.manual_seed(3)
            model, stats = _model(C, D, K, op, dtype, constraint)
            loss, grad, fused = _closure(model, stats)
            assert fused is switch
            res[switch] = (loss.cpu(), grad.cpu())
        e_l, e_g = rel_err(res[True][0], res[False][0]), rel_err(res[True][1], res[False][1])
        print(key, op, constraint, dtype, f"loss {e_l:.2e} grad {e_g:.2e}")
        assert e_l <= _tol(key, op, "loss", dtype, 1e-9)
        assert e_g <= _tol(key, op, "grad", dtype, _grad_floor(op))


@pytest.mark.parametrize("op", ["bhattacharyya", "mahalanobis"])
def test_pairwise_fit_fused_equals_generic(op, monkeypatch):
    """pairwise=True: two filters at a time behind a FixedFilters layer (the chain closure handles any parametrization)."""
    from sqfa_amd import distances
    C, D, K = CASES[2]
    losses = {}
    for switch in (True, False):
        monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", switch)
        model, stats = _model(C, D, K, op, torch.float64)
        loss, _ = model.fit(data_statistics=stats, max_epochs=2, pairwise=True, show_progress=False, return_loss=True)
        losses[switch] = loss.double().numpy()
    assert losses[True].shape == losses[False].shape == (4,)
    assert np.isfinite(losses[True]).all()
    assert rel_err(losses[True], losses[False]) <= 1e-8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
def test_fit_is_graph_captured(op, dtype, monkeypatch):
    from sqfa_amd import _optim
    replays = []
    orig_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays.append(1)
        return orig_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    C, D, K = CASES[3]
    model, stats = _model(C, D, K, op, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")     # the loop warns when a capture fails
        loss, _ = model.fit(data_statistics=stats, max_epochs=_optim.GRAPH_WARMUP_CLOSURES + 5, show_progress=False,
                            return_loss=True)
    assert len(replays) > 0
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("C,D,K", CASES)
def test_fit_trajectory_vs_reference(C, D, K, op, monkeypatch):
    from sqfa_amd import distances
    key = _key(C, D, K)
    ref = G8[f"{key}_{op}_fit_f64"]
    dev = {}
    for switch in (False, True):
        monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", switch)
        model, stats = _model(C, D, K, op, torch.float64)
        loss, _ = model.fit(data_statistics=stats, max_epochs=5, show_progress=False, return_loss=True)
        assert loss.shape == (5,)
        dev[switch] = rel_err(loss.double().numpy(), ref)
    print(f"trajectory {key} {op}: generic {dev[False]:.3e} fused {dev[True]:.3e}")
    assert dev[True] <= max(1e-8, 5 * dev[False])


@pytest.mark.parametrize("op", list(OPS))
def test_indefinite_class_is_reported_not_a_fault(op):
    """A class whose covariance is not positive definite: NaN distances, counted in the flags by the C call and turned into
    the reference's ValueError by fit()."""
    C, D, K = CASES[2]
    key = _key(C, D, K)
    mu, cov = _feature_stats(key, torch.float64)
    cov = cov.clone()
    cov[3] = -4.0 * cov[3]
    out = _native_call(mu, cov, OPS[op], -1.0 / (C * (C - 1) // 2))
    n_nan, n_inf = out["nonfinite"].tolist()
    assert n_nan >= 1 and n_nan + n_inf <= C * (C - 1) // 2
    assert torch.isnan(out["loss"])
    model, stats = _model(C, D, K, op, torch.float64)
    stats["covariances"][3] = -4.0 * stats["covariances"][3]
    with pytest.raises(ValueError, match="Some distances between classes are NaN"):
        model.fit(data_statistics=stats, max_epochs=2, show_progress=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,D,K", [CASES[1], CASES[3], CASES[5]])
def test_bitwise_reproducible(C, D, K, dtype):
    mu, cov = _feature_stats(_key(C, D, K), dtype)
    for kind in range(4):
        a = _native_call(mu, cov, kind, -0.01)
        b = _native_call(mu, cov, kind, -0.01)
        for name in ("loss", "gmu", "gcov", "dist"):
            assert torch.equal(a[name], b[name]), (kind, name)
    mu, cov = _large_inputs(dtype)
    a = _native_call(mu, cov, 1, -1e-6, want_dist=False)
    b = _native_call(mu, cov, 1, -1e-6, want_dist=False)
    for name in ("loss", "gmu", "gcov"):
        assert torch.equal(a[name], b[name]), name


def test_untouched_paths(monkeypatch):
    """sqfa_gauss_pair_terms is bit-identical whatever the switch says; a model with pair_shard set keeps the generic closure."""
    from sqfa_amd import _native, distances
    C, D, K = CASES[3]
    res = {}
    for switch in (True, False):
        monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", switch)
        for dtype in DTYPES:
            mu, cov = _feature_stats(_key(C, D, K), dtype)
            mu.requires_grad_(True)
            cov.requires_grad_(True)
            Q, LD = _native.GaussPairTerms.apply(mu, cov, mu, cov, True)
            gmu, gcov = torch.autograd.grad((Q * Q).sum() + LD.sum(), (mu, cov))
            res[(switch, dtype)] = (Q.detach(), LD.detach(), gmu, gcov)
    for dtype in DTYPES:
        for a, b in zip(res[(True, dtype)], res[(False, dtype)]):
            assert torch.equal(a, b)
    monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", True)
    model, stats = _model(C, D, K, "bhattacharyya", torch.float64)

    class FakeShard:
        shard, world_size = (0, 1), 1

        def reduce(self, *a):
            raise AssertionError("not reached")

    model.pair_shard = FakeShard()
    assert model._fused_closure_loss(model._prepare_statistics(stats)) is None
