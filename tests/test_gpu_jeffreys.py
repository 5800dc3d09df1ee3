"""GPU tests of the fused Jeffreys closure: sqfa_jeffreys_pairwise_loss (per-class precisions -> one O(m^2) pass over the
ordered class pairs -> per-class chain rule through the inverse), _native.ClassPairLoss (family "jeffreys") and the closures of SQFA
(jeffreys, jeffreys_root) and SecondMomentsSQFA (jeffreys_spd, jeffreys_spd_root), against the float64 textbook form of
tests/jeffreys_oracle.py and its autograd gradients.

Tolerances (the rule of tests/test_gpu_other_operators.py): float64 1e-9 relative (loss, distances) / 1e-8 (gradients);
float32 max(1e-5, 5 x the deviation of the float32 evaluation of the package's own direct-call torch expression,
divergences._jeffreys_matrix, from the float64 value on that case).  Both numbers are measured in the test and printed.
The float32 runs see the float32-rounded inputs, and so do both evaluations.

Geometry of the pair pass (jeffreys_kernel.hip, JeffCfg): G lanes per class group, TI classes per workgroup, TJ classes per
LDS tile;  m <= 4: G 4, TI 8, TJ 64 | m <= 8: G 8 | m <= 16: G 16 | m <= 24 and m <= 32: G 32 | m <= 48 and m <= 64: G 64
(float64 above 32: unstaged).  SIZE_EDGES takes both sides of every one of these; CLASS_EDGES at m = 4 one pair, one past a
pair, one past TI (9), one past TJ (65) and more than two tiles (130)."""
import functools
import warnings

import pytest
import torch

import jeffreys_oracle as jo
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
EPS = 1e-6
SIZE_EDGES = [(2, 1), (3, 2), (7, 3), (5, 5), (9, 8), (6, 16), (6, 17), (5, 32), (4, 33), (3, 64)]
CLASS_EDGES = [(2, 4), (3, 4), (9, 4), (65, 4), (130, 4)]
GAUSSIAN_OPS = {"jeffreys": False, "jeffreys_root": True}      # name -> sqrt_mode
SPD_OPS = {"jeffreys_spd": False, "jeffreys_spd_root": True}


def _native_call(mu, cov, sqrt_mode, weight, W=None, want_grad=True, want_dist=True):
    from sqfa_amd import _native
    out = _native.hip_jeffreys_pairwise_loss(mu, cov, sqrt_mode, EPS, weight, want_grad=want_grad, want_dist=want_dist,
                                             pair_weights=W)
    torch.cuda.synchronize()
    return out


def _module_expression(muA, covA, muB, covB):
    from sqfa_amd import divergences
    return divergences._jeffreys_matrix(muA, covA, muB, covB)


@functools.lru_cache(maxsize=None)
def _reference(n, m, means, sqrt_mode, weighted):
    """Inputs, the float64 oracle (textbook form) and the float32 yardstick (the module's expression in float32) of one
    case: computed once, shared by the dtypes, left unchanged."""
    mu32, cov32 = jo.make_classes(n, m, seed=1000 * n + m, dtype=torch.float32)
    mu32 = mu32 if means else None
    W32 = jo.make_weights(n, seed=n + m, dtype=torch.float32) if weighted else None
    if W32 is not None:
        W32 = -W32 / torch.tril(W32.double(), -1).sum().float()       # as the closure passes them: -W / sum W
    weight = -1.0 / (n * (n - 1) // 2)
    up = lambda t: None if t is None else t.double()
    e64 = jo.loss_and_gradients(up(mu32), cov32.double(), sqrt_mode, weight, up(W32))
    e32 = jo.loss_and_gradients(mu32, cov32, sqrt_mode, weight, W32, fn=_module_expression)
    return mu32, cov32, W32, weight, e64, e32


def _tolerance(name, dtype, yard, want):
    floor = 1e-8 if name in ("gmu", "gcov") else 1e-9
    return floor if dtype == torch.float64 else max(1e-5, 5 * rel_err(yard[name], want[name]))


def _check_native_call(n, m, dtype, means, sqrt_mode, weighted):
    mu32, cov32, W32, weight, e64, e32 = _reference(n, m, means, sqrt_mode, weighted)
    dev = lambda t: None if t is None else t.to(dtype).to(DEV)
    out = _native_call(dev(mu32), dev(cov32), sqrt_mode, weight, dev(W32))
    assert out["nonfinite"].tolist() == [0, 0]
    names = ["loss", "dist", "gcov"] + (["gmu"] if means else [])
    for name in names:
        tol = _tolerance(name, dtype, e32, e64)
        err = rel_err(out[name].cpu(), e64[name])
        yard = rel_err(e32[name], e64[name])
        print(f"n={n} m={m} {dtype} means={means} sqrt={sqrt_mode} weighted={weighted} {name}: err {err:.2e} "
              f"float32 expression {yard:.2e} tol {tol:.2e}")
        assert err <= tol, (n, m, dtype, means, sqrt_mode, weighted, name, err, tol)
    if not means:
        assert out["gmu"] is None
    assert torch.equal(out["gcov"], out["gcov"].transpose(1, 2))          # exactly symmetric
    diag = out["dist"].diagonal()
    expect = torch.full((n,), EPS, dtype=dtype, device=DEV).sqrt() if sqrt_mode else torch.zeros(n, dtype=dtype, device=DEV)
    assert torch.allclose(diag, expect, rtol=1e-6, atol=0)
    return out, (dev(mu32), dev(cov32), dev(W32), weight)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sqrt_mode", [False, True])
@pytest.mark.parametrize("means", [True, False])
@pytest.mark.parametrize("n,m", SIZE_EDGES + CLASS_EDGES)
def test_native_call_vs_oracle(n, m, means, sqrt_mode, weighted, dtype):
    out, (mu, cov, W, weight) = _check_native_call(n, m, dtype, means, sqrt_mode, weighted)
    # forward only, and without the distance matrix: the same loss bits
    fwd = _native_call(mu, cov, sqrt_mode, weight, W, want_grad=False, want_dist=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["nonfinite"].tolist() == [0, 0]
    assert fwd["gmu"] is None and fwd["gcov"] is None and fwd["dist"] is None
    nod = _native_call(mu, cov, sqrt_mode, weight, W, want_grad=True, want_dist=False)
    assert torch.equal(nod["gcov"], out["gcov"]) and nod["dist"] is None
    if means:
        assert torch.equal(nod["gmu"], out["gmu"])


@pytest.mark.parametrize("sqrt_mode", [False, True])
def test_close_classes_float32(sqrt_mode):
    """Classes 1e-3 apart: the explicit differences keep the digits the textbook traces cancel."""
    n, m = 4, 8
    mu0, cov0 = jo.make_classes(1, m, seed=77)
    g = torch.Generator().manual_seed(78)
    E = torch.randn(n, m, m, generator=g, dtype=torch.float64)
    E = 0.5 * (E + E.transpose(1, 2))
    dm = torch.randn(n, m, generator=g, dtype=torch.float64)
    E[0], dm[0] = 0.0, 0.0                                  # class 0 is the unperturbed one
    cov, mu = cov0 + 1e-3 * E, mu0 + 1e-3 * dm
    mu32, cov32 = mu.float(), cov.float()
    weight = -1.0 / 6
    e64 = jo.loss_and_gradients(mu32.double(), cov32.double(), sqrt_mode, weight)
    e32 = jo.loss_and_gradients(mu32, cov32, sqrt_mode, weight, fn=_module_expression)
    t32 = jo.loss_and_gradients(mu32, cov32, sqrt_mode, weight)                # the textbook form in float32
    out = _native_call(mu32.to(DEV), cov32.to(DEV), sqrt_mode, weight)
    assert out["nonfinite"].tolist() == [0, 0]
    for name in ("loss", "dist", "gmu", "gcov"):
        tol = _tolerance(name, torch.float32, e32, e64)
        err = rel_err(out[name].cpu(), e64[name])
        print(f"close classes sqrt={sqrt_mode} {name}: fused {err:.2e}  float32 expression {rel_err(e32[name], e64[name]):.2e}  "
              f"float32 textbook form {rel_err(t32[name], e64[name]):.2e}  tol {tol:.2e}")
        assert err <= tol, (name, err, tol)


# ---------------------------------------------------------------------------------------------------------------------
# closures
def _statistics(C, D, seed, dtype):
    mu, cov = jo.make_classes(C, D, seed=seed, dtype=torch.float32)
    return {"means": mu.to(dtype).to(DEV), "covariances": cov.to(dtype).to(DEV)}


def _points(C, D, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(N) % C
    X = torch.randn(N, D, generator=g) + 0.5 * torch.randn(C, D, generator=g)[y]
    return X.to(dtype).to(DEV), y.to(DEV)


def _model(op, D, K, dtype, constraint, seed=3, noise=0.05):
    import sqfa_amd
    from sqfa_amd import divergences
    cls = sqfa_amd.model.SQFA if op in GAUSSIAN_OPS else sqfa_amd.model.SecondMomentsSQFA
    torch.manual_seed(seed)
    model = cls(n_dim=D, n_filters=K, feature_noise=noise, distance_fun=getattr(divergences, op), constraint=constraint)
    if dtype == torch.float64:
        model = model.double()
    return model.to(DEV)


def _closure(model, stats, W=None):
    """One closure evaluation as the fitting loop does it: (loss, gradient of the single raw parameter, fused?)."""
    from sqfa_amd import _native, _optim
    prepared = model._prepare_statistics(stats)
    C = model._n_classes_total(prepared)
    (param,) = list(model.parameters())
    model._pair_weights = _native.normalized_pair_weights(W, C, param.dtype, param.device)
    try:
        model.zero_grad()
        fused = model._fused_closure_loss(prepared)
        if fused is not None:
            loss, flags = fused
            assert flags.tolist() == [0, 0]
        else:
            Dm = model.get_class_distances(prepared, regularized=True)
            _optim.check_distances_valid(Dm)
            rows, cols = torch.tril_indices(C, C, offset=-1)
            rows, cols = rows.to(DEV), cols.to(DEV)
            loss = -Dm[rows, cols].mean() if W is None else (model._pair_weights[rows, cols] * Dm[rows, cols]).sum()
        loss.backward()
    finally:
        model._pair_weights = None
    return loss.detach().cpu(), param.grad.detach().cpu().clone(), fused is not None


def _closure_parity(op, constraint, dtype, monkeypatch, make_stats, D, K, W=None):
    """fused (dtype) against the generic closure: in float64 directly; in float32 both against the float64 generic closure,
    the fused one within 5 x the float32 generic closure's own deviation (floor 1e-5)."""
    from sqfa_amd import divergences
    res = {}
    for switch, dt in ((True, dtype), (False, dtype), (False, torch.float64)):
        monkeypatch.setattr(divergences, "JEFFREYS_FUSED_CLOSURE", switch)
        model = _model(op, D, K, dt, constraint)
        loss, grad, fused = _closure(model, make_stats(op, dt), W)
        assert fused is switch
        res[(switch, dt)] = (loss, grad)
    want, yard, got = res[(False, torch.float64)], res[(False, dtype)], res[(True, dtype)]
    for k, name in enumerate(("loss", "grad")):
        floor = 1e-9 if name == "loss" else 1e-8
        tol = floor if dtype == torch.float64 else max(1e-5, 5 * rel_err(yard[k], want[k]))
        err = rel_err(got[k], want[k])
        print(f"{op} {constraint} {dtype} D={D} K={K} {name}: fused {err:.2e} generic {rel_err(yard[k], want[k]):.2e} tol {tol:.2e}")
        assert err <= tol, (op, constraint, dtype, name, err, tol)


def _dense(C, D, seed):
    def make(op, dt):
        stats = _statistics(C, D, seed, dt)
        return stats if op in GAUSSIAN_OPS else stats["covariances"]
    return make


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("constraint", ["sphere", "none", "orthogonal"])
@pytest.mark.parametrize("C,D,K", [(6, 12, 3), (5, 20, 17)])
@pytest.mark.parametrize("op", list(GAUSSIAN_OPS) + list(SPD_OPS))
def test_fused_equals_generic_closure(op, C, D, K, constraint, dtype, monkeypatch):
    _closure_parity(op, constraint, dtype, monkeypatch, _dense(C, D, 21), D, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(GAUSSIAN_OPS) + list(SPD_OPS))
def test_fused_equals_generic_closure_with_pair_weights(op, dtype, monkeypatch):
    W = jo.make_weights(6, seed=9)
    _closure_parity(op, "sphere", dtype, monkeypatch, _dense(6, 12, 22), 12, 3, W=W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(GAUSSIAN_OPS) + list(SPD_OPS))
def test_fused_equals_generic_closure_points_mode(op, dtype, monkeypatch):
    from sqfa_amd.statistics import ClassPoints

    def make(op_, dt):
        X, y = _points(6, 12, 60, 23, dt)
        return ClassPoints(X, y)

    _closure_parity(op, "sphere", dtype, monkeypatch, make, 12, 3)


def _fit(op, K, monkeypatch, fused, graph=True, pairwise=False, epochs=5):
    from sqfa_amd import _optim, divergences
    monkeypatch.setattr(divergences, "JEFFREYS_FUSED_CLOSURE", fused)
    monkeypatch.setattr(_optim, "GRAPH_CLOSURE", graph)
    model = _model(op, 12, K, torch.float64, "sphere")
    stats = _dense(6, 12, 24)(op, torch.float64)
    loss, _ = model.fit(data_statistics=stats, max_epochs=epochs, pairwise=pairwise, show_progress=False, return_loss=True)
    return loss, model.filters.detach().cpu()


@pytest.mark.parametrize("op", list(GAUSSIAN_OPS) + list(SPD_OPS))
def test_fit_fused_equals_generic(op, monkeypatch):
    loss_f, filters_f = _fit(op, 3, monkeypatch, True)
    loss_g, filters_g = _fit(op, 3, monkeypatch, False)
    assert loss_f.shape == loss_g.shape == (5,) and torch.isfinite(loss_f).all()
    print(f"{op}: filters {rel_err(filters_f, filters_g):.2e} loss {rel_err(loss_f, loss_g):.2e}")
    assert rel_err(filters_f, filters_g) <= 1e-8
    assert rel_err(loss_f, loss_g) <= 1e-8


def test_pairwise_fit_fused_equals_generic(monkeypatch):
    """pairwise=True: two filters at a time behind a FixedFilters layer (K = 4: the stages need an even count)."""
    loss_f, filters_f = _fit("jeffreys", 4, monkeypatch, True, pairwise=True, epochs=3)
    loss_g, filters_g = _fit("jeffreys", 4, monkeypatch, False, pairwise=True, epochs=3)
    assert loss_f.shape == loss_g.shape == (6,) and torch.isfinite(loss_f).all()
    assert rel_err(filters_f, filters_g) <= 1e-8


@pytest.mark.parametrize("op", ["jeffreys_root", "jeffreys_spd"])
def test_fit_is_graph_captured_and_replay_equals_eager(op, monkeypatch):
    from sqfa_amd import _optim
    replays = []
    orig_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays.append(1)
        return orig_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    epochs = _optim.GRAPH_WARMUP_CLOSURES + 5
    with warnings.catch_warnings():
        warnings.simplefilter("error")     # the loop warns when a capture fails
        loss, filters = _fit(op, 3, monkeypatch, True, epochs=epochs)
    assert len(replays) > 0
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]
    n_replays = len(replays)
    loss_e, filters_e = _fit(op, 3, monkeypatch, True, graph=False, epochs=epochs)
    assert len(replays) == n_replays                                       # the eager fit replayed nothing
    assert torch.equal(loss, loss_e) and torch.equal(filters, filters_e)


@pytest.mark.parametrize("op", ["jeffreys", "jeffreys_spd_root"])
def test_indefinite_class_is_reported_not_a_fault(op):
    """A class with a negative eigenvalue: NaN divergences, counted in the flags by the C call and turned into the
    ValueError of check_distances_valid by fit()."""
    n, m = 6, 5
    mu, cov = jo.make_classes(n, m, seed=31)
    lam, Q = torch.linalg.eigh(cov[3])
    lam[0] = -0.5
    cov[3] = (Q * lam) @ Q.T
    cov[3] = 0.5 * (cov[3] + cov[3].T)
    means = op in GAUSSIAN_OPS
    sqrt_mode = {**GAUSSIAN_OPS, **SPD_OPS}[op]
    out = _native_call(mu.to(DEV) if means else None, cov.to(DEV), sqrt_mode, -1.0 / 15)
    n_nan, n_inf = out["nonfinite"].tolist()
    assert n_nan >= 1 and n_nan + n_inf <= 15
    assert torch.isnan(out["loss"])
    # in a fit: the indefinite class in the statistics, no noise to repair it
    model = _model(op, m, m, torch.float64, "sphere", noise=0.0)       # square filters: a congruence keeps the inertia
    stats = {"means": mu.to(DEV), "covariances": cov.to(DEV)}
    with pytest.raises(ValueError, match="Some distances between classes are NaN"):
        model.fit(data_statistics=stats if means else stats["covariances"], max_epochs=2, show_progress=False)


def test_bitwise_reproducible():
    n, m = 130, 16
    mu, cov = jo.make_classes(n, m, seed=41, dtype=torch.float32)
    W = jo.make_weights(n, seed=42, dtype=torch.float32)
    W = -W / torch.tril(W, -1).sum()
    mu, cov, W = mu.to(DEV), cov.to(DEV), W.to(DEV)
    a = _native_call(mu, cov, True, 0.0, W)
    b = _native_call(mu, cov, True, 0.0, W)
    assert a["nonfinite"].tolist() == [0, 0]
    for name in ("loss", "gmu", "gcov", "dist"):
        assert torch.equal(a[name], b[name]), name


def test_more_filters_than_the_limit_take_the_generic_closure(monkeypatch):
    from sqfa_amd import _native
    C, D, K = 4, 66, 65

    def refuse(*a, **k):
        raise AssertionError("the native Jeffreys pass was called beyond its limit")

    monkeypatch.setattr(_native, "hip_jeffreys_pairwise_loss", refuse)
    model = _model("jeffreys", D, K, torch.float64, "sphere")
    stats = _statistics(C, D, 51, torch.float64)
    assert model._closure_plan() is None and not model._has_fused_closure()
    assert model._closure_plan(model._prepare_statistics(stats)) is None
    loss, _ = model.fit(data_statistics=stats, max_epochs=1, show_progress=False, return_loss=True)
    assert loss.shape == (1,) and torch.isfinite(loss).all()


def test_untouched_paths(monkeypatch):
    """The closures of the other operators never reach the Jeffreys pass."""
    import sqfa_amd
    from sqfa_amd import _native, distances

    def refuse(*a, **k):
        raise AssertionError("the native Jeffreys pass was called by another operator's closure")

    monkeypatch.setattr(_native, "hip_jeffreys_pairwise_loss", refuse)
    stats = _statistics(6, 12, 61, torch.float64)
    for cls, fn, data in ((sqfa_amd.model.SQFA, distances.bhattacharyya, stats),
                          (sqfa_amd.model.SecondMomentsSQFA, distances.log_euclidean, stats["covariances"])):
        torch.manual_seed(5)
        model = cls(n_dim=12, n_filters=3, feature_noise=0.05, distance_fun=fn).double().to(DEV)
        fused = model._fused_closure_loss(model._prepare_statistics(data))
        assert fused is not None and fused[1].tolist() == [0, 0]
        fused[0].backward()
        (param,) = list(model.parameters())
        assert torch.isfinite(fused[0]) and torch.isfinite(param.grad).all()
