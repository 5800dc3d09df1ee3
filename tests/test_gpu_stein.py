"""GPU tests of the fused Stein closure: sqfa_stein_pairwise_loss (per-class Cholesky -> one pass over the ordered class
pairs that factors every pair's mean matrix in registers -> per-class finish), _native.ClassPairLoss (family "stein") and
the closures of SecondMomentsSQFA (logdet.stein, logdet.stein_root), against the float64 generalised-eigenvalue route of
tests/stein_oracle.py and its closed-form gradient.

Bounds, max-abs scaled (stein_oracle.max_rel): float64 1e-11 on loss, distances and gradient; float32 max(1e-5, 5 x the
deviation of the oracle's own float32 evaluation of the three-log-determinant formula, numpy float32, on the same
float32-rounded inputs).  Both numbers are measured, printed and recorded with record_property.

Geometry of the pair pass (stein_kernel.hip): one workgroup per class, 256 / G lane groups of G lanes, one pair per group
and round, one matrix row per lane, MMAX columns in registers:  m <= 4: G 4 | m <= 8: G 8 | m <= 16: G 16 | m <= 24: G 32,
MMAX 24 | m <= 32: G 32 | m <= 48: G 64, MMAX 48 | m <= 64: G 64.  Up to 16 the gradient sums live in registers and the
groups are combined through LDS; above, every group has its own slice of the workspace.  SIZES takes both sides of every
one of these at n = 7 (partly filled rounds everywhere); CLASSES takes n = 2, 3, 33, 65 at m = 3, 16, 17, 33 and the
largest size (64, 32, 16, 8 and 4 groups: rounds partly filled and crossed)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import stein_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
EPS = 1e-6
SIZES = [(7, m) for m in (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 48, 49, 63, 64)]
CLASSES = [(n, m) for m in (3, 16, 17, 33) for n in (2, 3, 33, 65)] + [(2, 64), (65, 64)]
OPS = {"stein": False, "stein_root": True}      # name -> sqrt_mode


def _native_call(S, sqrt_mode, weight, W=None, want_grad=True, want_dist=True):
    from sqfa_amd import _native
    out = _native.hip_stein_pairwise_loss(S, sqrt_mode, EPS, weight, want_grad=want_grad, want_dist=want_dist, pair_weights=W)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _classes(n, m):
    """Float32-rounded inputs of one shape and their divergences by both routes: computed once, shared by every case."""
    S32 = so.make_classes(n, m, seed=1000 * n + m).astype(np.float32)
    S32 = 0.5 * (S32 + S32.transpose(0, 2, 1))
    S64 = S32.astype(np.float64)
    return S32, so.stein_eigenvalues(S64, S64), so.three_logdets(S32, S32, np.float32)


@functools.lru_cache(maxsize=None)
def _reference(n, m, sqrt_mode, weighted):
    """Inputs (float32-rounded), the float64 oracle and the float32 yardstick of one case: computed once, shared by the
    dtypes, left unchanged."""
    S32, div64, div32 = _classes(n, m)
    weight = -1.0 / (n * (n - 1) // 2)
    W32 = None
    if weighted:
        W = so.make_weights(n, seed=n + m)
        W32 = (-W / np.tril(W, -1).sum()).astype(np.float32)          # as the closure passes them: -W / sum W
    up = lambda a: None if a is None else a.astype(np.float64)
    e64 = so.loss_and_gradient(up(S32), sqrt_mode, weight, up(W32), div=div64)
    e32 = so.loss_and_gradient(S32, sqrt_mode, weight, W32, dtype=np.float32, div=div32)
    return S32, W32, weight, e64, e32


def _tolerance(name, dtype, yard, want):
    return 1e-11 if dtype == torch.float64 else max(1e-5, 5 * so.max_rel(yard[name], want[name]))


def _check_native_call(n, m, dtype, sqrt_mode, weighted, record_property):
    S32, W32, weight, e64, e32 = _reference(n, m, sqrt_mode, weighted)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(dtype).to(DEV)
    S, W = dev(S32), dev(W32)
    out = _native_call(S, sqrt_mode, weight, W)
    assert out["nonfinite"].tolist() == [0, 0]
    got = {"loss": out["loss"].item(), "dist": out["dist"].cpu().numpy(), "grad": out["gS"].cpu().numpy()}
    for name in ("loss", "dist", "grad"):
        tol = _tolerance(name, dtype, e32, e64)
        err = so.max_rel(got[name], e64[name])
        yard = so.max_rel(e32[name], e64[name])
        print(f"n={n} m={m} {dtype} sqrt={sqrt_mode} weighted={weighted} {name}: err {err:.2e} float32 oracle {yard:.2e} "
              f"tol {tol:.2e}")
        record_property(f"{name}_err", err)
        record_property(f"{name}_float32_oracle", yard)
        assert err <= tol, (n, m, dtype, sqrt_mode, weighted, name, err, tol)
    assert torch.equal(out["gS"], out["gS"].transpose(1, 2))          # exactly symmetric
    diag = out["dist"].diagonal()
    expect = torch.full((n,), EPS, dtype=dtype, device=DEV).sqrt() if sqrt_mode else torch.zeros(n, dtype=dtype, device=DEV)
    assert torch.allclose(diag, expect, rtol=1e-6, atol=0)
    return out, (S, W, weight)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sqrt_mode", [False, True])
@pytest.mark.parametrize("n,m", SIZES + CLASSES)
def test_native_call_vs_oracle(n, m, sqrt_mode, weighted, dtype, record_property):
    out, (S, W, weight) = _check_native_call(n, m, dtype, sqrt_mode, weighted, record_property)
    # forward only, and without the distance matrix: the same bits
    fwd = _native_call(S, sqrt_mode, weight, W, want_grad=False, want_dist=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["nonfinite"].tolist() == [0, 0]
    assert fwd["gS"] is None and fwd["dist"] is None
    nod = _native_call(S, sqrt_mode, weight, W, want_grad=True, want_dist=False)
    assert torch.equal(nod["gS"], out["gS"]) and nod["dist"] is None and torch.equal(nod["loss"], out["loss"])
    nog = _native_call(S, sqrt_mode, weight, W, want_grad=False, want_dist=True)
    assert torch.equal(nog["dist"], out["dist"]) and nog["gS"] is None


def test_zero_weight_pair_is_evaluated_and_takes_no_part():
    """w_10 = 0: the pair is in dist_out and in the counters, not in the loss or the gradient."""
    n, m = 7, 5
    S32, W32, _, _, _ = _reference(n, m, True, True)
    assert W32[1, 0] == 0 and W32[0, 1] == 0
    S, W = torch.from_numpy(S32).double().to(DEV), torch.from_numpy(W32).double().to(DEV)
    base = _native_call(S, True, 0.0, W)
    moved = S.clone()
    moved[0] *= 1.5                      # changes D_10 (and every D_0j)
    out = _native_call(moved, True, 0.0, W)
    assert out["dist"][1, 0] != base["dist"][1, 0]
    r, c = torch.tril_indices(n, n, offset=-1)
    assert abs((W[r, c] * out["dist"][r, c]).sum().item() - out["loss"].item()) <= 1e-12
    want = so.loss_and_gradient(moved.cpu().numpy(), True, 0.0, W.cpu().numpy())
    assert so.max_rel(out["gS"].cpu().numpy(), want["grad"]) <= 1e-11
    # an indefinite class whose pairs all have weight zero is still counted
    Wz = W.clone()
    Wz[0, :] = 0
    Wz[:, 0] = 0
    bad = S.clone()
    bad[0] = -bad[0]
    out = _native_call(bad, True, 0.0, Wz)
    assert out["nonfinite"].tolist()[0] == n - 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(65, 16), (33, 24), (9, 64)])
def test_bitwise_reproducible(n, m, dtype):
    S32, W32, _, _, _ = _reference(n, m, True, True)
    S, W = torch.from_numpy(S32).to(dtype).to(DEV), torch.from_numpy(W32).to(dtype).to(DEV)
    a = _native_call(S, True, 0.0, W)
    b = _native_call(S, True, 0.0, W)
    assert a["nonfinite"].tolist() == [0, 0]
    for name in ("loss", "gS", "dist"):
        assert torch.equal(a[name], b[name]), name
    assert torch.equal(a["gS"], a["gS"].transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# closures
C, D = 5, 12


def _scatters(seed, dtype=torch.float64):
    return torch.from_numpy(so.make_classes(C, D, seed)).to(dtype).to(DEV)


def _points(N, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(N) % C
    X = torch.randn(N, D, generator=g) * (0.7 + 0.3 * y[:, None]) + 0.5 * torch.randn(C, D, generator=g)[y]
    return X.to(dtype).to(DEV), y.to(DEV)


def _model(op, K, constraint="sphere", seed=3, noise=0.05, n_dim=D):
    import sqfa_amd
    from sqfa_amd import logdet
    torch.manual_seed(seed)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=n_dim, n_filters=K, feature_noise=noise,
                                             distance_fun=getattr(logdet, op), constraint=constraint)
    return model.double().to(DEV)


def _closure(model, stats, W=None):
    """One closure evaluation as the fitting loop does it: (loss, gradient of the single raw parameter, fused?)."""
    from sqfa_amd import _native, _optim
    prepared = model._prepare_statistics(stats)
    n = model._n_classes_total(prepared)
    (param,) = list(model.parameters())
    model._pair_weights = _native.normalized_pair_weights(W, n, param.dtype, param.device)
    try:
        model.zero_grad()
        fused = model._fused_closure_loss(prepared)
        if fused is not None:
            loss, flags = fused
            assert flags.tolist() == [0, 0]
        else:
            Dm = model.get_class_distances(prepared, regularized=True)
            _optim.check_distances_valid(Dm)
            rows, cols = torch.tril_indices(n, n, offset=-1)
            rows, cols = rows.to(DEV), cols.to(DEV)
            loss = -Dm[rows, cols].mean() if W is None else (model._pair_weights[rows, cols] * Dm[rows, cols]).sum()
        loss.backward()
    finally:
        model._pair_weights = None
    return loss.detach().cpu().numpy(), param.grad.detach().cpu().numpy().copy(), fused is not None


def _closure_parity(op, K, monkeypatch, record_property, make_stats, constraint="sphere", W=None):
    from sqfa_amd import logdet
    res = {}
    for switch in (True, False):
        monkeypatch.setattr(logdet, "STEIN_FUSED_CLOSURE", switch)
        model = _model(op, K, constraint)
        assert model._has_fused_closure() is switch
        loss, grad, fused = _closure(model, make_stats(), W)
        assert fused is switch
        res[switch] = (loss, grad)
    for k, name in enumerate(("loss", "grad")):
        err = so.max_rel(res[True][k], res[False][k])
        print(f"{op} K={K} {constraint} {name}: fused against generic {err:.2e}")
        record_property(f"{name}_err", err)
        assert err <= 1e-11, (op, K, constraint, name, err)


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("case", ["dense", "points", "pair_weights", "orthogonal"])
def test_fused_equals_generic_closure(case, op, K, monkeypatch, record_property):
    from sqfa_amd.statistics import ClassPoints
    make = lambda: _scatters(21)
    if case == "points":
        make = lambda: ClassPoints(*_points(60, 23))
    W = torch.from_numpy(so.make_weights(C, seed=9)) if case == "pair_weights" else None
    _closure_parity(op, K, monkeypatch, record_property, make, constraint="orthogonal" if case == "orthogonal" else "sphere", W=W)


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("op", list(OPS))
def test_graph_replay_equals_eager(op, K, monkeypatch):
    """The closure through _optim.GraphRunner: one eager pass, the capture, two replays -- the same bits every time."""
    from sqfa_amd import _optim
    monkeypatch.setattr(_optim, "GRAPH_WARMUP_CLOSURES", 1)
    model = _model(op, K)
    prepared = model._prepare_statistics(_scatters(25))
    (param,) = list(model.parameters())
    box = {}

    def stage():
        param.grad = None
        loss, flags = model._fused_closure_loss(prepared)
        loss.backward()
        box["loss"], box["flags"], box["grad"] = loss.detach(), flags, param.grad

    runner = _optim.GraphRunner([stage], box)
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")     # the runner warns when a capture fails
        for _ in range(3):
            out = runner.run()
            torch.cuda.synchronize()
            seen.append((out["loss"].clone(), out["flags"].clone(), out["grad"].clone(), runner.state))
    assert [s[3] for s in seen] == ["warmup", "on", "on"]
    for loss, flags, grad, _ in seen[1:]:
        assert torch.equal(loss, seen[0][0]) and torch.equal(grad, seen[0][2]) and flags.tolist() == [0, 0]
    assert torch.isfinite(seen[0][0]) and seen[0][2].abs().max() > 0


def _fit(op, K, monkeypatch, fused, graph=True, pairwise=False, epochs=3):
    from sqfa_amd import _optim, logdet
    monkeypatch.setattr(logdet, "STEIN_FUSED_CLOSURE", fused)
    monkeypatch.setattr(_optim, "GRAPH_CLOSURE", graph)
    model = _model(op, K)
    loss, _ = model.fit(data_statistics=_scatters(24), max_epochs=epochs, pairwise=pairwise, show_progress=False,
                        return_loss=True)
    return loss, model.filters.detach().cpu()


@pytest.mark.parametrize("op", list(OPS))
def test_fit_fused_equals_generic(op, monkeypatch):
    loss_f, filters_f = _fit(op, 3, monkeypatch, True)
    loss_g, filters_g = _fit(op, 3, monkeypatch, False)
    assert loss_f.shape == loss_g.shape == (3,) and torch.isfinite(loss_f).all() and loss_f[-1] < loss_f[0]
    print(f"{op}: final loss fused {loss_f[-1].item():.12f} generic {loss_g[-1].item():.12f}")
    assert abs(loss_f[-1].item() - loss_g[-1].item()) <= 1e-6          # the loop's own atol


def test_pairwise_fit_and_graph_fit(monkeypatch):
    """pairwise=True (two filters at a time behind a FixedFilters layer) and a fit long enough to replay its graph."""
    from sqfa_amd import _optim
    loss_f, _ = _fit("stein", 4, monkeypatch, True, pairwise=True, epochs=2)
    loss_g, _ = _fit("stein", 4, monkeypatch, False, pairwise=True, epochs=2)
    assert loss_f.shape == loss_g.shape == (4,) and abs(loss_f[-1].item() - loss_g[-1].item()) <= 1e-6
    replays = []
    orig_replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), orig_replay(self))[1])
    epochs = _optim.GRAPH_WARMUP_CLOSURES + 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss, filters = _fit("stein_root", 3, monkeypatch, True, epochs=epochs)
    assert len(replays) > 0 and torch.isfinite(loss).all() and loss[-1] < loss[0]
    loss_e, filters_e = _fit("stein_root", 3, monkeypatch, True, graph=False, epochs=epochs)
    assert torch.equal(loss, loss_e) and torch.equal(filters, filters_e)


@pytest.mark.parametrize("op", list(OPS))
def test_indefinite_class_is_reported_not_a_fault(op):
    """A class with a negative eigenvalue: NaN divergences, counted in the flags by the C call and turned into the
    ValueError of check_distances_valid by fit()."""
    n, m = 6, 5
    S = torch.from_numpy(so.make_classes(n, m, seed=31))
    lam, Q = torch.linalg.eigh(S[3])
    lam[0] = -0.5
    S[3] = (Q * lam) @ Q.T
    S[3] = 0.5 * (S[3] + S[3].T)
    out = _native_call(S.to(DEV), OPS[op], -1.0 / 15)
    n_nan, n_inf = out["nonfinite"].tolist()
    assert n_nan == n - 1 and n_inf == 0                  # the pairs of class 3, and only those
    assert torch.isnan(out["loss"])
    nan_rows = torch.isnan(out["dist"]).sum(dim=1).cpu()
    assert nan_rows.tolist() == [1, 1, 1, n - 1, 1, 1]
    # in a fit: the indefinite class in the statistics, no noise to repair it
    model = _model(op, m, noise=0.0, n_dim=m)              # square filters: a congruence keeps the inertia
    assert model._has_fused_closure()
    with pytest.raises(ValueError, match="Some distances between classes are NaN"):
        model.fit(data_statistics=S.to(DEV), max_epochs=2, show_progress=False)


def test_more_filters_than_the_limit_take_the_generic_closure(monkeypatch):
    from sqfa_amd import _native
    with pytest.raises(NotImplementedError, match="Stein"):
        _native.hip_stein_pairwise_loss(torch.eye(65, dtype=torch.float64, device=DEV).repeat(2, 1, 1), False, EPS, -1.0)

    def refuse(*a, **k):
        raise AssertionError("the native Stein pass was called beyond its limit")

    monkeypatch.setattr(_native, "_class_pair_call", refuse)
    model = _model("stein", 65, n_dim=66)
    stats = torch.from_numpy(so.make_classes(3, 66, seed=51)).to(DEV)
    assert model._closure_plan() is None and not model._has_fused_closure()
    assert model._closure_plan(model._prepare_statistics(stats)) is None
    loss, _ = model.fit(data_statistics=stats, max_epochs=1, show_progress=False, return_loss=True)
    assert loss.shape == (1,) and torch.isfinite(loss).all()
