"""GPU tests of the fused log-Euclidean closure: sqfa_log_euclidean_pairwise_loss (per-class logarithm -> one pass over the
ordered class pairs -> Daleckii-Krein backward), _native.ClassPairLoss (family "log_euclidean") and SecondMomentsSQFA's closure with
log_euclidean / log_euclidean_sq as distance_fun, against the reference's values (golden G9,
tests/golden/make_golden_log_euclidean_closure.py) and a float64 CPU expression of the definition (eigh -> log -> explicit
differences, `_expression` below).

Tolerances (the rule of tests/test_gpu_other_operators.py): float64 1e-9 (loss, distances) / 1e-8 (gradients); float32
max(1e-5, 5 x the reference's own float32-vs-float64 deviation of that quantity on that case, G9's f32 keys).  Where the
reference was not run (tile and size edges, C=1000) the float32 yardstick is torch's own float32 evaluation of the same
expression on the same inputs, by the same rule.

Tile geometry of the pair pass (log_euclidean_kernel.hip, LogEucCfg): TI classes per workgroup and TJ classes per LDS tile,
  m <= 4: TI 8, TJ 64 | m <= 8: TI 4, TJ 64 | m <= 16: TI 4, TJ 56 (float32) / 24 (float64) | m <= 24: TI 2, TJ 24 / 8 |
  m <= 32: TI 2, TJ 12 / 4 | m <= 64: TI 1 (2 for float64 above 48), TJ 4 (2)
-- EDGE_SHAPES takes a class count one below and one above each of these at m = 4 and m = 16.

5-epoch float64 loss trajectory (test_fit_trajectory_vs_reference): the fused path may deviate from the golden by
5 x the generic path's own deviation, with a floor of 1e-8 relative; both are measured in the test and printed."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G9 = load_golden("g9_log_euclidean_closure.npz")
CASES = [tuple(int(v) for v in c) for c in G9["cases"]]
NOISE = {c: float(n) for c, n in zip(CASES, G9["noise"])}
OPS = {"log_euclidean": True, "log_euclidean_sq": False}   # name -> sqrt_mode
DTYPES = [torch.float64, torch.float32]
EPS = 1e-6


def _key(C, D, K):
    return f"C{C}_D{D}_K{K}"


def _unpack_sym(P):
    """(C, n(n+1)/2) lower triangles in np.tril_indices order -> (C,n,n) symmetric (the golden's storage of symmetric matrices)."""
    n = int(round((np.sqrt(8 * P.shape[-1] + 1) - 1) / 2))
    r, c = np.tril_indices(n)
    M = np.zeros((P.shape[0], n, n), dtype=P.dtype)
    M[:, r, c] = P
    M[:, c, r] = P
    return M


def _tol(key, op, what, dtype, floor64):
    if dtype == torch.float64:
        return floor64
    return max(1e-5, 5 * rel_err(G9[f"{key}_{op}_{what}_f32"], G9[f"{key}_{op}_{what}_f64"]))


def _native_call(S, sqrt_mode, weight, want_grad=True, want_dist=True):
    from sqfa_amd import _native
    out = _native.hip_log_euclidean_pairwise_loss(S, sqrt_mode, EPS, weight, want_grad=want_grad, want_dist=want_dist)
    torch.cuda.synchronize()
    return out


def _feature_scatters(key, dtype):
    return torch.tensor(_unpack_sym(G9[f"{key}_fscatters"]), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# the definition, on the CPU

def _spd_log(S):
    lam, Q = torch.linalg.eigh(S)
    return (Q * torch.log(lam)[..., None, :]) @ Q.transpose(-2, -1)


def _rows_D(L_rows, L_all, sqrt_mode):
    diff = L_rows[:, None] - L_all[None]            # explicit differences, (r,n,m,m)
    d2 = (diff * diff).sum(dim=(-2, -1))
    return torch.sqrt(d2 + EPS) if sqrt_mode else d2


def _expression(S, sqrt_mode, weight, rows=None):
    """S (n,m,m) CPU tensor.  (loss, D (n,n) or None, gS of `rows` (all classes when None)): class i's gradient is
    d/dS_i of weight * sum_{j != i} D_ij, symmetrised; the diagonal of D as the reference gives it."""
    n = S.shape[0]
    with torch.no_grad():
        L_all = _spd_log(S)
        total = torch.zeros((), dtype=S.dtype)
        D_full = torch.empty((n, n), dtype=S.dtype) if rows is None else None
        for r0 in range(0, n, 64):
            Dr = _rows_D(L_all[r0:r0 + 64], L_all, sqrt_mode)
            idx = torch.arange(r0, min(r0 + 64, n))
            total += (Dr * (torch.arange(n)[None, :] < idx[:, None])).sum()
            if D_full is not None:
                D_full[r0:r0 + 64] = Dr
    sel = torch.arange(n) if rows is None else torch.as_tensor(rows)
    S_r = S[sel].clone().requires_grad_(True)
    Dr = _rows_D(_spd_log(S_r), L_all, sqrt_mode)
    off = torch.ones_like(Dr, dtype=torch.bool)
    off[torch.arange(len(sel)), sel] = False
    (gS,) = torch.autograd.grad(weight * (Dr * off).sum(), S_r)
    return weight * total, D_full, 0.5 * (gS + gS.transpose(1, 2))


def _make_spd(n, m, seed):
    """0.7 x a common Wishart + 0.3 x a per-class Wishart of 4 m samples, + 0.01 I (the family of the golden's inputs)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(m, 4 * m, generator=g, dtype=torch.float64)
    A = torch.randn(n, m, 4 * m, generator=g, dtype=torch.float64)
    S = 0.7 * (X @ X.T / (4 * m)) + 0.3 * (A @ A.transpose(1, 2) / (4 * m)) + 0.01 * torch.eye(m, dtype=torch.float64)
    return 0.5 * (S + S.transpose(1, 2))


@functools.lru_cache(maxsize=None)
def _reference(n, m, sqrt_mode, rows=None):
    """Inputs and both evaluations of the expression for one shape: computed once, shared by the dtypes, left unchanged.
    The float32 run of the kernel sees the float32-rounded inputs, and so do both evaluations."""
    S32 = _make_spd(n, m, 1000 * n + m).float()
    weight = -1.0 / (n * (n - 1) // 2)
    e64 = _expression(S32.double(), sqrt_mode, weight, rows)
    e32 = _expression(S32, sqrt_mode, weight, rows)
    return S32, weight, e64, e32


def _check_against_expression(n, m, op, dtype, rows=None):
    sqrt_mode = OPS[op]
    S32, weight, e64, e32 = _reference(n, m, sqrt_mode, rows)
    out = _native_call(S32.to(dtype).to(DEV), sqrt_mode, weight, want_dist=rows is None)
    assert out["nonfinite"].tolist() == [0, 0]
    sel = slice(None) if rows is None else list(rows)
    got = {"loss": out["loss"].cpu(), "gS": out["gS"][sel].cpu()}
    names = ["loss", "gS"]
    if rows is None:
        got["D"] = out["dist"].cpu()
        names.append("D")
    want = dict(zip(("loss", "D", "gS"), e64))
    yard = dict(zip(("loss", "D", "gS"), e32))
    for name in names:
        floor = 1e-8 if name == "gS" else 1e-9
        tol = floor if dtype == torch.float64 else max(1e-5, 5 * rel_err(yard[name], want[name]))
        err = rel_err(got[name], want[name])
        print(f"n={n} m={m} {op} {dtype} {name}: err {err:.2e} tol {tol:.2e}")
        assert err <= tol, (n, m, op, dtype, name, err, tol)
    assert torch.equal(out["gS"], out["gS"].transpose(1, 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("C,D,K", CASES)
def test_cabi_parity_golden_cases(C, D, K, op, dtype):
    key, sqrt_mode = _key(C, D, K), OPS[op]
    S = _feature_scatters(key, dtype)
    weight = -1.0 / (C * (C - 1) // 2)
    out = _native_call(S, sqrt_mode, weight)
    assert out["nonfinite"].tolist() == [0, 0]
    errs = {"loss": rel_err(out["loss"].cpu(), G9[f"{key}_{op}_loss_f64"]),
            "D": rel_err(out["dist"].cpu(), G9[f"{key}_{op}_D_f64"]),
            "gS": rel_err(out["gS"].cpu(), _unpack_sym(G9[f"{key}_{op}_gS_f64"]))}
    print(key, op, dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["loss"] <= _tol(key, op, "loss", dtype, 1e-9)
    assert errs["D"] <= _tol(key, op, "D", dtype, 1e-9)
    assert errs["gS"] <= _tol(key, op, "gS", dtype, 1e-8)
    assert torch.equal(out["gS"], out["gS"].transpose(1, 2))             # full symmetric matrices
    assert torch.equal(out["dist"], out["dist"].t())                     # both triangles, from the same arithmetic
    diag = out["dist"].diagonal()
    assert torch.allclose(diag, torch.full_like(diag, EPS ** 0.5 if sqrt_mode else 0.0), rtol=1e-6, atol=0)
    fwd = _native_call(S, sqrt_mode, weight, want_grad=False, want_dist=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["gS"] is None and fwd["dist"] is None


# (n, m): one pair; every lane geometry and sizes that are no multiple of 4 or of the lane count; class counts one below and
# one above the i-tile (8 at m = 4; 4 at m = 16) and the j-tile (64 at m = 4; 56 for float32 and 24 for float64 at m = 16); more
# than one workgroup with a ragged last tile
EDGE_SHAPES = [(2, 3), (2, 16), (6, 2), (6, 5), (6, 8), (5, 31), (5, 32), (4, 63),
               (7, 4), (9, 4), (63, 4), (65, 4), (3, 16), (5, 16), (23, 16), (25, 16), (55, 16), (57, 16), (257, 4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("n,m", EDGE_SHAPES)
def test_tile_and_size_edges(n, m, op, dtype):
    out = _check_against_expression(n, m, op, dtype)
    assert torch.equal(out["dist"], out["dist"].t())


SAMPLED_ROWS = tuple(sorted({0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 255, 256, 257, 333, 400, 499, 500, 511, 512, 600, 640, 700,
                             767, 768, 777, 800, 850, 895, 896, 900, 950, 990, 991, 992, 995, 996, 997, 998, 999}))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(OPS))
def test_cabi_parity_c1000_m16_sampled_rows(op, dtype):
    assert len(SAMPLED_ROWS) == 40
    _check_against_expression(1000, 16, op, dtype, rows=SAMPLED_ROWS)


# ---------------------------------------------------------------------------------------------------------------------
def _model(C, D, K, op, dtype, constraint="sphere"):
    import sqfa_amd
    from sqfa_amd import distances
    key = _key(C, D, K)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=NOISE[(C, D, K)],
                                             distance_fun=getattr(distances, op), constraint=constraint)
    if dtype == torch.float64:
        model = model.double()
    model = model.to(DEV)
    if constraint == "sphere":   # other constraints keep their (seeded) random initial filters
        with torch.no_grad():
            model.parametrizations.filters.original.copy_(torch.tensor(G9[f"{key}_raw"], dtype=dtype))
    stats = torch.tensor(_unpack_sym(G9[f"{key}_scatters"]), dtype=dtype, device=DEV)
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
        raise AssertionError("the generic log-Euclidean chain was used by the fused closure")

    monkeypatch.setattr(_native.SpdFunction, "apply", refuse)
    monkeypatch.setattr(torch, "cdist", refuse)
    model, stats = _model(C, D, K, op, dtype)
    loss, grad, fused = _closure(model, stats)
    assert fused
    e_l, e_g = rel_err(loss.cpu(), G9[f"{key}_{op}_loss_f64"]), rel_err(grad.cpu(), G9[f"{key}_{op}_grad_f64"])
    print(key, op, dtype, f"loss {e_l:.2e} grad {e_g:.2e}")
    assert e_l <= _tol(key, op, "loss", dtype, 1e-9)
    assert e_g <= _tol(key, op, "grad", dtype, 1e-8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("constraint", ["sphere", "orthogonal"])
@pytest.mark.parametrize("op", list(OPS))
def test_fused_equals_generic_closure(op, constraint, dtype, monkeypatch):
    from sqfa_amd import distances
    for C, D, K in (CASES[1], CASES[3], CASES[4]):
        key = _key(C, D, K)
        res = {}
        for switch in (True, False):
            monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", switch)
            torch.manual_seed(3)
            model, stats = _model(C, D, K, op, dtype, constraint)
            loss, grad, fused = _closure(model, stats)
            assert fused is switch
            res[switch] = (loss.cpu(), grad.cpu())
        e_l, e_g = rel_err(res[True][0], res[False][0]), rel_err(res[True][1], res[False][1])
        print(key, op, constraint, dtype, f"loss {e_l:.2e} grad {e_g:.2e}")
        assert e_l <= _tol(key, op, "loss", dtype, 1e-9)
        assert e_g <= _tol(key, op, "grad", dtype, 1e-8)


@pytest.mark.parametrize("op", list(OPS))
def test_pairwise_fit_fused_equals_generic(op, monkeypatch):
    """pairwise=True: two filters at a time behind a FixedFilters layer (the chain closure handles any parametrization)."""
    from sqfa_amd import distances
    C, D, K = CASES[2]
    losses = {}
    for switch in (True, False):
        monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", switch)
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
    ref = G9[f"{key}_{op}_fit_f64"]
    dev = {}
    for switch in (False, True):
        monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", switch)
        model, stats = _model(C, D, K, op, torch.float64)
        loss, _ = model.fit(data_statistics=stats, max_epochs=5, show_progress=False, return_loss=True)
        assert loss.shape == (5,)
        dev[switch] = rel_err(loss.double().numpy(), ref)
    print(f"trajectory {key} {op}: generic {dev[False]:.3e} fused {dev[True]:.3e}")
    assert dev[True] <= max(1e-8, 5 * dev[False])


@pytest.mark.parametrize("op", list(OPS))
def test_indefinite_class_is_reported_not_a_fault(op):
    """A class whose scatter is not positive definite: NaN distances, counted in the flags by the C call and turned into
    the reference's ValueError by fit()."""
    C, D, K = CASES[2]
    S = _feature_scatters(_key(C, D, K), torch.float64).clone()
    S[3] = -4.0 * S[3]
    out = _native_call(S, OPS[op], -1.0 / (C * (C - 1) // 2))
    n_nan, n_inf = out["nonfinite"].tolist()
    assert n_nan >= 1 and n_nan + n_inf <= C * (C - 1) // 2
    assert torch.isnan(out["loss"])
    model, stats = _model(C, D, K, op, torch.float64)
    stats[3] = -4.0 * stats[3]
    with pytest.raises(ValueError, match="Some distances between classes are NaN"):
        model.fit(data_statistics=stats, max_epochs=2, show_progress=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,D,K", [CASES[1], CASES[3], CASES[5], CASES[6]])
def test_bitwise_reproducible(C, D, K, dtype):
    S = _feature_scatters(_key(C, D, K), dtype)
    for sqrt_mode in (True, False):
        a = _native_call(S, sqrt_mode, -0.01)
        b = _native_call(S, sqrt_mode, -0.01)
        for name in ("loss", "gS", "dist"):
            assert torch.equal(a[name], b[name]), (sqrt_mode, name)
    big = _make_spd(1000, 16, 7).to(dtype).to(DEV)
    a = _native_call(big, True, -1e-6)
    b = _native_call(big, True, -1e-6)
    for name in ("loss", "gS", "dist"):
        assert torch.equal(a[name], b[name]), name


def test_untouched_paths(monkeypatch):
    """distances.log_euclidean(S, S) is bit-identical whatever the switch says; a model with pair_shard set keeps the generic
    closure."""
    from sqfa_amd import distances
    C, D, K = CASES[3]
    res = {}
    for switch in (True, False):
        monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", switch)
        for dtype in DTYPES:
            S = _feature_scatters(_key(C, D, K), dtype).requires_grad_(True)
            Dm = distances.log_euclidean(S, S)
            D2 = distances.log_euclidean_sq(S, S[:4])          # the cross case
            (g,) = torch.autograd.grad(Dm.sum() + D2.sum(), S)
            res[(switch, dtype)] = (Dm.detach(), D2.detach(), g)
    for dtype in DTYPES:
        for a, b in zip(res[(True, dtype)], res[(False, dtype)]):
            assert torch.equal(a, b)
    monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", True)
    model, stats = _model(C, D, K, "log_euclidean", torch.float64)
    assert model._fused_closure_loss(model._prepare_statistics(stats)) is not None

    class FakeShard:
        shard, world_size = (0, 1), 1

        def reduce(self, *a):
            raise AssertionError("not reached")

    model.pair_shard = FakeShard()
    assert model._fused_closure_loss(model._prepare_statistics(stats)) is None
