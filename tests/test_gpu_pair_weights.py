"""GPU tests of the per-pair class weights: sqfa_gauss_pairwise_loss_weighted and sqfa_log_euclidean_pairwise_loss_weighted
(loss = sum_{i>j} w_ij D_ij with its gradient, w = -W / sum_{i>j} W), the weighted closures of both models and the weighted
sharded evaluation.

Tolerances (the rule of tests/test_gpu_gauss_kernel_rows.py, no new constant): float64 kernel against the float64
expression 1e-9 (values) / 1e-8 (gradients; Hellinger gradients 1e-6).  float32: max(1e-5, 5 x dev), dev = rel_err(the
same expression evaluated in float32 torch, in float64) on the same float32-rounded inputs and weights, measured here per
quantity and printed -- never anything a kernel returned.  The single-pair indexing checks compare one product with one
distance: 1e-6 relative in float32, 1e-12 in float64 (the loss is a double-precision sum of one non-zero term).

Weights: pair_weight_cases.make_weights (seeded; symmetric, uniform in [0.25, 1.75], about 20 % exact zeros, no class with
all-zero pairs -- asserted there).  Every reference is computed once per case on the CPU and shared."""
import ctypes
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gauss_oracle
from conftest import ROOT, load_golden, rel_err
from pair_weight_cases import check_weights, make_weights, normalized, single_pair, weighted_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
DTYPES = [torch.float64, torch.float32]
KINDS = {0: "bhattacharyya", 1: "hellinger", 2: "mahalanobis_sq", 3: "mahalanobis"}
LE_OPS = {"log_euclidean": True, "log_euclidean_sq": False}   # name -> sqrt_mode


def _tol(dtype, dev, gradient, hellinger=False):
    if dtype == torch.float64:
        return (1e-6 if hellinger else 1e-8) if gradient else 1e-9
    return max(1e-5, 5 * dev)


def _uniform(C):
    return -1.0 / (C * (C - 1) // 2)


@functools.lru_cache(maxsize=None)
def _weights(C, dtype):
    """The case's weights, normalised and rounded to `dtype` (what the kernel and both evaluations of the expression see)."""
    W = make_weights(C, 77 * C + 5)
    check_weights(W)
    return normalized(W).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. Gaussian fused entry, weighted


@functools.lru_cache(maxsize=None)
def _gauss_stats(C, K, dtype):
    mu, cov = gauss_oracle.inputs(C, K, 1000 * C + K)
    return mu.to(dtype), cov.to(dtype)


def _gauss_expression(mu, cov, Wn, kind, dtype):
    mu = mu.detach().to(dtype).requires_grad_(True)
    cov = cov.detach().to(dtype).requires_grad_(True)
    D = gauss_oracle._rows_D(mu, cov, mu, cov, kind)
    loss = torch.tril(Wn.to(dtype) * D, -1).sum()
    gmu, gcov = torch.autograd.grad(loss, (mu, cov))
    return loss.detach(), gmu, gcov, D.detach()


@functools.lru_cache(maxsize=None)
def _gauss_reference(C, K, kind, dtype):
    mu, cov = _gauss_stats(C, K, dtype)
    Wn = _weights(C, dtype)
    ref = _gauss_expression(mu, cov, Wn, kind, torch.float64)
    dev = None
    if dtype == torch.float32:
        dev = tuple(rel_err(lo, hi) for lo, hi in zip(_gauss_expression(mu, cov, Wn, kind, torch.float32)[:3], ref[:3]))
    return ref, dev


def _gauss_call(mu, cov, kind, weight, Wn=None, want_grad=True, want_dist=False):
    from sqfa_amd import _native
    out = _native.hip_gauss_pairwise_loss(mu, cov, kind, EPS, weight, want_grad=want_grad, want_dist=want_dist, pair_weights=Wn)
    torch.cuda.synchronize()
    return out


def _check_gauss(C, K, kind, dtype, label):
    (loss_e, gmu_e, gcov_e, D_e), dev = _gauss_reference(C, K, kind, dtype)
    if kind == 1:   # a condition on the inputs: a saturated Hellinger distance has no gradient left to check
        assert D_e[~torch.eye(C, dtype=torch.bool)].max().item() < 0.99
    mu, cov = (t.to(DEV) for t in _gauss_stats(C, K, dtype))
    Wn = _weights(C, dtype).to(DEV)
    out = _gauss_call(mu, cov, kind, 0.0, Wn)
    assert out["nonfinite"].tolist() == [0, 0]
    assert out["gmu"].shape == (C, K) and out["gcov"].shape == (C, K, K)
    errs = (rel_err(out["loss"].cpu(), loss_e), rel_err(out["gmu"].cpu(), gmu_e), rel_err(out["gcov"].cpu(), gcov_e))
    print(f"weighted gauss {label} C={C} K={K} {KINDS[kind]} {str(dtype)[6:]} loss {errs[0]:.2e} gmu {errs[1]:.2e} gcov {errs[2]:.2e}",
          "dev", [f"{v:.2e}" for v in dev] if dev else None)
    d = dev if dev is not None else (None, None, None)
    assert errs[0] <= _tol(dtype, d[0], False)
    assert errs[1] <= _tol(dtype, d[1], True, kind == 1)
    assert errs[2] <= _tol(dtype, d[2], True, kind == 1)
    assert torch.equal(out["gcov"], out["gcov"].transpose(1, 2))         # full symmetric matrices, bitwise
    fwd = _gauss_call(mu, cov, kind, 0.0, Wn, want_grad=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["gmu"] is None and fwd["gcov"] is None
    assert fwd["nonfinite"].tolist() == [0, 0]
    again = _gauss_call(mu, cov, kind, 0.0, Wn)
    for name in ("loss", "gmu", "gcov"):
        assert torch.equal(again[name], out[name]), name
    return out


GAUSS_ROWS = [(9, K) for K in (7, 8, 12, 15, 16)] + [(7, K) for K in (18, 32, 40, 64)]
# wave and round boundaries (j beyond the first round of 256 indexes the weight row), many passes per LDS group, and the
# host-padded K (n * n >= 20000: K = 5 is padded to 8 by the host, the weights stay (n, n))
GAUSS_COUNTS = [(2, 8), (65, 8), (257, 8), (257, 17), (142, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("C,K", GAUSS_ROWS)
def test_gauss_weighted_rows(C, K, kind, dtype):
    _check_gauss(C, K, kind, dtype, "rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("n,K", GAUSS_COUNTS)
def test_gauss_weighted_class_counts(n, K, kind, dtype, monkeypatch):
    from sqfa_amd import _native
    padded_to = []
    pad = _native._pad_gauss

    def spy(mu, cov, M):
        padded_to.append(M)
        return pad(mu, cov, M)

    monkeypatch.setattr(_native, "_pad_gauss", spy)
    _check_gauss(n, K, kind, dtype, "counts")
    assert set(padded_to) == ({8} if (n, K) == (142, 5) else set())


# ---------------------------------------------------------------------------------------------------------------------
# 2. log-Euclidean fused entry, weighted


def _make_spd(n, m, seed):
    """0.7 x a common Wishart + 0.3 x a per-class Wishart of 4 m samples, + 0.01 I (the family of golden G9's inputs)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(m, 4 * m, generator=g, dtype=torch.float64)
    A = torch.randn(n, m, 4 * m, generator=g, dtype=torch.float64)
    S = 0.7 * (X @ X.T / (4 * m)) + 0.3 * (A @ A.transpose(1, 2) / (4 * m)) + 0.01 * torch.eye(m, dtype=torch.float64)
    return 0.5 * (S + S.transpose(1, 2))


def _le_expression(S, Wn, sqrt_mode, dtype):
    """sum_{i>j} Wn_ij D_ij with L = log S through eigh and explicit differences; gradient symmetrised."""
    S = S.detach().to(dtype).requires_grad_(True)
    lam, Q = torch.linalg.eigh(S)
    L = (Q * torch.log(lam)[..., None, :]) @ Q.transpose(-2, -1)
    diff = L[:, None] - L[None]
    d2 = (diff * diff).sum(dim=(-2, -1))
    D = torch.sqrt(d2 + EPS) if sqrt_mode else d2
    loss = torch.tril(Wn.to(dtype) * D, -1).sum()
    (gS,) = torch.autograd.grad(loss, S)
    return loss.detach(), 0.5 * (gS + gS.transpose(1, 2)), D.detach()


@functools.lru_cache(maxsize=None)
def _le_reference(n, m, sqrt_mode):
    """float32-rounded inputs and weights (both dtypes of the kernel see them), the expression in float64 and in float32."""
    S32 = _make_spd(n, m, 1000 * n + m).float()
    Wn32 = _weights(n, torch.float32)
    e64 = _le_expression(S32, Wn32, sqrt_mode, torch.float64)
    e32 = _le_expression(S32, Wn32, sqrt_mode, torch.float32)
    return S32, Wn32, e64, e32


def _le_call(S, sqrt_mode, weight, Wn=None, want_grad=True, want_dist=False):
    from sqfa_amd import _native
    out = _native.hip_log_euclidean_pairwise_loss(S, sqrt_mode, EPS, weight, want_grad=want_grad, want_dist=want_dist,
                                                  pair_weights=Wn)
    torch.cuda.synchronize()
    return out


# one shape per dispatch row, then class counts straddling the tile widths (TI 8, TJ 64 at m = 4; TI 4, TJ 56 / 24 at m = 16)
LE_SHAPES = [(6, 3), (6, 5), (5, 16), (5, 24), (5, 32), (4, 40), (4, 63),
             (7, 4), (9, 4), (63, 4), (65, 4), (23, 16), (25, 16), (257, 4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(LE_OPS))
@pytest.mark.parametrize("n,m", LE_SHAPES)
def test_log_euclidean_weighted(n, m, op, dtype):
    sqrt_mode = LE_OPS[op]
    S32, Wn32, e64, e32 = _le_reference(n, m, sqrt_mode)
    S, Wn = S32.to(dtype).to(DEV), Wn32.to(dtype).to(DEV)
    out = _le_call(S, sqrt_mode, 0.0, Wn)
    assert out["nonfinite"].tolist() == [0, 0]
    for idx, (name, got) in enumerate((("loss", out["loss"]), ("gS", out["gS"]))):
        dev = rel_err(e32[idx], e64[idx])
        tol = _tol(dtype, dev, name == "gS")
        err = rel_err(got.cpu(), e64[idx])
        print(f"weighted log-euclidean n={n} m={m} {op} {str(dtype)[6:]} {name}: err {err:.2e} dev {dev:.2e} tol {tol:.2e}")
        assert err <= tol, (name, err, tol)
    assert torch.equal(out["gS"], out["gS"].transpose(1, 2))
    fwd = _le_call(S, sqrt_mode, 0.0, Wn, want_grad=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["gS"] is None
    again = _le_call(S, sqrt_mode, 0.0, Wn)
    assert torch.equal(again["loss"], out["loss"]) and torch.equal(again["gS"], out["gS"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. indexing: one pair (a, b) with weight 1, every other pair 0


def _one_pair_tol(dtype):
    return 1e-6 if dtype == torch.float32 else 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("C,K,a,b", [(9, 8, 5, 2), (9, 8, 8, 0), (65, 4, 64, 1), (65, 4, 40, 39), (65, 4, 63, 0)])
def test_gauss_single_pair(C, K, a, b, kind, dtype):
    mu, cov = (t.to(DEV) for t in _gauss_stats(C, K, dtype))
    Wn = normalized(single_pair(C, a, b)).to(dtype).to(DEV)
    plain = _gauss_call(mu, cov, kind, _uniform(C), want_dist=True)
    out = _gauss_call(mu, cov, kind, 0.0, Wn)
    D_ab = plain["dist"][a, b].item()
    assert abs(out["loss"].item() + D_ab) <= _one_pair_tol(dtype) * abs(D_ab)
    assert out["nonfinite"].tolist() == [0, 0]
    others = [c for c in range(C) if c not in (a, b)]
    assert bool((out["gmu"][others] == 0).all()) and bool((out["gcov"][others] == 0).all())
    assert bool((out["gmu"][[a, b]] != 0).any(dim=1).all()) and bool((out["gcov"][[a, b]] != 0).flatten(1).any(dim=1).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(LE_OPS))
@pytest.mark.parametrize("n,m,a,b", [(9, 8, 5, 2), (9, 8, 8, 0), (65, 4, 64, 1), (65, 4, 40, 39), (65, 4, 63, 0)])
def test_log_euclidean_single_pair(n, m, a, b, op, dtype):
    sqrt_mode = LE_OPS[op]
    S = _make_spd(n, m, 1000 * n + m).to(dtype).to(DEV)
    Wn = normalized(single_pair(n, a, b)).to(dtype).to(DEV)
    plain = _le_call(S, sqrt_mode, _uniform(n), want_dist=True)
    out = _le_call(S, sqrt_mode, 0.0, Wn)
    D_ab = plain["dist"][a, b].item()
    assert abs(out["loss"].item() + D_ab) <= _one_pair_tol(dtype) * abs(D_ab)
    assert out["nonfinite"].tolist() == [0, 0]
    others = [c for c in range(n) if c not in (a, b)]
    assert bool((out["gS"][others] == 0).all())
    assert bool((out["gS"][[a, b]] != 0).flatten(1).any(dim=1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. consistency with the unweighted entries


def _raw_gauss(fn_name, mu, cov, kind, weight, W=None):
    """The C entry `fn_name` itself through ctypes; the weighted signature when the name says so (W None: a NULL matrix)."""
    from sqfa_amd import _lib, _native
    lib = _lib.load()
    n, m = cov.shape[0], cov.shape[-1]
    code = _native._dtype_code(cov)
    with _native._on_stream(cov.device) as stream:
        ws, nbytes = _native._workspace(lib.sqfa_gauss_pairwise_workspace_bytes, n, m, code)
        loss = torch.empty((), dtype=cov.dtype, device=DEV)
        flags = torch.empty(2, dtype=torch.int32, device=DEV)
        gmu, gcov = torch.empty_like(mu), torch.empty_like(cov)
        dist_ = torch.empty((n, n), dtype=cov.dtype, device=DEV)
        head = [_native._ptr(mu), _native._ptr(cov), n, m, code, kind, EPS]
        tail = [weight, _native._ptr(loss), _native._ptr(gmu), _native._ptr(gcov), _native._ptr(dist_), _native._ptr(flags),
                _native._ptr(ws), nbytes, stream]
        mid = [_native._ptr(W)] if fn_name.endswith("_weighted") else []
        assert getattr(lib, fn_name)(*head, *mid, *tail) == 0
    torch.cuda.synchronize()
    return loss, gmu, gcov, dist_, flags


def _raw_le(fn_name, S, sqrt_mode, weight, W=None):
    from sqfa_amd import _lib, _native
    lib = _lib.load()
    n, m = S.shape[0], S.shape[-1]
    code = _native._dtype_code(S)
    with _native._on_stream(S.device) as stream:
        ws, nbytes = _native._workspace(lib.sqfa_log_euclidean_workspace_bytes, n, m, code)
        loss = torch.empty((), dtype=S.dtype, device=DEV)
        flags = torch.empty(2, dtype=torch.int32, device=DEV)
        gS = torch.empty_like(S)
        dist_ = torch.empty((n, n), dtype=S.dtype, device=DEV)
        head = [_native._ptr(S), n, m, code, int(sqrt_mode), EPS]
        tail = [weight, _native._ptr(loss), _native._ptr(gS), _native._ptr(dist_), _native._ptr(flags), _native._ptr(ws),
                nbytes, stream]
        mid = [_native._ptr(W)] if fn_name.endswith("_weighted") else []
        assert getattr(lib, fn_name)(*head, *mid, *tail) == 0
    torch.cuda.synchronize()
    return loss, gS, dist_, flags


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("C,K", [(9, 8), (65, 7), (9, 16), (7, 18), (300, 16)])
def test_gauss_null_weights_are_the_old_entry(C, K, kind, dtype):
    mu, cov = (t.to(DEV) for t in _gauss_stats(C, K, dtype))
    old = _raw_gauss("sqfa_gauss_pairwise_loss", mu, cov, kind, _uniform(C))
    new = _raw_gauss("sqfa_gauss_pairwise_loss_weighted", mu, cov, kind, _uniform(C), None)
    for name, a, b in zip(("loss", "gmu", "gcov", "dist", "flags"), old, new):
        assert torch.equal(a, b), name
    # W = ones: the present loss to rounding.  Both sides are the kernel's own arithmetic with the same weight per pair:
    # the floor of the float32 rule (1e-5, a deviation of zero) bounds them without a measured deviation
    ones = normalized(torch.ones(C, C, dtype=torch.float64)).to(dtype).to(DEV)
    w1 = _raw_gauss("sqfa_gauss_pairwise_loss_weighted", mu, cov, kind, 123.0, ones)    # uniform_weight is ignored
    assert torch.equal(w1[3], old[3]) and w1[4].tolist() == [0, 0]
    assert rel_err(w1[0].cpu(), old[0].cpu()) <= _tol(dtype, 0.0, False)
    assert rel_err(w1[1].cpu(), old[1].cpu()) <= _tol(dtype, 0.0, True, kind == 1)
    assert rel_err(w1[2].cpu(), old[2].cpu()) <= _tol(dtype, 0.0, True, kind == 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(LE_OPS))
@pytest.mark.parametrize("n,m", [(9, 4), (65, 4), (25, 16), (5, 32), (4, 63), (300, 16)])
def test_log_euclidean_null_weights_are_the_old_entry(n, m, op, dtype):
    sqrt_mode = LE_OPS[op]
    S = _make_spd(n, m, 1000 * n + m).to(dtype).to(DEV)
    old = _raw_le("sqfa_log_euclidean_pairwise_loss", S, sqrt_mode, _uniform(n))
    new = _raw_le("sqfa_log_euclidean_pairwise_loss_weighted", S, sqrt_mode, _uniform(n), None)
    for name, a, b in zip(("loss", "gS", "dist", "flags"), old, new):
        assert torch.equal(a, b), name
    ones = normalized(torch.ones(n, n, dtype=torch.float64)).to(dtype).to(DEV)
    w1 = _raw_le("sqfa_log_euclidean_pairwise_loss_weighted", S, sqrt_mode, 123.0, ones)
    assert torch.equal(w1[2], old[2]) and w1[3].tolist() == [0, 0]
    # as for the Gaussian entry: the kernel's own arithmetic on both sides, the floor of the float32 rule
    assert rel_err(w1[0].cpu(), old[0].cpu()) <= _tol(dtype, 0.0, False)
    assert rel_err(w1[1].cpu(), old[1].cpu()) <= _tol(dtype, 0.0, True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the loss pinned to the reference's recorded distance matrices

G8 = load_golden("g8_gauss_closure.npz")
G9 = load_golden("g9_log_euclidean_closure.npz")
G8_CASES = [tuple(int(v) for v in c) for c in G8["cases"]]
G9_CASES = [tuple(int(v) for v in c) for c in G9["cases"]]
G8_OPS = {"bhattacharyya": 0, "hellinger": 1, "mahalanobis_sq": 2, "mahalanobis": 3}


def _golden_tol(G, key, op, dtype):
    if dtype == torch.float64:
        return 1e-9
    return max(1e-5, 5 * rel_err(G[f"{key}_{op}_loss_f32"], G[f"{key}_{op}_loss_f64"]))


def _unpack_sym(P):
    n = int(round((np.sqrt(8 * P.shape[-1] + 1) - 1) / 2))
    r, c = np.tril_indices(n)
    M = np.zeros((P.shape[0], n, n), dtype=P.dtype)
    M[:, r, c] = P
    M[:, c, r] = P
    return M


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(G8_OPS))
@pytest.mark.parametrize("C,D,K", G8_CASES)
def test_gauss_weighted_loss_vs_recorded_distances(C, D, K, op, dtype):
    key = f"C{C}_D{D}_K{K}"
    W = make_weights(C, 31 * C + K)
    want = weighted_loss(W, torch.tensor(G8[f"{key}_{op}_D_f64"], dtype=torch.float64))
    mu = torch.tensor(G8[f"{key}_fmu"], dtype=dtype, device=DEV)
    cov = torch.tensor(G8[f"{key}_fcov"], dtype=dtype, device=DEV)
    out = _gauss_call(mu, cov, G8_OPS[op], 0.0, normalized(W).to(dtype).to(DEV))
    err, tol = rel_err(out["loss"].cpu(), want), _golden_tol(G8, key, op, dtype)
    print(f"weighted gauss golden {key} {op} {str(dtype)[6:]}: err {err:.2e} tol {tol:.2e}")
    assert out["nonfinite"].tolist() == [0, 0] and err <= tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(LE_OPS))
@pytest.mark.parametrize("C,D,K", G9_CASES)
def test_log_euclidean_weighted_loss_vs_recorded_distances(C, D, K, op, dtype):
    key = f"C{C}_D{D}_K{K}"
    W = make_weights(C, 31 * C + K)
    want = weighted_loss(W, torch.tensor(G9[f"{key}_{op}_D_f64"], dtype=torch.float64))
    S = torch.tensor(_unpack_sym(G9[f"{key}_fscatters"]), dtype=dtype, device=DEV)
    out = _le_call(S, LE_OPS[op], 0.0, normalized(W).to(dtype).to(DEV))
    err, tol = rel_err(out["loss"].cpu(), want), _golden_tol(G9, key, op, dtype)
    print(f"weighted log-euclidean golden {key} {op} {str(dtype)[6:]}: err {err:.2e} tol {tol:.2e}")
    assert out["nonfinite"].tolist() == [0, 0] and err <= tol


# ---------------------------------------------------------------------------------------------------------------------
# 6. model level: C = 12, D = 16

MC, MD = 12, 16
MODEL_OPS = {"affine_invariant": "smsqfa", "bures_wasserstein": "smsqfa", "log_euclidean": "smsqfa",
             "fisher_rao_lower_bound": "sqfa", "bhattacharyya": "sqfa", "mahalanobis": "sqfa"}
PAIR_KERNEL_OPS = ("affine_invariant", "bures_wasserstein", "fisher_rao_lower_bound")


def _operator(op):
    from sqfa_amd import distances, transport
    return getattr(transport, op) if hasattr(transport, op) and not hasattr(distances, op) else getattr(distances, op)


@functools.lru_cache(maxsize=None)
def _model_stats():
    """float32-rounded statistics, float64 on the CPU (every dtype of every model sees the same values)."""
    g = torch.Generator().manual_seed(4242)
    A = torch.randn(MC, MD, 4 * MD, generator=g, dtype=torch.float64)
    common = torch.randn(MD, 4 * MD, generator=g, dtype=torch.float64)
    cov = 0.6 * (common @ common.T) / (4 * MD) + 0.4 * (A @ A.transpose(1, 2)) / (4 * MD) + 0.05 * torch.eye(MD, dtype=torch.float64)
    cov = (0.5 * (cov + cov.transpose(1, 2))).float().double()
    mu = (0.4 * torch.randn(MC, MD, generator=g, dtype=torch.float64)).float().double()
    return {"means": mu, "covariances": cov}


def _model(op, K, constraint, dtype, seed=3):
    import sqfa_amd
    import model_cases as mc
    kind = MODEL_OPS.get(op, "sqfa")
    torch.manual_seed(seed)
    cls = sqfa_amd.model.SQFA if kind == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    with mc.default_dtype(dtype):
        model = cls(n_dim=MD, n_filters=K, feature_noise=0.01, distance_fun=_operator(op), constraint=constraint)
    if dtype == torch.float64:
        model = model.double()
    model = model.to(DEV)
    if constraint == "orthogonal":
        # torch registers `base` as a transposed view; the native map (and with it the single node) takes a contiguous one
        # (model_cases.set_orthogonal_base does the same with a stored base).  The values, and so the filters, stay.
        par = model.parametrizations.filters[0]
        par.base = par.base.contiguous()
    stats = {k: v.to(dtype).to(DEV) for k, v in _model_stats().items()}
    data = stats if kind == "sqfa" else stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
    return model, data


def _closure(model, data, Wn):
    """One weighted closure evaluation as the fitting loop does it: (loss, gradient of the raw parameter, fused?)."""
    from sqfa_amd import _optim
    prepared = model._prepare_statistics(data)
    model.zero_grad()
    model._pair_weights = Wn
    try:
        fused = model._fused_closure_loss(prepared)
        if fused is not None:
            loss, flags = fused
            assert flags.tolist() == [0, 0]
        else:
            Dm = model.get_class_distances(prepared, regularized=True)
            _optim.check_distances_valid(Dm)
            rows, cols = torch.tril_indices(MC, MC, offset=-1)
            loss = (Wn[rows.to(DEV), cols.to(DEV)] * Dm[rows.to(DEV), cols.to(DEV)]).sum()
        loss.backward()
    finally:
        model._pair_weights = None
    (param,) = list(model.parameters())
    return loss.detach().cpu(), param.grad.detach().cpu().clone(), fused is not None


def _generic_switches(monkeypatch, model=None):
    from sqfa_amd import distances
    monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", False)
    monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", False)
    if model is not None:
        model.SINGLE_NODE_CLOSURE = False


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("constraint", ["sphere", "orthogonal"])
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("op", list(MODEL_OPS))
def test_weighted_fused_closure_equals_generic(op, K, constraint, dtype, monkeypatch):
    from sqfa_amd import _native
    W = make_weights(MC, 900 + K)
    model, data = _model(op, K, constraint, dtype)
    Wn = _native.normalized_pair_weights(W, MC, dtype, DEV)
    raw0 = model.parametrizations.filters.original.detach().clone()
    plan = model._closure_plan(model._prepare_statistics(data))
    assert plan is not None and plan.evaluator == {"affine_invariant": "single_node", "bures_wasserstein": "single_node",
                                                   "fisher_rao_lower_bound": "single_node", "log_euclidean": "log_euclidean",
                                                   "bhattacharyya": "gauss", "mahalanobis": "gauss"}[op]
    l_f, g_f, fused = _closure(model, data, Wn)
    assert fused
    with monkeypatch.context() as mp_:
        _generic_switches(mp_, model)
        l_g, g_g, fused_g = _closure(model, data, Wn)
        assert fused_g == (op in PAIR_KERNEL_OPS)          # the pair-kernel operators keep the chain of autograd nodes
        e_l, e_g = rel_err(l_f, l_g), rel_err(g_f, g_g)
        if op in PAIR_KERNEL_OPS:
            # the bounds of test_single_node_closure_matches_autograd_chain (the same pair kernels on both sides)
            tol_l, tol_g = (1e-12, 1e-10) if dtype == torch.float64 else (2e-6, 2e-4)
            dev = None
        elif dtype == torch.float64:
            tol_l, tol_g, dev = 1e-9, 1e-8, None
        else:
            # the generic closure's own float32 deviation: the same model in float64 on the same float32-rounded inputs
            m64, d64 = _model(op, K, constraint, torch.float64)
            m64.SINGLE_NODE_CLOSURE = False
            with torch.no_grad():
                m64.parametrizations.filters.original.copy_(raw0.double())
                if constraint == "orthogonal":
                    m64.parametrizations.filters[0].base.copy_(model.parametrizations.filters[0].base.double())
            l64, g64, _ = _closure(m64, d64, _native.normalized_pair_weights(W, MC, torch.float32, DEV).double())
            dev = (rel_err(l_g, l64), rel_err(g_g, g64))
            tol_l, tol_g = max(1e-5, 5 * dev[0]), max(1e-5, 5 * dev[1])
    model.SINGLE_NODE_CLOSURE = True
    print(f"weighted closure {op} K={K} {constraint} {str(dtype)[6:]}: loss {e_l:.2e} (tol {tol_l:.1e}) grad {e_g:.2e} (tol {tol_g:.1e}) dev {dev}")
    assert e_l <= tol_l and e_g <= tol_g
    # the comparison can tell: the uniform closure is further away than ten times what the weighted ones are allowed
    l_u, g_u, _ = _closure(model, data, None)
    assert rel_err(l_u, l_g) > 10 * tol_l or rel_err(g_u, g_g) > 10 * tol_g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(MODEL_OPS))
def test_weighted_fit_is_graph_captured_and_follows_the_eager_fit(op, dtype, monkeypatch):
    from sqfa_amd import _optim
    W = make_weights(MC, 904)
    replays = []
    orig_replay = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays.append(1)
        return orig_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counting_replay)
    model, data = _model(op, 4, "sphere", dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")     # the loop warns when a capture fails
        loss, _ = model.fit(data_statistics=data, max_epochs=5, show_progress=False, return_loss=True, pair_weights=W)
    assert len(replays) > 0 and loss.shape == (5,)
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]
    assert model._pair_weights is None
    if dtype != torch.float64:
        return
    n_graph = len(replays)
    with monkeypatch.context() as mp_:
        _generic_switches(mp_)
        mp_.setattr(_optim, "GRAPH_CLOSURE", False)
        eager, data = _model(op, 4, "sphere", dtype)
        eager.SINGLE_NODE_CLOSURE = False
        loss_e, _ = eager.fit(data_statistics=data, max_epochs=5, show_progress=False, return_loss=True, pair_weights=W)
    assert len(replays) == n_graph
    err = rel_err(loss.double().numpy(), loss_e.double().numpy())
    print(f"weighted trajectory {op}: fused+graph vs eager generic {err:.3e}")
    assert err <= 1e-8      # the bound of test_pairwise_fit_fused_equals_generic (fused against generic trajectories)


def test_wasserstein_generic_closure_takes_weights():
    from sqfa_amd import transport
    W = make_weights(MC, 905)
    model, data = _model("wasserstein", 4, "sphere", torch.float64)
    assert model.distance_fun is transport.wasserstein and not model._has_fused_closure()
    with torch.no_grad():
        want = weighted_loss(W, model.get_class_distances(data, regularized=True)).item()
        uniform = weighted_loss(torch.ones(MC, MC, dtype=torch.float64), model.get_class_distances(data, regularized=True)).item()
    loss, _ = model.fit(data_statistics=data, max_epochs=3, show_progress=False, return_loss=True, pair_weights=W)
    assert abs(loss[0].item() - want) <= (1e-9 + 2.0 ** -23) * abs(want)       # fit() records its losses in float32
    assert abs(want - uniform) > 1e-3 * abs(uniform)
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]


# ---------------------------------------------------------------------------------------------------------------------
# 7. sharded: two ranks share cuda:0 over gloo


def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sqfa_amd._optim as opt
        from pair_weight_cases import make_weights as mw
        from sqfa_amd import _native
        from sqfa_amd.parallel import ClassShard, PairShard
        import test_gpu_pair_weights as me
        W = mw(me.MC, 906)
        out = {}
        model, data = me._model("affine_invariant", 3, "sphere", torch.float64)
        Wn = _native.normalized_pair_weights(W, me.MC, torch.float64, me.DEV)
        single = me._closure(model, data, Wn)
        out["single"] = (single[0].numpy(), single[1].numpy())
        model.pair_shard = PairShard()
        sharded = me._closure(model, data, Wn)
        out["pair_shard"] = (sharded[0].numpy(), sharded[1].numpy())
        # the same through ShardedClosure: graphs around the all-reduce (three eager passes, the capture, two replays)
        prepared = model._prepare_statistics(data)
        model._pair_weights = Wn
        try:
            assert opt.ShardedClosure.supported(model, prepared)
            split = opt.ShardedClosure(model, prepared)
            for _ in range(opt.GRAPH_WARMUP_CLOSURES + 3):
                packed, grad = split.run()
            torch.cuda.synchronize()
            out["split"] = (packed[0].cpu().numpy(), grad.cpu().numpy(), packed[1:3].cpu().tolist(), split.state)
        finally:
            model._pair_weights = None
        # a sharded fit: rank 1 is handed other weights -- rank 0's are broadcast with the rest of the replicated state
        fit_model, data = me._model("affine_invariant", 3, "sphere", torch.float64)
        fit_model.pair_shard = PairShard()
        mine = W if rank == 0 else mw(me.MC, 907)
        loss, _ = fit_model.fit(data_statistics=data, max_epochs=3, show_progress=False, return_loss=True, pair_weights=mine)
        out["fit"] = (loss.numpy(), fit_model.filters.detach().cpu().numpy())
        # class-sharded statistics (uneven shards; SQFA): the weights stay (C, C) over all classes
        for name, class_sharded in (("fit_single", False), ("fit_class_shard", True)):
            cs_model, stats = me._model("fisher_rao_lower_bound", 3, "sphere", torch.float64)
            lo, hi = (0, 5) if rank == 0 else (5, me.MC)
            if class_sharded:
                cs_model.pair_shard = PairShard()
                cs_model.class_shard = ClassShard(hi - lo)
                stats = {k: v[lo:hi].contiguous() for k, v in stats.items()}
            loss, _ = cs_model.fit(data_statistics=stats, max_epochs=3, show_progress=False, return_loss=True, pair_weights=W)
            out[name] = (loss.numpy(), cs_model.filters.detach().cpu().numpy())
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_weighted_match_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31100 + os.getpid() % 2000
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, r0), (_, r1) = results
    l1, g1 = r0["single"]
    for name in ("pair_shard", "split"):
        assert np.array_equal(r0[name][0], r1[name][0]) and np.array_equal(r0[name][1], r1[name][1])   # identical on both ranks
        l, g = r0[name][0], r0[name][1]
        # the bounds of test_two_ranks_on_one_gpu_match_single_process (float64)
        assert abs(float(l) - float(l1)) < 1e-11 * abs(float(l1)), name
        assert np.linalg.norm(g - g1) < 1e-8 * np.linalg.norm(g1), name
    assert r0["split"][2] == [0.0, 0.0] and r0["split"][3] == "on" and r1["split"][3] == "on"
    # the fit: both ranks used rank 0's weights, and start from the single-process weighted loss
    assert np.array_equal(r0["fit"][0], r1["fit"][0]) and np.array_equal(r0["fit"][1], r1["fit"][1])
    assert abs(float(r0["fit"][0][0]) - float(l1)) <= (1e-9 + 2.0 ** -23) * abs(float(l1))
    assert r0["fit"][0][-1] < r0["fit"][0][0]
    # class-sharded: the bounds of test_sharded_closure_runs_as_two_graphs_around_one_all_reduce against the single process
    (l_cs, F_cs), (l_s, F_s) = r0["fit_class_shard"], r0["fit_single"]
    assert np.array_equal(l_cs, r1["fit_class_shard"][0]) and np.array_equal(F_cs, r1["fit_class_shard"][1])
    assert np.abs(l_cs - l_s).max() < 1e-9 and np.linalg.norm(F_cs - F_s) < 1e-8 * np.linalg.norm(F_s)


# ---------------------------------------------------------------------------------------------------------------------
# 8. a class that is not positive definite, with weights


@pytest.mark.parametrize("family", ["gauss", "log_euclidean"])
def test_indefinite_class_with_weights_is_reported_not_a_fault(family):
    """NaN distances are counted in the flags whatever the weights are -- also when every pair of the bad class has weight
    zero -- and fit() turns them into the reference's ValueError."""
    C, K = 12, 4
    P = C * (C - 1) // 2
    W = make_weights(C, 908)
    W_masked = W.clone()
    W_masked[3, :] = 0.0
    W_masked[:, 3] = 0.0
    for weights in (W, W_masked):
        Wn = normalized(weights).to(DEV)
        if family == "gauss":
            mu, cov = (t.to(DEV) for t in _gauss_stats(C, K, torch.float64))
            cov = cov.clone()
            cov[3] = -4.0 * cov[3]
            out = _gauss_call(mu, cov, 0, 0.0, Wn)
        else:
            S = _make_spd(C, K, 5).to(DEV)
            S[3] = -4.0 * S[3]
            out = _le_call(S, True, 0.0, Wn)
        n_nan, n_inf = out["nonfinite"].tolist()
        assert n_nan >= 1 and n_nan + n_inf <= P
    op = "bhattacharyya" if family == "gauss" else "log_euclidean"
    for weights in (W, W_masked):
        model, data = _model(op, 4, "sphere", torch.float64)
        bad = data["covariances"] if isinstance(data, dict) else data
        bad[3] = -4.0 * bad[3]
        with pytest.raises(ValueError, match="Some distances between classes are NaN"):
            model.fit(data_statistics=data, max_epochs=2, show_progress=False, pair_weights=weights)
        assert model._pair_weights is None
