"""What tests/test_hard_classes.py and tests/test_gpu_close_classes.py share: the operators of the four class-pair families,
their inputs on the levels of tests/hard_classes.py, the float64 truth, each family's existing oracle expression evaluated
in the dtype under test on the CPU (the yardstick), the family's existing error metric and its existing constants.

The yardstick's raw divergence goes through max(., 0) before any square root (`clamp=True` of the oracles; the package's
own Jeffreys expression does it itself), so it is finite where the plain expression is NaN."""
import functools

import numpy as np
import torch

import gauss_oracle
import hard_classes as hc
import jeffreys_oracle as jo
import stein_oracle as so
from conftest import rel_err

EPS = hc.EPS
# op -> (family, mode of the native call, takes means, D is a square root)
OPS = {
    "bhattacharyya": ("gauss", 0, True, False), "hellinger": ("gauss", 1, True, True),
    "mahalanobis_sq": ("gauss", 2, True, False), "mahalanobis": ("gauss", 3, True, True),
    "stein": ("stein", False, False, False), "stein_root": ("stein", True, False, True),
    "jeffreys": ("jeffreys", False, True, False), "jeffreys_root": ("jeffreys", True, True, True),
    "jeffreys_spd": ("jeffreys", False, False, False), "jeffreys_spd_root": ("jeffreys", True, False, True),
    "log_euclidean_sq": ("log_euclidean", False, False, False), "log_euclidean": ("log_euclidean", True, False, True),
}
FAMILIES = {f: [op for op, spec in OPS.items() if spec[0] == f] for f in ("gauss", "stein", "jeffreys", "log_euclidean")}
QUANTITIES = ("loss", "dist", "gcov", "gmu")
LEVELS = ("L1", "L2", "L3", "mixed")
# L3's condition number per family where the truth is not good enough at 1e6 (tests/test_hard_classes.py measures it)
# log-Euclidean: the truth is the float64 definition, error about eps cond / t; at 1e2 it reached 1.9e-10 against the 1e-10
# it may have, at 1e1 it holds
L3_COND = {"log_euclidean": 1e1}
DTYPES = {"float32": (torch.float32, np.float32), "float64": (torch.float64, np.float64)}


def _le():
    import test_gpu_log_euclidean_closure as le
    return le


def level_dtypes(level):
    return ("float64",) if level == "L3" else ("float64", "float32")


@functools.lru_cache(maxsize=None)
def inputs(family, level, n, m):
    """(mu (n,m), S (n,m,m)) float64 numpy, read-only.  The close levels are the same classes for every family (L3 at the
    family's condition number); mixed starts from the family's own generator."""
    seed = 1000 * n + m
    if level != "mixed":
        kw = dict(hc.LEVELS[level])
        if level == "L3":
            kw["cond"] = L3_COND.get(family, kw["cond"])
        mu, S = hc.close_classes(n, m, seed=seed, **kw)
    else:
        far = n - 3
        if family == "gauss":
            fmu, fS = (t.numpy() for t in gauss_oracle.inputs(far, m, seed))
        elif family == "jeffreys":
            fmu, fS = (t.numpy() for t in jo.make_classes(far, m, seed))
        elif family == "stein":
            fmu, fS = None, so.make_classes(far, m, seed)
        else:
            fmu, fS = None, _le()._make_spd(far, m, seed).numpy()
        if fmu is None:
            fmu = np.random.default_rng(seed).standard_normal((far, m)) * 0.3
        mu, S = hc.mixed_classes(fmu, fS, seed)
    mu.setflags(write=False)
    S.setflags(write=False)
    return mu, S


@functools.lru_cache(maxsize=None)
def weights(n, weighted):
    W = hc.random_weights(n, seed=n) if weighted else hc.uniform_weights(n)
    W = W.astype(np.float32).astype(np.float64)      # both dtypes see the same numbers
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def _terms(family, level, n, m):
    return hc.pair_terms(*inputs(family, level, n, m))


@functools.lru_cache(maxsize=None)
def truth(op, level, n, m, weighted=False):
    family, mode, means, _ = OPS[op]
    mu, S = inputs(family, level, n, m)
    W = weights(n, weighted)
    if family == "log_euclidean":
        return hc.log_euclidean_truth(S, mode, W)
    terms = _terms(family, level, n, m)
    if family == "gauss":
        return hc.gauss_truth(mu, S, mode, W, terms)
    if family == "stein":
        return hc.stein_truth(S, mode, W, terms)
    return hc.jeffreys_truth(mu if means else None, S, mode, W, terms)


def _log_euclidean_expression(S, sqrt_mode, W):
    """The expression of test_gpu_log_euclidean_closure.py (its _spd_log and _rows_D) with per-pair weights."""
    le = _le()
    n = S.shape[0]
    Sv = S.clone().requires_grad_(True)
    Lg = le._spd_log(Sv)
    D = le._rows_D(Lg, Lg, sqrt_mode)
    r, c = torch.tril_indices(n, n, offset=-1)
    loss = (W[r, c] * D[r, c]).sum()
    (g,) = torch.autograd.grad(loss, Sv)
    D = D.detach().clone()
    D.fill_diagonal_(EPS ** 0.5 if sqrt_mode else 0.0)
    return {"loss": loss.detach(), "dist": D, "gcov": 0.5 * (g + g.transpose(1, 2)), "gmu": None}


@functools.lru_cache(maxsize=None)
def yardstick(op, level, n, m, dtype, weighted=False):
    """The family's oracle expression in `dtype` ("float32" | "float64") on the CPU: dict of float64 numpy arrays."""
    family, mode, means, _ = OPS[op]
    tdt, ndt = DTYPES[dtype]
    mu, S = inputs(family, level, n, m)
    W = weights(n, weighted)
    tmu, tS, tW = (torch.from_numpy(np.array(a)).to(tdt) for a in (mu, S, W))
    if family == "gauss":
        loss, gmu, gcov, D = gauss_oracle._full_expression(tmu, tS, mode, None, dtype=tdt, clamp=True, W=tW)
        out = {"loss": loss, "dist": D, "gcov": gcov, "gmu": gmu}
    elif family == "stein":
        S_ = S.astype(ndt)
        e = so.loss_and_gradient(S_, mode, None, W.astype(ndt), dtype=ndt, div=so.three_logdets(S_, S_, ndt), clamp=True)
        out = {"loss": e["loss"], "dist": e["dist"], "gcov": e["grad"], "gmu": None}
    elif family == "jeffreys":
        from sqfa_amd import divergences
        out = jo.loss_and_gradients(tmu if means else None, tS, mode, None, tW, fn=divergences._jeffreys_matrix)
    else:
        out = _log_euclidean_expression(tS, mode, tW)
    return {k: None if v is None else np.asarray(v, np.float64) for k, v in out.items()}


def metric(op):
    """The family's existing error metric."""
    return so.max_rel if OPS[op][0] == "stein" else (lambda got, want: float(rel_err(got, want)))


def per_pair(got, want):
    """max over the pairs i != j of |got - want| / want."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    off = ~np.eye(want.shape[0], dtype=bool)
    return float((np.abs(got - want)[off] / want[off]).max())


def constant(op, name, dtype):
    """The family's existing tolerance constant (test_gpu_gauss_kernel_rows.py, test_gpu_stein.py, test_gpu_jeffreys.py,
    test_gpu_log_euclidean_closure.py)."""
    if dtype == "float32":
        return 1e-5
    family = OPS[op][0]
    if family == "stein":
        return 1e-11
    if name in ("gcov", "gmu"):
        return 1e-6 if op == "hellinger" else 1e-8
    return 1e-9


def names(op):
    return [q for q in QUANTITIES if q != "gmu" or OPS[op][2]]
