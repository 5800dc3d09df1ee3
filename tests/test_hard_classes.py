"""CPU tests of the close, ill-conditioned classes of tests/hard_classes.py: the inputs have the properties they claim, the
float64 truth agrees with a 50-digit mpmath evaluation of the defining formulas to a tenth of every bound asserted with it
(tests/test_gpu_close_classes.py: max(the family's constant, 5 x the float64 yardstick)), and the package's torch
expressions stay finite, non-negative and above sqrt(eps) on them in both dtypes."""
import functools

import numpy as np
import pytest
import torch

import hard_classes as hc
import hard_yardsticks as hy

N_MP = 5
SIZES_MP = (4, 8, 17)
CLOSE = ("L1", "L2", "L3")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 8, 17, 33, 64])
@pytest.mark.parametrize("level", CLOSE)
def test_input_properties(level, m):
    n = 7
    kw = hc.LEVELS[level]
    mu, S = hc.level_classes(level, n, m, seed=1000 * n + m)
    assert np.array_equal(S, S.transpose(0, 2, 1))
    lam = np.linalg.eigvalsh(S)
    assert lam.min() > 0
    cond = lam[:, -1] / lam[:, 0]
    assert (cond <= 2 * kw["cond"]).all() and (cond >= kw["cond"] / 2).all(), cond
    assert np.array_equal(S[n - 1], S[1]) and np.array_equal(mu[n - 1], mu[1])
    if kw["round32"]:
        assert np.array_equal(S, S.astype(np.float32).astype(np.float64))
        assert np.array_equal(mu, mu.astype(np.float32).astype(np.float64))
    ld = hc.pair_terms(mu, S)["ld"]
    assert ld[n - 1, 1] == 0 and ld[1, n - 1] == 0
    pairs = ~np.eye(n, dtype=bool)
    pairs[n - 1, 1] = pairs[1, n - 1] = False
    scale = kw["t"] ** 2 * m          # 1/2 |M|_F^2 with M = t (E_i - E_j) / 2, |E|_F^2 about m
    assert (ld[pairs] >= scale / 50).all() and (ld[pairs] <= scale).all(), (ld[pairs].min() / scale, ld[pairs].max() / scale)


def test_mixed_classes_hold_far_and_close_pairs():
    for family in hy.FAMILIES:
        mu, S = hy.inputs(family, "mixed", 7, 8)
        assert S.shape == (7, 8, 8) and np.array_equal(S, S.transpose(0, 2, 1)) and np.linalg.eigvalsh(S).min() > 0
        ld = hc.pair_terms(mu, S)["ld"]
        close = ld[np.ix_([1, 4, 5, 6], [1, 4, 5, 6])][~np.eye(4, dtype=bool)]
        far = ld[:4, :4][~np.eye(4, dtype=bool)]
        assert close.max() <= 1e-4 and far.min() >= 1e3 * close.max(), (family, close.max(), far.min())


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mp_values(family, level, m):
    """Every base quantity V_ij of the ordered pairs with dV_ij/dS_i and dV_ij/dmu_i, by the DEFINING formulas (three
    log-determinants, the textbook traces, differences of inverses) in 50-digit arithmetic, rounded to float64 at the end."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    mu, S = hy.inputs(family, level, N_MP, m)
    n = N_MP
    Sm = [mpmath.matrix(S[c].tolist()) for c in range(n)]
    mum = [mpmath.matrix(mu[c].tolist()) for c in range(n)]
    P = [mpmath.inverse(A) for A in Sm]
    ld = [mpmath.log(mpmath.det(A)) for A in Sm]
    keys = ("stein", "jc", "jeffreys", "Q")
    V = {k: np.zeros((n, n)) for k in keys}
    dS = {k: np.zeros((n, n, m, m)) for k in keys}
    dmu = {k: np.zeros((n, n, m)) for k in ("jeffreys", "Q")}
    f = lambda A: np.array(A.tolist(), dtype=object).astype(np.float64)
    for i in range(n):
        for j in range(i):
            Pbar = mpmath.inverse((Sm[i] + Sm[j]) / 2)
            stein = mpmath.log(mpmath.det((Sm[i] + Sm[j]) / 2)) - (ld[i] + ld[j]) / 2
            tr = lambda A: sum(A[k, k] for k in range(m))
            jc = (tr(P[j] * Sm[i]) + tr(P[i] * Sm[j])) / 2 - m
            for a, b, sign in ((i, j, 1), (j, i, -1)):
                delta = (mum[i] - mum[j]) * sign
                s = Pbar * delta
                Pad, Pbd = P[a] * delta, P[b] * delta
                jm = ((Pad + Pbd).T * delta)[0, 0] / 2
                V["stein"][a, b], V["jc"][a, b] = float(stein), float(jc)
                V["jeffreys"][a, b], V["Q"][a, b] = float(jc + jm), float((delta.T * s)[0, 0])
                dS["stein"][a, b] = f((Pbar - P[a]) / 2)
                Gjc = (P[b] - P[a] * Sm[b] * P[a]) / 2
                dS["jc"][a, b] = f(Gjc)
                dS["jeffreys"][a, b] = f(Gjc - Pad * Pad.T / 2)
                dS["Q"][a, b] = f(-(s * s.T) / 2)
                dmu["jeffreys"][a, b] = f(Pad + Pbd).ravel()
                dmu["Q"][a, b] = f(2 * s).ravel()
    return V, dS, dmu


def _mp_log_euclidean(level, m, sqrt_mode):
    """The log-Euclidean loss, distances and gradient (Daleckii-Krein) in 50-digit arithmetic."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    _, S = hy.inputs("log_euclidean", level, N_MP, m)
    n = N_MP
    W = hy.weights(n, False)
    eig = [mpmath.eigsy(mpmath.matrix(S[c].tolist())) for c in range(n)]
    diag = lambda v: mpmath.diag([v[k] for k in range(m)])
    Lg = [Q * diag([mpmath.log(E[k]) for k in range(m)]) * Q.T for E, Q in eig]
    D = [[mpmath.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i != j:
                d = Lg[i] - Lg[j]
                v = sum(d[a, b] ** 2 for a in range(m) for b in range(m))
                D[i][j] = mpmath.sqrt(v + hc.EPS) if sqrt_mode else v
    gcov = np.zeros((n, m, m))
    for i in range(n):
        GL = mpmath.zeros(m)
        for j in range(n):
            if i != j:
                GL += (Lg[i] - Lg[j]) * (2 * mpmath.mpf(float(W[i, j])) * (1 / (2 * D[i][j]) if sqrt_mode else 1))
        E, Q = eig[i]
        inner = Q.T * GL * Q
        for a in range(m):
            for b in range(m):
                inner[a, b] *= 1 / E[a] if a == b else (mpmath.log(E[a]) - mpmath.log(E[b])) / (E[a] - E[b])
        G = Q * inner * Q.T
        gcov[i] = np.array(((G + G.T) / 2).tolist(), dtype=object).astype(np.float64)
    dist = np.array([[float(x) for x in row] for row in D])
    np.fill_diagonal(dist, np.sqrt(hc.EPS) if sqrt_mode else 0.0)
    r, c = np.tril_indices(n, -1)
    loss = float(sum(mpmath.mpf(float(W[a, b])) * D[a][b] for a, b in zip(r, c)))
    return {"loss": loss, "dist": dist, "gcov": gcov, "gmu": None}


def _mp_reference(op, level, m):
    family, mode, means, _ = hy.OPS[op]
    if family == "log_euclidean":
        return _mp_log_euclidean(level, m, mode)
    V, dS, dmu = _mp_values(family, level, m)
    W = hy.weights(N_MP, False)
    if family == "stein":
        return hc._assemble(W, *hc._root(V["stein"], dS["stein"], None, mode, hc.EPS))
    if family == "jeffreys":
        k = "jeffreys" if means else "jc"
        return hc._assemble(W, *hc._root(V[k], dS[k], dmu[k] if means else None, mode, hc.EPS))
    if mode in (2, 3):
        return hc._assemble(W, *hc._root(V["Q"], dS["Q"], dmu["Q"], mode == 3, hc.EPS))
    Bh, dB, dm = V["Q"] / 8 + V["stein"] / 2, dS["Q"] / 8 + dS["stein"] / 2, dmu["Q"] / 8
    if mode == 0:
        return hc._assemble(W, Bh, 0.0, dB, dm)
    D = np.sqrt(-np.expm1(-Bh) + hc.EPS)
    c = 0.5 * np.exp(-Bh) / D
    return hc._assemble(W, D, np.sqrt(hc.EPS), c[:, :, None, None] * dB, c[:, :, None] * dm)


@pytest.mark.parametrize("m", SIZES_MP)
@pytest.mark.parametrize("level", CLOSE)
@pytest.mark.parametrize("family", list(hy.FAMILIES))
def test_truth_against_mpmath(family, level, m):
    """The truth's own error is at most a tenth of the float64 bound asserted with it (the float32 bounds are wider).  L3
    runs at hy.L3_COND's condition number for a family whose truth misses this at 1e6 (log-Euclidean: its truth is the
    float64 definition, with error eps cond / t)."""
    for op in hy.FAMILIES[family]:
        want = _mp_reference(op, level, m)
        got = hy.truth(op, level, N_MP, m)
        yard = hy.yardstick(op, level, N_MP, m, "float64")
        err_of = hy.metric(op)
        for name in hy.names(op):
            err = err_of(got[name], want[name])
            bound = max(hy.constant(op, name, "float64"), 5 * err_of(yard[name], want[name]))
            print(f"{op} {level} m={m} {name}: truth against mpmath {err:.2e}, float64 bound {bound:.2e}")
            assert err <= 0.1 * bound, (op, level, m, name, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
def _package_call(op, mu, S):
    from sqfa_amd import distances, divergences, logdet
    family, _, means, _ = hy.OPS[op]
    fn = getattr({"gauss": distances, "stein": logdet, "jeffreys": divergences, "log_euclidean": distances}[family], op)
    if means:
        stats = {"means": mu, "covariances": S}
        return fn(stats, stats)
    return fn(S, S)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("m", [8, 16, 33])
@pytest.mark.parametrize("level", ["L1", "L2", "mixed"])
@pytest.mark.parametrize("op", list(hy.OPS))
def test_package_expressions_stay_valid(op, level, m, dtype):
    """Finite, divergences >= 0, square-root distances >= sqrt(eps) (1 - 1e-6), values and gradients, on every pair."""
    n = 7
    tdt = hy.DTYPES[dtype][0]
    mu, S = (torch.from_numpy(np.array(a)).to(tdt) for a in hy.inputs(hy.OPS[op][0], level, n, m))
    S.requires_grad_(True)
    D = _package_call(op, mu, S)
    assert D.shape == (n, n) and torch.isfinite(D).all(), (op, level, m, dtype, int((~torch.isfinite(D)).sum()))
    if hy.OPS[op][3]:
        assert D.min().item() >= hc.EPS ** 0.5 * (1 - 1e-6), D.min().item()
    else:
        assert D.min().item() >= 0, D.min().item()
    r, c = torch.tril_indices(n, n, offset=-1)
    (g,) = torch.autograd.grad(D[r, c].sum(), S)
    assert torch.isfinite(g).all()
