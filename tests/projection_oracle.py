"""float64 numpy / torch-CPU definition of the projection side of a closure evaluation -- everything around the pair
distance: the sphere map, T = Psi F^T, S = F T + noise I (or its Calvo-Oller embedding), the backward product, the means
gradient and the sphere backward (kernels: project_kernel.hip, feature_kernels.hip, closure_glue.hip).  Imports nothing
from sqfa_amd.

Every function returns Val(value, mag, n):
    value  the quantity in float64 (or in `dtype`, when one is passed: the SAME expression evaluated in that precision --
           tests/test_projection_oracle.py uses it to show that a plain float32 evaluation stays inside the bound)
    mag    its magnitude: the same expression with every term replaced by its absolute value (|Psi| |F|^T, ...)
    n      the number of terms summed into an element, from the shapes alone
and a result `out` of arithmetic with unit roundoff u is accepted when, elementwise,
    |out - value| <= C_FACTOR * n * u * mag                                      (ratio() <= C_FACTOR)
the standard bound of a sum of n products evaluated in any order (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1: gamma_n = n u / (1 - n u)), with C_FACTOR = 2 for fma-or-not and the final store.  Where a quantity is a chain of
such sums, n is the sum of the links' counts and mag the composed magnitude: the first-order bound of the chain.
"""
import collections

import numpy as np

Val = collections.namedtuple("Val", "value mag n")
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
C_FACTOR = 2.0
F64 = np.float64


def unit(dtype):
    return UNIT[np.dtype(dtype)]


def rounded(a, dtype):
    """`a` rounded to `dtype`, as float64: what a kernel of that dtype is given."""
    return np.asarray(a, dtype=F64).astype(dtype).astype(F64)


def ratio(out, val, dtype):
    """Largest |out - value| / (n u mag) over the elements (the test asserts <= C_FACTOR).  Elements of zero magnitude
    (or n == 0: an empty class group) must be reproduced exactly: inf otherwise."""
    out = np.asarray(out, dtype=F64)
    value = np.asarray(val.value, dtype=F64)
    assert out.shape == value.shape, (out.shape, value.shape)
    err = np.abs(out - value)
    den = np.broadcast_to(np.asarray(val.n, dtype=F64) * unit(dtype) * np.asarray(val.mag, dtype=F64), err.shape)
    if not np.isfinite(out).all():
        return float("inf")
    zero = den == 0
    if (err[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / den[~zero]).max())


def _abs64(a):
    return np.abs(np.asarray(a, dtype=F64))


# ---- the kernels' operations --------------------------------------------------------------------------------------


def project(Psi, F, dtype=F64):
    """T_c = Psi_c F^T: (C,D,D), (K,D) -> (C,D,K).  n = D."""
    P, Fd = np.asarray(Psi).astype(dtype), np.asarray(F).astype(dtype)
    return Val(np.matmul(P, Fd.T), np.matmul(_abs64(P), _abs64(Fd).T), P.shape[-1])


def feature_scatters(F, T, noise, means_f=None, dtype=F64):
    """S_c = F T_c + noise I -> (C,K,K); with the projected means m (C,K) the Calvo-Oller embedding
    [[S + m m^T, m], [m^T, 1]] -> (C,K+1,K+1).  n = D + 2 (the products, the noise, m m^T); the border and the corner
    are copies (any n >= 0 does: they must be exact up to n u |m|, and are exact)."""
    Fd, Td = np.asarray(F).astype(dtype), np.asarray(T).astype(dtype)
    K, D = Fd.shape
    C = Td.shape[0]
    eye = np.eye(K, dtype=dtype)
    S = np.matmul(Fd[None], Td) + dtype(noise) * eye
    mag = np.matmul(_abs64(Fd)[None], _abs64(Td)) + abs(float(dtype(noise))) * np.eye(K)
    if means_f is None:
        return Val(S, mag, D + 2)
    m = np.asarray(means_f).astype(dtype)
    E = np.empty((C, K + 1, K + 1), dtype=dtype)
    E[:, :K, :K] = S + m[:, :, None] * m[:, None, :]
    E[:, :K, K] = m
    E[:, K, :K] = m
    E[:, K, K] = 1
    Em = np.empty((C, K + 1, K + 1))
    Em[:, :K, :K] = mag + _abs64(m)[:, :, None] * _abs64(m)[:, None, :]
    Em[:, :K, K] = _abs64(m)
    Em[:, K, :K] = _abs64(m)
    Em[:, K, K] = 1
    return Val(E, Em, D + 2)


def group_counts(C, n_groups):
    return np.array([len(range(g, C, n_groups)) for g in range(n_groups)])


def backward_partials(G, T, n_groups, dtype=F64):
    """P_g = sum over the classes c = g, g + n_groups, ... of (G_c + G_c^T)[:K,:K] T_c^T -> (n_groups,K,D); G (C,ldg,ldg)
    with ldg >= K.  n = 2 K per class of the group (each of G_ab T_db and G_ba T_db is a term); a group without a class
    has n = 0: exact zeros."""
    Gd, Td = np.asarray(G).astype(dtype), np.asarray(T).astype(dtype)
    C, D, K = Td.shape
    Gk = Gd[:, :K, :K]
    per_class = np.matmul(Gk + Gk.transpose(0, 2, 1), Td.transpose(0, 2, 1))
    per_mag = np.matmul(_abs64(Gk) + _abs64(Gk).transpose(0, 2, 1), _abs64(Td).transpose(0, 2, 1))
    P = np.zeros((n_groups, K, D), dtype=dtype)
    mag = np.zeros((n_groups, K, D))
    for g in range(min(n_groups, C)):
        P[g] = per_class[g::n_groups].sum(0)
        mag[g] = per_mag[g::n_groups].sum(0)
    return Val(P, mag, (2 * K * group_counts(C, n_groups))[:, None, None])


def embed_backward_means(gE, m, dtype=F64):
    """g_m = (G + G^T) m + gE[:K,K] + gE[K,:K] with G = gE[:K,:K]: (C,K+1,K+1), (C,K) -> (C,K).  n = 2 K + 2."""
    g, md = np.asarray(gE).astype(dtype), np.asarray(m).astype(dtype)
    K = md.shape[1]
    G = g[:, :K, :K]
    out = np.einsum("cab,cb->ca", G + G.transpose(0, 2, 1), md) + g[:, :K, K] + g[:, K, :K]
    Ga = _abs64(G)
    mag = np.einsum("cab,cb->ca", Ga + Ga.transpose(0, 2, 1), _abs64(md)) + _abs64(g[:, :K, K]) + _abs64(g[:, K, :K])
    return Val(out, mag, 2 * K + 2)


def sphere_forward(X, dtype=F64):
    """(F, norms): norms_k = ||X_k||, F = X / norms.  norms: D squares and the root, n = D + 1 (the root halves the
    relative error of the sum; kept); F: one division more, n = D + 2."""
    Xd = np.asarray(X).astype(dtype)
    D = Xd.shape[1]
    norms = np.sqrt((Xd * Xd).sum(1))
    F = Xd / norms[:, None]
    n64 = np.sqrt((_abs64(Xd) ** 2).sum(1))
    return Val(F, _abs64(Xd) / n64[:, None], D + 2), Val(norms, n64, D + 1)


def sphere_backward(X, norms, partials, extra, gloss, dtype=F64):
    """dL/dX = gloss (gF - F (F . gF)) / norms with gF = extra + sum_g partials[g] and F = X / norms; norms None (no
    constraint): gloss gF.  partials (n_groups,K,D) or None, extra (K,D) or None, gloss scalar or None (= 1).
    Magnitude |gloss| (|gF| + |F| sum |F| |gF|) / norms.  n: the n_groups + 1 terms of gF, the D terms of the dot product
    and five elementwise roundings (X / norms, F dot, the subtraction, gloss, / norms); n_groups + 2 without norms."""
    Xd = np.asarray(X).astype(dtype)
    K, D = Xd.shape
    n_groups = 0 if partials is None else np.asarray(partials).shape[0]
    g = np.zeros((K, D), dtype=dtype)
    gm = np.zeros((K, D))
    if extra is not None:
        g = g + np.asarray(extra).astype(dtype)
        gm = gm + _abs64(np.asarray(extra).astype(dtype))
    if n_groups:
        g = g + np.asarray(partials).astype(dtype).sum(0)
        gm = gm + _abs64(np.asarray(partials).astype(dtype)).sum(0)
    scale = dtype(1.0 if gloss is None else gloss)
    if norms is None:
        return Val(scale * g, abs(float(scale)) * gm, n_groups + 2)
    nd = np.asarray(norms).astype(dtype)[:, None]
    F = Xd / nd
    out = scale * (g - F * (F * g).sum(1, keepdims=True)) / nd
    Fa, na = _abs64(F), _abs64(nd)
    mag = abs(float(scale)) * (gm + Fa * (Fa * gm).sum(1, keepdims=True)) / na
    return Val(out, mag, n_groups + 1 + D + 5)


# ---- the whole stage ---------------------------------------------------------------------------------------------


def _orthogonal_parts(X):
    """V, M^-1, W of tests/orthogonal_oracle.py (compact WY form of torch's Householder map)."""
    X = np.asarray(X, dtype=F64)
    K, D = X.shape
    V = np.tril(X.T, -1)
    V[np.arange(K), np.arange(K)] = 1.0
    G = V.T @ V
    M = np.triu(G, 1) + np.diag(np.diag(G) / 2.0)
    Minv = np.linalg.inv(M)
    return V, Minv, Minv @ V[:K].T


def orthogonal_forward_torch(X, base):
    """orthogonal_oracle.forward restated in torch so that autograd differentiates it (the integer diagonal sign is not
    differentiated).  X (K,D), base (D,D) float64 tensors."""
    import torch
    K, D = X.shape
    eye = torch.eye(D, K, dtype=X.dtype)
    V = torch.tril(X.T, -1) + eye
    G = V.T @ V
    M = torch.triu(G, 1) + torch.diag(torch.diagonal(G) / 2.0)
    W = torch.linalg.solve(M, V[:K].T)
    s = torch.trunc(torch.diagonal(X[:, :K])).detach()
    return (base @ ((eye - V @ W) * s[None, :])).T


def stage(X, Psi, means, noise, kind, gS, gloss):
    """The whole chain for a given upstream gradient gS (symmetric per class, (C,m,m) with m = K or K + 1) and incoming
    loss gradient gloss.  kind: "sphere", "identity", or the (D,D) base matrix of an orthogonal parametrization.

        F = X / ||X||_row | X | orthogonal_oracle.forward(X, base);  S = F Psi F^T + noise I;
        out = S, or oracle.reference_path.embed_gaussian(means F^T, S);  L = gloss * sum(gS * out)

    Returns a dict:
        out          Val of S | E
        dX_autograd  dL/dX from torch autograd on the plain float64 expression above
        dX           Val of dL/dX from the hand-written backward formulas of this module (the two check each other:
                     tests/test_projection_oracle.py), with the composed magnitude and term count
        F, norms     float64 filters and row norms (norms None unless kind == "sphere")
    """
    import torch
    from oracle import reference_path
    import orthogonal_oracle

    X = np.asarray(X, dtype=F64)
    Psi = np.asarray(Psi, dtype=F64)
    gS = np.asarray(gS, dtype=F64)
    K, D = X.shape
    C = Psi.shape[0]
    base = None if isinstance(kind, str) else np.asarray(kind, dtype=F64)

    # -- autograd on the plain expression
    Xt = torch.tensor(X, requires_grad=True)
    Pt = torch.tensor(Psi)
    if base is not None:
        Ft = orthogonal_forward_torch(Xt, torch.tensor(base))
    elif kind == "sphere":
        Ft = Xt / torch.linalg.norm(Xt, dim=1, keepdim=True)
    elif kind == "identity":
        Ft = Xt
    else:
        raise ValueError(kind)
    St = Ft.unsqueeze(0) @ Pt @ Ft.T.unsqueeze(0) + noise * torch.eye(K, dtype=torch.float64)
    out_t = St if means is None else reference_path.embed_gaussian(torch.tensor(np.asarray(means, dtype=F64)) @ Ft.T, St)
    (float(gloss) * (torch.tensor(gS) * out_t).sum()).backward()
    dX_autograd = Xt.grad.numpy()

    # -- the hand-written chain, with magnitudes and term counts
    norms = None
    if base is not None:
        F = orthogonal_oracle.forward(X, base)
        V, Minv, W = _orthogonal_parts(X)
        Wm = np.abs(Minv) @ np.abs(V[:K].T)
        Fm = (np.abs(base) @ (np.eye(D, K) + np.abs(V) @ Wm)).T
        n_F = 2 * D + 2 * K          # V^T V and base P over D, the two K x K solves / products over K
    elif kind == "sphere":
        Fv, nv = sphere_forward(X)
        F, Fm, n_F, norms = Fv.value, Fv.mag, Fv.n, nv.value
    else:
        F, Fm, n_F = X, np.abs(X), 0
    T = project(Psi, F)
    Tm = np.matmul(np.abs(Psi), Fm.T)
    n_T = D + n_F
    m = mm = None
    if means is not None:
        mu = np.asarray(means, dtype=F64)
        m, mm, n_m = mu @ F.T, np.abs(mu) @ Fm.T, D + n_F
    fs = feature_scatters(F, T.value, noise, m)
    Sm = np.matmul(Fm[None], Tm) + abs(noise) * np.eye(K)
    n_out = n_F + n_T + D + 2        # F twice (once inside T), the two products, noise and m m^T
    if m is not None:
        Em = fs.mag.copy()
        Em[:, :K, :K] = Sm + mm[:, :, None] * mm[:, None, :]
        Em[:, :K, K] = mm
        Em[:, K, :K] = mm
        Sm = Em
        n_out += 2 * n_m
    out = Val(fs.value, Sm, n_out)

    P = backward_partials(gS, T.value, 1)
    Ga = np.abs(gS[:, :K, :K])
    gF = P.value[0]
    gFm = np.matmul(Ga + Ga.transpose(0, 2, 1), Tm.transpose(0, 2, 1)).sum(0)
    n_gF = n_T + 2 * K * C
    if m is not None:
        gm = embed_backward_means(gS, m)
        gmm = (np.einsum("cab,cb->ca", Ga + Ga.transpose(0, 2, 1), mm) + np.abs(gS[:, :K, K]) + np.abs(gS[:, K, :K]))
        gF = gF + gm.value.T @ mu
        gFm = gFm + gmm.T @ np.abs(mu)
        n_gF += n_m + gm.n + C
    if base is not None:
        dX = orthogonal_oracle.backward(X, base, gloss * gF)
        gPm = np.abs(base).T @ (abs(gloss) * gFm).T
        Zm = np.abs(Minv).T @ (np.abs(V).T @ gPm)
        gMm = Zm @ Wm.T
        Nm = np.triu(gMm, 1)
        gVm = gPm @ Wm.T + np.abs(V) @ (Nm + Nm.T + np.diag(np.diag(gMm)))
        gVm[:K] += Zm.T
        dXm = np.tril(gVm, -1).T
        n_dX = n_gF + 2 + 3 * D + 4 * K       # class reduction and gloss; base^T gF, V^T gP, V gM over D, the K x K steps over K
    elif kind == "sphere":
        sb = sphere_backward(X, norms, gF[None], None, gloss)
        dX = sb.value
        dXm = abs(gloss) * (gFm + Fm * (Fm * gFm).sum(1, keepdims=True)) / norms[:, None]
        n_dX = n_gF + sb.n + 2 * n_F          # F twice more in the sphere backward
    else:
        dX, dXm, n_dX = gloss * gF, abs(gloss) * gFm, n_gF + 2
    return {"out": out, "dX_autograd": dX_autograd, "dX": Val(dX, dXm, n_dX), "F": F, "norms": norms}


# ---- seeded input families (shared by the CPU and the GPU test file) ------------------------------------------------


def rng_for(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def symmetric_scatters(rng, C, D, dtype):
    """Psi = A + A^T of a rounded A: exactly symmetric in `dtype` (the sum of two values of the dtype is rounded the
    same way on both sides of the diagonal)."""
    A = rounded(rng.standard_normal((C, D, D)) / np.sqrt(D), dtype)
    return rounded(A + A.transpose(0, 2, 1), dtype)


def spd_scatters(rng, C, D, dtype):
    """Well-conditioned covariance-like scatters for the chain (its orthogonal and sphere maps need nothing of Psi, but
    the magnitudes stay comparable to the values): A A^T / R + 0.05 I, symmetrised exactly after rounding."""
    R = D + 2
    A = rng.standard_normal((C, D, R))
    P = rounded(np.matmul(A, A.transpose(0, 2, 1)) / R + 0.05 * np.eye(D), dtype)
    lower = np.tril(P)
    return lower + np.tril(P, -1).transpose(0, 2, 1)


def normal(rng, shape, dtype, scale=1.0):
    return rounded(scale * rng.standard_normal(shape), dtype)


def symmetric_gradient(rng, C, m, dtype):
    g = rounded(rng.standard_normal((C, m, m)), dtype)
    lower = np.tril(g)
    return lower + np.tril(g, -1).transpose(0, 2, 1)


# One builder per kernel under test: the inputs a case of tests/test_gpu_projection_kernels.py hands to the kernel, already
# rounded to the dtype under test (float64 arrays holding values of that dtype).


def case_project(C, D, K, dtype):
    rng = rng_for(1, C, D, K)
    return {"Psi": symmetric_scatters(rng, C, D, dtype), "F": normal(rng, (K, D), dtype)}


def case_forward(C, D, K, dtype):
    rng = rng_for(2, C, D, K)
    return {"F": normal(rng, (K, D), dtype), "T": normal(rng, (C, D, K), dtype), "m": normal(rng, (C, K), dtype, 0.5)}


def case_backward(C, D, K, ldg, symmetric, dtype):
    rng = rng_for(3, C, D, K, ldg)
    G = symmetric_gradient(rng, C, ldg, dtype) if symmetric else normal(rng, (C, ldg, ldg), dtype)
    return {"G": G, "T": normal(rng, (C, D, K), dtype)}


def case_sphere(K, D, n_groups, dtype):
    rng = rng_for(4, K, D, n_groups)
    X = normal(rng, (K, D), dtype)
    norms = rounded(np.sqrt((X * X).sum(1)), dtype)
    return {"X": X, "norms": norms, "partials": normal(rng, (n_groups, K, D), dtype) if n_groups else None,
            "extra": normal(rng, (K, D), dtype), "gloss": float(rounded(-1.75 + 0.01 * K, dtype))}


def case_embed(C, K, dtype):
    rng = rng_for(5, C, K)
    return {"gE": normal(rng, (C, K + 1, K + 1), dtype), "m": normal(rng, (C, K), dtype, 0.5)}


CHAIN_KINDS = ("sphere", "identity", "orthogonal")


def case_chain(K, D, C, kind, with_means, dtype):
    """X, Psi, means, gS, gloss of a chain case; kind "orthogonal": X and base from orthogonal_oracle.make_case."""
    import orthogonal_oracle
    rng = rng_for(6, K, D, C, CHAIN_KINDS.index(kind), int(with_means))
    base = None
    if kind == "orthogonal":
        X, base, _ = orthogonal_oracle.make_case(K, D, "mixed", seed=3)
        X, base = rounded(X, dtype), rounded(base, dtype)
    else:
        X = normal(rng, (K, D), dtype)
    m = K + 1 if with_means else K
    return {"X": X, "base": base, "Psi": spd_scatters(rng, C, D, dtype),
            "means": normal(rng, (C, D), dtype, 0.1) if with_means else None,
            "gS": symmetric_gradient(rng, C, m, dtype), "gloss": 3.0, "noise": float(rounded(0.01, dtype))}
