#!/usr/bin/env python3
"""Regenerate g9_log_euclidean_closure.npz: the closure of SecondMomentsSQFA with log_euclidean / log_euclidean_sq as
distance_fun, as the *reference* package computes it on the CPU.

    SQFA_REFERENCE_SRC=<reference checkout>/src PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_log_euclidean_closure.py

The reference is needed at generation time only; the file written holds DATA: inputs made by the generator below
and what the reference computes for them, in float64 ("_f64") and float32 ("_f32": the reference's own deviation is the
yardstick of the float32 tolerances).

Per case (C, D, K, noise) -- K = 1, 3 (not a multiple of 4, fewer entries than a wave), 4, 16, 17, 33, 64 (one per lane
geometry of the pair pass, and the size limit):
  {case}_scatters (C,D,D), {case}_raw (K,D)     class second moments, raw (unnormalised) filters
  {case}_fscatters (C,K,K)                       feature scatters at those filters (sphere, + noise I)
(symmetric matrices are stored as their lower triangles, (C, n(n+1)/2) in np.tril_indices order: pack_sym / unpack_sym)
and per operator:
  {case}_{op}_D_{tag} (C,C)                      get_class_distances(regularized=True)
  {case}_{op}_loss_{tag}, _grad_{tag} (K,D)      closure loss (-mean over i > j) and its gradient wrt the raw filters
  {case}_{op}_gS_{tag} (C,K,K)                   gradient of the same loss wrt the feature scatters
  {case}_{op}_fit_f64 (5)                        loss per epoch of a 5-epoch float64 fit from the raw filters
Every stored output is finite (asserted); the smallest off-diagonal log_euclidean distance is printed (the square-root kind
is not at its eps floor)."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF_SRC = os.environ.get("SQFA_REFERENCE_SRC")
if not REF_SRC:
    sys.exit("set SQFA_REFERENCE_SRC to the src directory of a checkout of the reference package")
sys.path.insert(0, REF_SRC)

import torch  # noqa: E402

import sqfa  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)

OPS = ("log_euclidean", "log_euclidean_sq")
CASES = ((5, 10, 1, 1e-2), (7, 12, 3, 1e-2), (12, 20, 4, 1e-3), (10, 24, 16, 1e-2), (9, 40, 17, 1e-2), (6, 48, 33, 1e-2),
         (4, 72, 64, 1e-2))


def case_key(C, D, K):
    return f"C{C}_D{D}_K{K}"


def pack_sym(M):
    """(C,n,n) symmetric -> (C, n(n+1)/2): the lower triangles, np.tril_indices order (halves the file)."""
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    r, c = np.tril_indices(M.shape[-1])
    return np.ascontiguousarray(M[:, r, c])


def unpack_sym(P):
    """Inverse of pack_sym."""
    n = int(round((np.sqrt(8 * P.shape[-1] + 1) - 1) / 2))
    r, c = np.tril_indices(n)
    M = np.zeros((P.shape[0], n, n), dtype=P.dtype)
    M[:, r, c] = P
    M[:, c, r] = P
    return M


def make_inputs(rng, C, D, K):
    """0.7 x a common Wishart + 0.3 x a per-class Wishart of 4 D samples (as g8), raw filters randn."""
    X = rng.standard_normal((4 * D, D))
    common = X.T @ X / (4 * D)
    scatters = np.empty((C, D, D))
    for c in range(C):
        Y = rng.standard_normal((4 * D, D))
        scatters[c] = 0.7 * common + 0.3 * (Y.T @ Y / (4 * D))
        scatters[c] = 0.5 * (scatters[c] + scatters[c].T)
    raw = rng.standard_normal((K, D))
    return scatters, raw


def tril_loss(Dm):
    n = Dm.shape[0]
    rows, cols = torch.tril_indices(n, n, offset=-1)
    return -Dm[rows, cols].mean()


def build_model(op, D, K, noise, raw, dt):
    torch.set_default_dtype(dt)
    model = sqfa.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=noise, distance_fun=getattr(sqfa.distances, op),
                                         constraint="sphere")
    if dt == torch.float64:
        model = model.double()
    with torch.no_grad():
        model.parametrizations.filters.original.copy_(torch.tensor(raw, dtype=dt))
    return model


def main():
    rng = np.random.default_rng(909)
    out = {"cases": np.array([c[:3] for c in CASES]), "noise": np.array([c[3] for c in CASES]), "ops": np.array(OPS)}
    for C, D, K, noise in CASES:
        key = case_key(C, D, K)
        scatters, raw = make_inputs(rng, C, D, K)
        out[f"{key}_scatters"], out[f"{key}_raw"] = pack_sym(scatters), raw
        for op in OPS:
            for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                model = build_model(op, D, K, noise, raw, dt)
                stats = torch.tensor(scatters, dtype=dt)
                Dm = model.get_class_distances(stats, regularized=True).reshape(C, C)
                loss = tril_loss(Dm)
                model.zero_grad()
                loss.backward()
                grad = model.parametrizations.filters.original.grad
                # the same loss as a function of the feature scatters
                with torch.no_grad():
                    F = model.filters.detach()
                    fs = F @ stats @ F.T + model.noise_mat[None]
                fsg = fs.clone().requires_grad_(True)
                (gS,) = torch.autograd.grad(tril_loss(getattr(sqfa.distances, op)(fsg, fsg).reshape(C, C)), [fsg])
                gS = 0.5 * (gS + gS.transpose(1, 2))   # the gradient wrt a symmetric matrix, as a full symmetric matrix
                if tag == "f64" and op == "log_euclidean":
                    fs_np = fs.numpy()
                    fs_np = 0.5 * (fs_np + np.swapaxes(fs_np, 1, 2))   # symmetric to the last bit (F S F^T is, to rounding)
                    out[f"{key}_fscatters"] = pack_sym(fs_np)
                    off = ~np.eye(C, dtype=bool)
                    print(f"{key}: min off-diagonal log_euclidean = {float(Dm.detach().numpy()[off].min()):.4f}")
                for name, val in (("D", Dm), ("loss", loss), ("grad", grad), ("gS", gS)):
                    val = val.detach().numpy()
                    assert np.isfinite(val).all(), (key, op, tag, name)
                    out[f"{key}_{op}_{name}_{tag}"] = pack_sym(val) if name == "gS" else val
            model = build_model(op, D, K, noise, raw, torch.float64)
            fit_loss, _ = model.fit(data_statistics=torch.tensor(scatters), max_epochs=5, show_progress=False, return_loss=True)
            fit_loss = fit_loss.double().numpy()
            assert fit_loss.shape == (5,) and np.isfinite(fit_loss).all(), (key, op, fit_loss)
            out[f"{key}_{op}_fit_f64"] = fit_loss
            print(f"  {op}: loss {float(out[f'{key}_{op}_loss_f64']):.6f}, fit {fit_loss}")
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, "g9_log_euclidean_closure.npz"), **out)


if __name__ == "__main__":
    main()
