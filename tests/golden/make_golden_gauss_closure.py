#!/usr/bin/env python3
"""Regenerate g8_gauss_closure.npz: the closure of SQFA with bhattacharyya / hellinger / mahalanobis_sq / mahalanobis as
distance_fun, as the *reference* package computes it on the CPU.

    SQFA_REFERENCE_SRC=<reference checkout>/src PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss_closure.py

The reference is needed at generation time only; the file written holds DATA: inputs made by the generator below
and what the reference computes for them, in float64 ("_f64") and float32 ("_f32": the reference's own deviation is the
yardstick of the float32 tolerances).

Per case (C, D, K, noise) -- K = 1, 3 (register kernel, K % 4 != 0), 4, 16, 17 (LDS kernel in float32), 33:
  {case}_mu (C,D), {case}_cov (C,D,D), {case}_raw (K,D)        class statistics, raw (unnormalised) filters
  {case}_fmu (C,K), {case}_fcov (C,K,K)                          feature statistics at those filters (sphere, + noise I)
and per operator:
  {case}_{op}_D_{tag} (C,C)          get_class_distances(regularized=True)
  {case}_{op}_loss_{tag}, _grad_{tag} (K,D)   closure loss (-mean over i > j) and its gradient wrt the raw filters
  {case}_{op}_gmu_{tag}, _gcov_{tag} gradient of the same loss wrt the feature statistics
  {case}_{op}_fit_f64 (5)            loss per epoch of a 5-epoch float64 fit from the raw filters
Condition on the inputs (asserted): min over pairs of exp(-Bh) >= 1e-3 at the initial filters (overlapping classes: Hellinger
is not saturated), every stored output finite."""
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

OPS = ("bhattacharyya", "hellinger", "mahalanobis_sq", "mahalanobis")
CASES = ((5, 10, 1, 1e-2), (7, 12, 3, 1e-2), (12, 20, 4, 1e-3), (10, 24, 16, 1e-2), (9, 40, 17, 1e-2), (6, 48, 33, 1e-2))


def case_key(C, D, K):
    return f"C{C}_D{D}_K{K}"


def make_inputs(rng, C, D, K):
    """Overlapping classes: 0.7 x a common covariance + 0.3 x a per-class Wishart of 4 D samples, means 0.3 randn."""
    X = rng.standard_normal((4 * D, D))
    common = X.T @ X / (4 * D)
    cov = np.empty((C, D, D))
    for c in range(C):
        Y = rng.standard_normal((4 * D, D))
        cov[c] = 0.7 * common + 0.3 * (Y.T @ Y / (4 * D))
        cov[c] = 0.5 * (cov[c] + cov[c].T)
    mu = 0.3 * rng.standard_normal((C, D))
    raw = rng.standard_normal((K, D))
    return mu, cov, raw


def tril_loss(Dm):
    n = Dm.shape[0]
    rows, cols = torch.tril_indices(n, n, offset=-1)
    return -Dm[rows, cols].mean()


def build_model(op, D, K, noise, raw, dt):
    torch.set_default_dtype(dt)
    model = sqfa.model.SQFA(n_dim=D, n_filters=K, feature_noise=noise, distance_fun=getattr(sqfa.distances, op),
                            constraint="sphere")
    if dt == torch.float64:
        model = model.double()
    with torch.no_grad():
        model.parametrizations.filters.original.copy_(torch.tensor(raw, dtype=dt))
    return model


def main():
    rng = np.random.default_rng(808)
    out = {"cases": np.array([c[:3] for c in CASES]), "noise": np.array([c[3] for c in CASES]), "ops": np.array(OPS)}
    for C, D, K, noise in CASES:
        key = case_key(C, D, K)
        mu, cov, raw = make_inputs(rng, C, D, K)
        out[f"{key}_mu"], out[f"{key}_cov"], out[f"{key}_raw"] = mu, cov, raw
        for op in OPS:
            for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                model = build_model(op, D, K, noise, raw, dt)
                stats = {"means": torch.tensor(mu, dtype=dt), "covariances": torch.tensor(cov, dtype=dt)}
                Dm = model.get_class_distances(stats, regularized=True)
                loss = tril_loss(Dm)
                model.zero_grad()
                loss.backward()
                grad = model.parametrizations.filters.original.grad
                # the same loss as a function of the feature statistics
                with torch.no_grad():
                    F = model.filters.detach()
                    fmu = stats["means"] @ F.T
                    fcov = F @ stats["covariances"] @ F.T + model.noise_mat[None]
                fs = {"means": fmu.clone().requires_grad_(True), "covariances": fcov.clone().requires_grad_(True)}
                gmu, gcov = torch.autograd.grad(tril_loss(getattr(sqfa.distances, op)(fs, fs).reshape(C, C)),
                                                [fs["means"], fs["covariances"]])
                if tag == "f64" and op == "bhattacharyya":
                    out[f"{key}_fmu"], out[f"{key}_fcov"] = fmu.numpy(), fcov.numpy()
                    off = ~np.eye(C, dtype=bool)
                    overlap = float(np.exp(-Dm.detach().numpy()[off]).min())
                    assert overlap >= 1e-3, (key, overlap)
                    print(f"{key}: min exp(-Bh) = {overlap:.3f}")
                for name, val in (("D", Dm), ("loss", loss), ("grad", grad), ("gmu", gmu), ("gcov", gcov)):
                    val = val.detach().numpy()
                    assert np.isfinite(val).all(), (key, op, tag, name)
                    out[f"{key}_{op}_{name}_{tag}"] = val
            model = build_model(op, D, K, noise, raw, torch.float64)
            stats = {"means": torch.tensor(mu), "covariances": torch.tensor(cov)}
            fit_loss, _ = model.fit(data_statistics=stats, max_epochs=5, show_progress=False, return_loss=True)
            fit_loss = fit_loss.double().numpy()
            assert fit_loss.shape == (5,) and np.isfinite(fit_loss).all(), (key, op, fit_loss)
            out[f"{key}_{op}_fit_f64"] = fit_loss
            print(f"  {op}: loss {float(out[f'{key}_{op}_loss_f64']):.6f}, fit {fit_loss}")
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, "g8_gauss_closure.npz"), **out)


if __name__ == "__main__":
    main()
