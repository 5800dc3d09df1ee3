"""Bures-Wasserstein pair stage (sqfa_bw_pairwise: K0 + BW prologue + K0b + K1 + K2 + sandwich, closure loss + gradient, self
mode) against the affine-invariant pair stage (sqfa_airm_pairwise) on the same classes, Jacobi sweeps per pair of both
metrics (sweep_counter), and the tutorial's torch expression (loss + autograd gradient) at C = 300, m = 16.

    python tools/time_bw_pairs.py            cases (C, m, dtype): (1000, 16, f32) (1000, 16, f64) (300, 64, f32) (100, 128, f32)

Classes: random SPD matrices with a common dominant covariance (Sigma_c = M D_c M^T + 0.05 I, D_c diagonal in [0.5, 2]).
Stage timings: median of 5 rounds of 10 eager calls each between torch.cuda events (ms per call)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sqfa_amd import _native, linalg

DEV = "cuda:0"


def classes(C, m, dtype, seed=0):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((m, m)) / np.sqrt(m)
    d = rng.uniform(0.5, 2.0, (C, m))
    S = np.einsum("ij,cj,kj->cik", M, d, M) + 0.05 * np.eye(m)
    return torch.tensor(S, dtype=dtype, device=DEV)


def stage(S, metric, sweeps=None):
    C = S.shape[0]
    P = C * (C - 1) // 2
    kw = {"metric": "bw"} if metric == "bw" else {}
    with _native.policies(sweep_counter=sweeps):
        o = _native.hip_pair_backend(S, None, scale=1.0, eps=1e-6, sqrt_mode=True, weights=None, uniform_weight=-1.0 / P,
                                     shard=(0, 1), want_loss=True, want_grad=True, want_dist=False, want_eig=False, **kw)
    return o


def ms_per_call(fn, reps=10, rounds=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def sweeps_per_pair(S, metric):
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    stage(S, metric, cnt)
    torch.cuda.synchronize()
    s, rounds = cnt.tolist()
    return s / max(rounds, 1)


def tutorial_loss(S):
    tr = torch.einsum("ijj->i", S)
    Cm = linalg.conjugate_matrix(S, linalg.spd_sqrt(S))
    D = torch.sqrt(torch.abs(tr[None, :] + tr[:, None] - 2 * torch.sqrt(torch.linalg.eigvalsh(Cm)).sum(-1)) + 1e-6)
    C = S.shape[0]
    return -torch.tril(D, -1).sum() / (C * (C - 1) // 2)


def main():
    print("C     m    dtype    airm_ms   bw_ms   bw/airm   sweeps_airm  sweeps_bw   (sweeps: per wave round = per pair row of"
          " lanes; LDS path: per pair)")
    for C, m, dt in ((1000, 16, torch.float32), (1000, 16, torch.float64), (300, 64, torch.float32),
                     (100, 128, torch.float32)):
        S = classes(C, m, dt)
        t_a = ms_per_call(lambda: stage(S, "airm"))
        t_b = ms_per_call(lambda: stage(S, "bw"))
        print(f"{C:<5} {m:<4} {str(dt)[6:]:<8} {t_a:8.3f} {t_b:8.3f} {t_b / t_a:8.2f}   {sweeps_per_pair(S, 'airm'):10.2f}"
              f"  {sweeps_per_pair(S, 'bw'):9.2f}", flush=True)
    S = classes(300, 16, torch.float32)

    def torch_path():
        X = S.detach().clone().requires_grad_(True)
        tutorial_loss(X).backward()

    t_t = ms_per_call(torch_path, reps=3, rounds=3)
    t_b = ms_per_call(lambda: stage(S, "bw"))
    print(f"C=300 m=16 float32 loss+grad: tutorial torch expression {t_t:.3f} ms, native BW {t_b:.3f} ms, "
          f"speed-up {t_t / t_b:.1f}x", flush=True)


if __name__ == "__main__":
    main()
