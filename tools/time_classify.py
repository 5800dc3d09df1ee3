"""Times sqfa_amd.classify's native Gaussian class scores against a torch expression on the same GPU and scikit-learn's
QuadraticDiscriminantAnalysis on the CPU, and writes profiles/classify_time.txt.

    python tools/time_classify.py                 the table (median of 7 runs, device events, variants alternating)
    python tools/time_classify.py --trace-run     three native predict calls at (60000, 1000, 16) float32 and nothing else:
                                                  the run to put under `rocprofv3 --kernel-trace --stats -- python ...`

The torch expression is written here (not the package's fallback): batched cholesky and solve_triangular (against the
identity) once, then per chunk of classes the whitened differences by bmm, squares, offset, and a running (best, index)
over the chunks; the chunk keeps the (classes, N, K) temporary near 256 MB.
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sqfa_amd import classify  # noqa: E402

DEV = "cuda:0"
SHAPES = [(60000, 1000, 16, torch.float32), (60000, 1000, 16, torch.float64), (10000, 10, 16, torch.float32),
          (50000, 100, 16, torch.float32), (60000, 300, 32, torch.float32), (20000, 100, 64, torch.float32)]
RUNS = 7
PEAK_F32_MFMA = 157.3e12


def problem(N, C, K, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = torch.randn(C, K, K + 3, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2) / (K + 3) + 0.05 * torch.eye(K, dtype=torch.float64)
    mu = torch.randn(C, K, generator=g, dtype=torch.float64)
    y = torch.arange(N) % C
    Z = mu[y] + torch.einsum("nij,nj->ni", torch.linalg.cholesky(cov)[y], torch.randn(N, K, generator=g, dtype=torch.float64))
    return Z.to(DEV, dtype), y.to(DEV), mu.to(DEV, dtype), cov.to(DEV, dtype)


class TorchQDA:
    def __init__(self, mu, cov, budget=1 << 28):
        self.mu, self.L = mu, torch.linalg.cholesky(cov)
        C, K = mu.shape
        # solve_triangular against the identity, once: with the samples as right-hand sides hipBLAS's batched trsm fails
        # to allocate its workspace at N = 60 000 (HIPBLAS_STATUS_ALLOC_FAILED), so the solve per chunk is a bmm with L^-1
        self.W = torch.linalg.solve_triangular(self.L, torch.eye(K, dtype=cov.dtype, device=cov.device).expand_as(self.L), upper=False)
        self.offset = -torch.log(torch.diagonal(self.L, dim1=-2, dim2=-1)).sum(-1) - 0.5 * K * math.log(2 * math.pi) - math.log(C)
        self.budget = budget

    def predict(self, Z):
        N, K = Z.shape
        C = self.mu.shape[0]
        step = max(1, min(C, self.budget // (N * K * Z.element_size())))
        best = idx = None
        for c0 in range(0, C, step):
            diff = (Z[None] - self.mu[c0:c0 + step, None]).transpose(-1, -2)
            y = torch.bmm(self.W[c0:c0 + step], diff)
            s = -0.5 * (y * y).sum(1) + self.offset[c0:c0 + step, None]      # (c, N)
            b, i = s.max(0)
            i = i + c0
            if best is None:
                best, idx = b, i
            else:
                take = b > best
                best, idx = torch.where(take, b, best), torch.where(take, i, idx)
        return idx


def timed(fn):
    """(ms by device events, peak bytes above what was allocated before) of one call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return start.elapsed_time(stop), peak


def fmt(ts):
    return f"{statistics.median(ts):9.3f} [{min(ts):.3f} .. {max(ts):.3f}]"


def table(out):
    try:
        from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis
    except ImportError:
        QuadraticDiscriminantAnalysis = None
    lines = [f"# tools/time_classify.py -- {torch.cuda.get_device_name(0)} -- torch {torch.__version__}",
             f"# ms per call (device events): median [min .. max] over {RUNS} runs, variants alternating inside every run;",
             "# peak = bytes allocated above the inputs during the call.  torch = the chunked expression of this tool"
             " (cholesky + solve_triangular once, then bmm + running argmax per chunk of classes)",
             "# sklearn = QuadraticDiscriminantAnalysis.predict on the CPUs of the same machine, wall clock, one run"
             + ("" if QuadraticDiscriminantAnalysis is not None else " -- scikit-learn is not importable on this machine: column absent")]
    for N, C, K, dtype in SHAPES:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        assert clf._factors is not None
        ref = TorchQDA(mu, cov)
        variants = {"native predict": lambda: clf.predict(Z), "native scores": lambda: clf.scores(Z),
                    "native log_evidence": lambda: clf.log_evidence(Z), "torch predict": lambda: ref.predict(Z)}
        agree = float((clf.predict(Z) == ref.predict(Z)).double().mean())
        for fn in variants.values():   # warm
            fn()
        ms = {k: [] for k in variants}
        peak = {k: 0 for k in variants}
        for _ in range(RUNS):
            for k, fn in variants.items():
                t, p = timed(fn)
                ms[k].append(t)
                peak[k] = max(peak[k], p)
        start = time.perf_counter()
        classify.GaussianClassifier(mu, cov)
        torch.cuda.synchronize()
        factor_ms = 1e3 * (time.perf_counter() - start)
        lines.append(f"N={N} C={C} K={K} {str(dtype).split('.')[-1]}: native and torch predictions agree on {agree:.4%}; "
                     f"classifier construction (factor pass + one read) {factor_ms:.3f} ms wall")
        flops = 2.0 * N * C * K * K
        for k in variants:
            extra = ""
            if k == "native predict":
                med = statistics.median(ms[k]) * 1e-3
                extra = f"   {flops / med / 1e12:6.1f} TF = {flops / med / PEAK_F32_MFMA:.1%} of 157.3 TF (2 N C K^2, whole call)"
            lines.append(f"    {k:20s} {fmt(ms[k])} ms   peak {peak[k] / 1e6:10.2f} MB{extra}")
        speed = statistics.median(ms["torch predict"]) / statistics.median(ms["native predict"])
        lines.append(f"    torch / native predict: {speed:.1f} x in time, {peak['torch predict'] / max(peak['native predict'], 1):.0f} x in peak memory")
        if QuadraticDiscriminantAnalysis is not None:
            Zc, yc = Z.double().cpu().numpy(), y.cpu().numpy()
            qda = QuadraticDiscriminantAnalysis().fit(Zc, yc)
            start = time.perf_counter()
            qda.predict(Zc)
            lines.append(f"    sklearn predict      {1e3 * (time.perf_counter() - start):9.1f} ms wall (own fit on the same samples, float64)")
        del Z, y, mu, cov, clf, ref, variants
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


def trace_run():
    N, C, K, dtype = SHAPES[0]
    Z, _, mu, cov = problem(N, C, K, dtype)
    clf = classify.GaussianClassifier(mu, cov)
    for _ in range(3):
        clf.predict(Z)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_time.txt"))
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
    else:
        table(args.out)
