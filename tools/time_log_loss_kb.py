"""Times the native Gaussian class scores and log-loss over every KB = ceil(K / 16), both dtypes, with and without means:
tools/time_classify.py and tools/time_log_loss.py take K > 16 only at float32 and always with means.

    python tools/time_log_loss_kb.py               ms (device events), median [min .. max] of 9 runs, variants alternating:
                                                   log_evidence (gauss_scores_kernel) and loss plus all gradients
                                                   (gl_sample_kernel, gl_class_kernel and the small passes)
    python tools/time_log_loss_kb.py --trace-run   six loss-plus-gradient calls at K = 48 and 64 with means, both dtypes, and
                                                   nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- python ...`

SQFA_HIP_LIBRARY selects the library; an A/B is two runs per library, each a process of its own.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sqfa_amd import classify  # noqa: E402

DEV = "cuda:0"
N, C = 40000, 200
RUNS = 9


def problem(K, dtype, means):
    g = torch.Generator().manual_seed(N + C + K)
    A = torch.randn(C, K, K + 3, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2) / (K + 3) + 0.05 * torch.eye(K, dtype=torch.float64)
    mu = torch.randn(C, K, generator=g, dtype=torch.float64) if means else None
    y = torch.arange(N) % C
    Z = torch.einsum("nij,nj->ni", torch.linalg.cholesky(cov)[y], torch.randn(N, K, generator=g, dtype=torch.float64))
    if means:
        Z = Z + mu[y]
    to = lambda t: None if t is None else t.to(DEV, dtype)
    return to(Z), y.to(DEV), to(mu), to(cov)


def loss_and_gradients(Z, y, mu, cov):
    leaves = [t.clone().requires_grad_() if t is not None else None for t in (Z, mu, cov)]

    def call():
        for t in leaves:
            if t is not None:
                t.grad = None
        classify.gaussian_log_loss(leaves[0], y, leaves[1], leaves[2]).backward()
    return call


def timed(fn):
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def table():
    for dtype in (torch.float32, torch.float64):
        for K in (16, 32, 48, 64):
            for means in (True, False):
                Z, y, mu, cov = problem(K, dtype, means)
                clf = classify.GaussianClassifier(mu, cov)
                variants = {"log_evidence": lambda: clf.log_evidence(Z), "loss+gradients": loss_and_gradients(Z, y, mu, cov)}
                ms = {k: [] for k in variants}
                for run in range(RUNS + 1):   # the first run warms
                    for k, fn in variants.items():
                        t = timed(fn)
                        if run:
                            ms[k].append(t)
                for k in variants:
                    print(f"N={N} C={C} K={K} {str(dtype)[6:]} {'means' if means else 'zeromean'} {k:16s} "
                          f"{statistics.median(ms[k]):9.3f} [{min(ms[k]):.3f} .. {max(ms[k]):.3f}]", flush=True)


def trace_run():
    for dtype in (torch.float32, torch.float64):
        for K in (48, 64):
            call = loss_and_gradients(*problem(K, dtype, True))
            for _ in range(6):
                call()
            torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    if ap.parse_args().trace_run:
        trace_run()
    else:
        table()
