"""ms per loss+gradient closure INSIDE fit(), after the graph capture, with uniform pair weights (pair_weights=None) and with
a (C,C) weight matrix (fit(pair_weights=W)):

    python tools/time_weighted_closure.py [--out profiles/weighted_closure_time.txt] [--label NAME] [--quick]

On a tree without fit(pair_weights=...) only the uniform column is reported: run it there for the baseline (column (a) of
the table in README.md; (b) and (c) are the two columns of a run on this tree).  Sizes (C, D, K): c3 (1000, 784, 16) and
(300, 784, 32), float32.  Operators: affine_invariant and log_euclidean (SecondMomentsSQFA), fisher_rao_lower_bound,
bhattacharyya and mahalanobis (SQFA).  Statistics: 0.7 x a common Wishart + 0.3 x a per-class Wishart, means 0.1 N(0, I),
feature_noise 0.01.  Weights: symmetric, uniform in [0.25, 1.75], about 20 % of the pairs exactly zero.

Timing (the method of tools/time_orthogonal_closure.py): fit(max_epochs=8, atol=0) calls the closure ~170 times; the host
clock is read at every closure entry (each closure ends with the read-back of its loss, so the host follows the device) and
a fit's figure is the MEDIAN interval between consecutive closures after the first 10 (past the eager warm-up closures and
the capture) -- the LBFGS update between two closures is inside it, the same work on every side.  One untimed fit first,
then 3 timed fits per side, the sides alternating; reported: median over the fits and [min .. max] (the run-to-run spread),
and closures per fit."""
import argparse
import inspect
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import _lbfgs, _optim, distances

DEV = "cuda:0"
SIZES = ((1000, 784, 16), (300, 784, 32))
OPERATORS = (("affine_invariant", "smsqfa"), ("fisher_rao_lower_bound", "sqfa"), ("bhattacharyya", "sqfa"),
             ("mahalanobis", "sqfa"), ("log_euclidean", "smsqfa"))
HAS_WEIGHTS = "pair_weights" in inspect.signature(_optim.fitting_loop).parameters
SIDES = ("uniform", "weighted") if HAS_WEIGHTS else ("uniform",)
SKIP = 10


def statistics(C, D, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 2 * D
    X = torch.randn(n, D, generator=g, device=DEV, dtype=torch.float32)
    common = X.T @ X / n
    cov = torch.empty(C, D, D, dtype=torch.float32, device=DEV)
    for c0 in range(0, C, 50):
        c1 = min(C, c0 + 50)
        Y = torch.randn(c1 - c0, n, D, generator=g, device=DEV, dtype=torch.float32)
        W = Y.transpose(1, 2) @ Y / n
        cov[c0:c1] = 0.7 * common + 0.3 * 0.5 * (W + W.transpose(1, 2))
    return {"means": 0.1 * torch.randn(C, D, generator=g, device=DEV, dtype=torch.float32), "covariances": cov}


def weights(C, seed=1):
    g = torch.Generator().manual_seed(seed)
    W = torch.tril((0.25 + 1.5 * torch.rand(C, C, generator=g)) * (torch.rand(C, C, generator=g) >= 0.2), -1)
    return W + W.T


class ClosureClock:
    """Wraps the closure the fitting loop hands to the optimizer: host time at every entry."""

    def __init__(self):
        self.stamps = []
        self._orig = _lbfgs.CompactLBFGS.step

    def __enter__(self):
        clock, orig = self, self._orig

        def step(opt, closure):
            def counted(*a, **k):
                clock.stamps.append(time.perf_counter())
                return closure(*a, **k)

            if hasattr(closure, "deferred"):
                def deferred():
                    clock.stamps.append(time.perf_counter())
                    return closure.deferred()

                counted.deferred = deferred
                counted.check_flags = closure.check_flags
            return orig(opt, counted)

        _lbfgs.CompactLBFGS.step = step
        return self

    def __exit__(self, *exc):
        _lbfgs.CompactLBFGS.step = self._orig
        return False


def one_fit(side, op, kind, D, K, data, W):
    torch.manual_seed(1)
    cls = sqfa_amd.model.SQFA if kind == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    model = cls(n_dim=D, n_filters=K, feature_noise=0.01, distance_fun=getattr(distances, op)).to(DEV)
    extra = {"pair_weights": W} if side == "weighted" else {}
    with ClosureClock() as clock:
        loss, _ = model.fit(data_statistics=data, max_epochs=8, atol=0.0, show_progress=False, return_loss=True, **extra)
        torch.cuda.synchronize()
        clock.stamps.append(time.perf_counter())
    assert torch.isfinite(loss).all()
    gaps = np.diff(np.array(clock.stamps))[SKIP:]
    return 1e3 * float(np.median(gaps)), len(clock.stamps) - 1


def fmt(t):
    return "      -      " if t is None else f"{np.median(t):7.3f} [{min(t):.3f} .. {max(t):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--quick", action="store_true", help="a small size only (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_weighted_closure.py measures on the GPU only")
    lines = [f"# tools/time_weighted_closure.py -- {args.label} -- fit(pair_weights=...) {'present' if HAS_WEIGHTS else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             "# ms per closure inside fit(), float32: median [min .. max] over 3 fits; closures per fit (of the last side)",
             f"# {'C':>4} {'D':>4} {'K':>3} {'operator':<24} {'uniform':<26} {'weighted':<26} weighted/uniform closures"]
    print("\n".join(lines), flush=True)
    for C, D, K in (((60, 64, 8),) if args.quick else SIZES):
        stats = statistics(C, D)
        scatters = stats["covariances"] + stats["means"][:, :, None] * stats["means"][:, None, :]
        W = weights(C)
        for op, kind in OPERATORS:
            data = stats if kind == "sqfa" else scatters
            times = {s: [] for s in SIDES}
            for s in SIDES:
                one_fit(s, op, kind, D, K, data, W)     # untimed: libraries, allocator, symmetry check of the statistics
            for _ in range(3):
                for s in SIDES:
                    ms, calls = one_fit(s, op, kind, D, K, data, W)
                    times[s].append(ms)
            ratio = f"{np.median(times['weighted']) / np.median(times['uniform']):6.3f}" if HAS_WEIGHTS else "   -  "
            line = (f"  {C:>4} {D:>4} {K:>3} {op:<24} {fmt(times['uniform']):<26} {fmt(times.get('weighted')):<26} "
                    f"{ratio:<16} {calls}")
            print(line, flush=True)
            lines.append(line)
        del stats, scatters
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
