"""ms per loss+gradient closure INSIDE fit() of SecondMomentsSQFA with log_euclidean / log_euclidean_sq as distance_fun:

  generic   distances.LOG_EUCLIDEAN_FUSED_CLOSURE = False: the fitting loop's generic closure (projection -> SpdFunction ->
            cdist -> validity check on the host -> tril gather + mean -> autograd backward), never captured
  fused     the switch on: projection -> _native.ClassPairLoss, captured in a HIP graph after the warm-up closures

    python tools/time_log_euclidean_closure.py [--out profiles/log_euclidean_closure_time.txt] [--label NAME] [--quick]

On a tree without the fused path (no distances.LOG_EUCLIDEAN_FUSED_CLOSURE) only the generic column is reported: run it there
for the baseline.  Sizes (C, D, K, dtype): (1000, 784, 16) float32 and float64, (30, 784, 16), (300, 784, 32), (100, 784, 64)
float32.  Statistics: 0.7 x a common Wishart + 0.3 x a per-class Wishart, feature_noise 0.01.

Timing: fit(max_epochs=8, atol=0) calls the closure ~170 times; the host clock is read at every closure entry (each closure
ends with the read-back of its loss, so the host follows the device) and a fit's figure is the MEDIAN interval between
consecutive closures after the first 10 (past the eager warm-up closures and the capture) -- the LBFGS update between two
closures is inside it, the same work on both sides.  One untimed fit first, then 5 timed fits per side, the two sides
alternating; reported: median over the fits and [min .. max] (the run-to-run spread), and closures per fit."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import _lbfgs, distances

DEV = "cuda:0"
OPS = ("log_euclidean", "log_euclidean_sq")
SIZES = ((1000, 784, 16, torch.float32), (1000, 784, 16, torch.float64), (30, 784, 16, torch.float32),
         (300, 784, 32, torch.float32), (100, 784, 64, torch.float32))
HAS_FUSED = hasattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE")
SKIP = 10


def statistics(C, D, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 2 * D
    X = torch.randn(n, D, generator=g, device=DEV, dtype=torch.float32)
    common = (X.T @ X / n).to(dtype)
    scatters = torch.empty(C, D, D, dtype=dtype, device=DEV)
    for c0 in range(0, C, 50):
        c1 = min(C, c0 + 50)
        Y = torch.randn(c1 - c0, n, D, generator=g, device=DEV, dtype=torch.float32)
        W = (Y.transpose(1, 2) @ Y / n).to(dtype)
        scatters[c0:c1] = 0.7 * common + 0.3 * 0.5 * (W + W.transpose(1, 2))
    return scatters


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


def one_fit(op, C, D, K, dtype, stats, switch):
    if HAS_FUSED:
        distances.LOG_EUCLIDEAN_FUSED_CLOSURE = switch
    torch.manual_seed(1)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=0.01, distance_fun=getattr(distances, op))
    model = (model.double() if dtype == torch.float64 else model).to(DEV)
    with ClosureClock() as clock:
        loss, _ = model.fit(data_statistics=stats, max_epochs=8, atol=0.0, show_progress=False, return_loss=True)
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
    ap.add_argument("--quick", action="store_true", help="first and third size only (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_log_euclidean_closure.py measures on the GPU only")
    lines = [f"# tools/time_log_euclidean_closure.py -- {args.label} -- fused path {'present' if HAS_FUSED else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             "# ms per closure inside fit(): median [min .. max] over 5 fits; closures per fit",
             f"# {'C':>4} {'D':>4} {'K':>3} dtype   {'operator':<17} {'generic (switch off)':<26} {'fused + graph (on)':<26} closures"]
    print("\n".join(lines), flush=True)
    sizes = (SIZES[0], SIZES[2]) if args.quick else SIZES
    for C, D, K, dtype in sizes:
        stats = statistics(C, D, dtype)
        for op in OPS:
            sides = (False, True) if HAS_FUSED else (False,)
            times = {s: [] for s in sides}
            for s in sides:
                one_fit(op, C, D, K, dtype, stats, s)     # untimed: libraries, allocator, symmetry check of the statistics
            for _ in range(5):
                for s in sides:
                    ms, calls = one_fit(op, C, D, K, dtype, stats, s)
                    times[s].append(ms)
            line = (f"  {C:>4} {D:>4} {K:>3} {str(dtype)[6:]:<7} {op:<17} {fmt(times[False]):<26} "
                    f"{fmt(times.get(True)):<26} {calls}")
            print(line, flush=True)
            lines.append(line)
        del stats
        torch.cuda.empty_cache()
    if HAS_FUSED:
        distances.LOG_EUCLIDEAN_FUSED_CLOSURE = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
