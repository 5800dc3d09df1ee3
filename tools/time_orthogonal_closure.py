"""ms per loss+gradient closure INSIDE fit() of SecondMomentsSQFA (affine-invariant distance, the single-node graph closure)
under the filter constraints:

  sphere       constraint="sphere", for scale
  torch        constraint="orthogonal" with constraints.NATIVE_ORTHOGONAL = False: torch's _Orthogonal.forward (tril, column
               norms, householder_product, sign, base @ Q) and its autograd backward in front of the chain closure
  native       constraint="orthogonal" with the switch on: sqfa_orthogonal_forward / _backward inside the one-node closure

    python tools/time_orthogonal_closure.py [--out profiles/orthogonal_closure_time.txt] [--label NAME] [--quick]

On a tree without the native map (no constraints.NATIVE_ORTHOGONAL) the sphere and torch columns are reported: run it there
for the baseline.  Sizes (C, D, K): c3 (1000, 784, 16), c5 (100, 3072, 16), (30, 784, 16); float32 and float64.  Statistics:
0.7 x a common Wishart + 0.3 x a per-class Wishart, feature_noise 0.01.

Timing: fit(max_epochs=8, atol=0) calls the closure ~170 times; the host clock is read at every closure entry (each closure
ends with the read-back of its loss, so the host follows the device) and a fit's figure is the MEDIAN interval between
consecutive closures after the first 10 (past the eager warm-up closures and the capture) -- the LBFGS update between two
closures is inside it, the same work on every side.  One untimed fit first, then 3 timed fits per side, the sides
alternating; reported: median over the fits and [min .. max] (the run-to-run spread), and closures per fit."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import _lbfgs, constraints

DEV = "cuda:0"
SIDES = ("sphere", "torch", "native")
SIZES = tuple((C, D, K, dt) for C, D, K in ((1000, 784, 16), (100, 3072, 16), (30, 784, 16)) for dt in (torch.float32, torch.float64))
HAS_NATIVE = hasattr(constraints, "NATIVE_ORTHOGONAL")
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


def one_fit(side, C, D, K, dtype, stats):
    if HAS_NATIVE:
        constraints.NATIVE_ORTHOGONAL = side == "native"
    torch.manual_seed(1)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=0.01,
                                             constraint="sphere" if side == "sphere" else "orthogonal")
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
    ap.add_argument("--quick", action="store_true", help="the smallest size only (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_orthogonal_closure.py measures on the GPU only")
    sides = SIDES if HAS_NATIVE else SIDES[:2]
    lines = [f"# tools/time_orthogonal_closure.py -- {args.label} -- native orthogonal map {'present' if HAS_NATIVE else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             "# ms per closure inside fit(): median [min .. max] over 3 fits; closures per fit (of the last side)",
             f"# {'C':>4} {'D':>4} {'K':>3} dtype   {'sphere':<26} {'orthogonal, torch map':<26} {'orthogonal, native map':<26} closures"]
    print("\n".join(lines), flush=True)
    for C, D, K, dtype in (SIZES[4:] if args.quick else SIZES):
        stats = statistics(C, D, dtype)
        times = {s: [] for s in sides}
        for s in sides:
            one_fit(s, C, D, K, dtype, stats)     # untimed: libraries, allocator, symmetry check of the statistics
        for _ in range(3):
            for s in sides:
                ms, calls = one_fit(s, C, D, K, dtype, stats)
                times[s].append(ms)
        line = (f"  {C:>4} {D:>4} {K:>3} {str(dtype)[6:]:<7} {fmt(times['sphere']):<26} {fmt(times['torch']):<26} "
                f"{fmt(times.get('native')):<26} {calls}")
        print(line, flush=True)
        lines.append(line)
        del stats
        torch.cuda.empty_cache()
    if HAS_NATIVE:
        constraints.NATIVE_ORTHOGONAL = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
