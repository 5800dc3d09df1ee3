"""ms per loss+gradient closure INSIDE fit(), Jeffreys divergence against the fused closures the package already has:

  bhattacharyya   SQFA, sqfa_gauss_pairwise_loss (O(K^3) per pair), captured in a HIP graph
  log_euclidean   SecondMomentsSQFA, sqfa_log_euclidean_pairwise_loss (per-class eigen-decomposition), captured
  jeffreys        SQFA, sqfa_jeffreys_pairwise_loss (O(K^2) per pair), captured                       [fused]
  jeffreys        the same with divergences.JEFFREYS_FUSED_CLOSURE = False: the fitting loop's generic closure (inv -> the
                  (C,C,K,K) difference tensors -> validity check on the host -> tril gather + mean -> autograd), never
                  captured                                                                            [generic]
  jeffreys_spd    SecondMomentsSQFA, the means-free kernels, captured                                 [fused]

    python tools/time_jeffreys_closure.py [--out profiles/jeffreys_closure_time.txt] [--label NAME] [--quick]

On a tree without sqfa_amd.divergences only the first two columns are reported: run it there for the baseline of the
untouched closures.  Sizes (C, D, K, dtype): (1000, 784, 16) float32 and float64, (30, 784, 16), (300, 784, 32),
(100, 784, 64) float32.  Statistics: 0.7 x a common Wishart + 0.3 x a per-class Wishart, means 0.3 randn, feature_noise 0.01.

Timing: fit(max_epochs=8, atol=0) calls the closure ~170 times; a device event is recorded on the stream at every closure
entry and a fit's figure is the MEDIAN device time between consecutive closure entries after the first 10 (past the eager
warm-up closures and the capture) -- the LBFGS update between two closures is inside it, the same work for every variant.
One untimed fit per variant first, then 7 timed fits per variant, the variants alternating; reported: median over the fits
and [min .. max] (the run-to-run spread)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import _lbfgs, distances

try:
    from sqfa_amd import divergences
except ImportError:
    divergences = None

DEV = "cuda:0"
SIZES = ((1000, 784, 16, torch.float32), (1000, 784, 16, torch.float64), (30, 784, 16, torch.float32),
         (300, 784, 32, torch.float32), (100, 784, 64, torch.float32))
SKIP = 10
FITS = 7
# name -> (model, operator module, operator, fused switch)
VARIANTS = {"bhattacharyya": ("sqfa", distances, "bhattacharyya", True),
            "log_euclidean": ("smsqfa", distances, "log_euclidean", True)}
if divergences is not None:
    VARIANTS.update({"jeffreys fused": ("sqfa", divergences, "jeffreys", True),
                     "jeffreys generic": ("sqfa", divergences, "jeffreys", False),
                     "jeffreys_spd fused": ("smsqfa", divergences, "jeffreys_spd", True)})


def statistics(C, D, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 2 * D
    X = torch.randn(n, D, generator=g, device=DEV, dtype=torch.float32)
    common = (X.T @ X / n).to(dtype)
    cov = torch.empty(C, D, D, dtype=dtype, device=DEV)
    for c0 in range(0, C, 50):
        c1 = min(C, c0 + 50)
        Y = torch.randn(c1 - c0, n, D, generator=g, device=DEV, dtype=torch.float32)
        W = (Y.transpose(1, 2) @ Y / n).to(dtype)
        cov[c0:c1] = 0.7 * common + 0.3 * 0.5 * (W + W.transpose(1, 2))
    means = (0.3 * torch.randn(C, D, generator=g, device=DEV, dtype=torch.float32)).to(dtype)
    return {"means": means, "covariances": cov}


class ClosureEvents:
    """Wraps the closure the fitting loop hands to the optimizer: a device event at every entry."""

    def __init__(self):
        self.events = []
        self._orig = _lbfgs.CompactLBFGS.step

    def mark(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.events.append(ev)

    def __enter__(self):
        clock, orig = self, self._orig

        def step(opt, closure):
            def counted(*a, **k):
                clock.mark()
                return closure(*a, **k)

            if hasattr(closure, "deferred"):
                def deferred():
                    clock.mark()
                    return closure.deferred()

                counted.deferred = deferred
                counted.check_flags = closure.check_flags
            return orig(opt, counted)

        _lbfgs.CompactLBFGS.step = step
        return self

    def __exit__(self, *exc):
        _lbfgs.CompactLBFGS.step = self._orig
        return False


def one_fit(variant, D, K, dtype, stats):
    kind, module, op, switch = VARIANTS[variant]
    if divergences is not None:
        divergences.JEFFREYS_FUSED_CLOSURE = switch
    torch.manual_seed(1)
    cls = sqfa_amd.model.SQFA if kind == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    model = cls(n_dim=D, n_filters=K, feature_noise=0.01, distance_fun=getattr(module, op))
    model = (model.double() if dtype == torch.float64 else model).to(DEV)
    data = stats if kind == "sqfa" else stats["covariances"]
    with ClosureEvents() as clock:
        loss, _ = model.fit(data_statistics=data, max_epochs=8, atol=0.0, show_progress=False, return_loss=True)
        clock.mark()
        torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    ev = clock.events
    gaps = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(len(ev) - 1)])[SKIP:]
    return float(np.median(gaps)), len(ev) - 1


def fmt(t):
    return f"{np.median(t):8.3f} [{min(t):.3f} .. {max(t):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--quick", action="store_true", help="third size only (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_jeffreys_closure.py measures on the GPU only")
    lines = [f"# tools/time_jeffreys_closure.py -- {args.label} -- sqfa_amd.divergences "
             f"{'present' if divergences is not None else 'absent'} -- {torch.cuda.get_device_name(0)}",
             f"# ms per closure inside fit() (device events): median [min .. max] over {FITS} fits; closures per fit",
             f"# {'C':>4} {'D':>4} {'K':>3} dtype   {'variant':<19} {'ms per closure':<30} closures"]
    print("\n".join(lines), flush=True)
    sizes = (SIZES[2],) if args.quick else SIZES
    for C, D, K, dtype in sizes:
        stats = statistics(C, D, dtype)
        times = {v: [] for v in VARIANTS}
        calls = {}
        for v in VARIANTS:
            one_fit(v, D, K, dtype, stats)     # untimed: libraries, allocator, symmetry check of the statistics
        for _ in range(FITS):
            for v in VARIANTS:
                ms, calls[v] = one_fit(v, D, K, dtype, stats)
                times[v].append(ms)
        for v in VARIANTS:
            line = f"  {C:>4} {D:>4} {K:>3} {str(dtype)[6:]:<7} {v:<19} {fmt(times[v]):<30} {calls[v]}"
            print(line, flush=True)
            lines.append(line)
        del stats
        torch.cuda.empty_cache()
    if divergences is not None:
        divergences.JEFFREYS_FUSED_CLOSURE = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
