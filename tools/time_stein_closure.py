"""ms per loss+gradient closure INSIDE fit() of SecondMomentsSQFA, Stein divergence against the fused closures the package
already has:

  affine_invariant   the pair kernels (sqfa_airm_pairwise), captured in a HIP graph
  log_euclidean      sqfa_log_euclidean_pairwise_loss (per-class eigen-decomposition), captured
  stein              sqfa_stein_pairwise_loss (one Cholesky factorisation and inverse per ordered pair), captured  [fused]
  stein              the same with logdet.STEIN_FUSED_CLOSURE = False: the fitting loop's generic closure (torch.logdet of
                     the (C,C,K,K) mean matrices in chunks -> validity check on the host -> tril gather + mean -> autograd),
                     never captured                                                                              [generic]
  stein_root         sqrt(|S| + eps), captured                                                                   [fused]

    python tools/time_stein_closure.py [--out profiles/stein_closure_time.txt] [--label NAME] [--quick] [--untouched]

On a tree without sqfa_amd.logdet only the first two columns are reported: run it there (twice) for the baseline of the
untouched closures and its run-to-run spread; --untouched times the same two alone on a tree that has the module, the
like-for-like figure for them (in the five-variant run they follow the generic fits, 20 ms closures with GB of
temporaries).  Sizes, statistics and the timing method are those of
tools/time_jeffreys_closure.py (its SIZES, statistics() and ClosureEvents): a device event at every closure entry, a fit's
figure is the median device time between consecutive closure entries after the first 10, one untimed fit per variant, then
7 timed fits per variant, the variants alternating; reported: median over the fits and [min .. max]."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import distances

import time_jeffreys_closure as tj

try:
    from sqfa_amd import logdet
except ImportError:
    logdet = None

DEV = tj.DEV
# name -> (operator module, operator, fused switch)
VARIANTS = {"affine_invariant": (distances, "affine_invariant", True),
            "log_euclidean": (distances, "log_euclidean", True)}
if logdet is not None:
    VARIANTS.update({"stein fused": (logdet, "stein", True),
                     "stein generic": (logdet, "stein", False),
                     "stein_root fused": (logdet, "stein_root", True)})


def one_fit(variant, D, K, dtype, scatters):
    module, op, switch = VARIANTS[variant]
    if logdet is not None:
        logdet.STEIN_FUSED_CLOSURE = switch
    torch.manual_seed(1)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=0.01, distance_fun=getattr(module, op))
    model = (model.double() if dtype == torch.float64 else model).to(DEV)
    with tj.ClosureEvents() as clock:
        loss, _ = model.fit(data_statistics=scatters, max_epochs=8, atol=0.0, show_progress=False, return_loss=True)
        clock.mark()
        torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    ev = clock.events
    gaps = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(len(ev) - 1)])[tj.SKIP:]
    return float(np.median(gaps)), len(ev) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--quick", action="store_true", help="third size only (rehearsal)")
    ap.add_argument("--untouched", action="store_true", help="affine_invariant and log_euclidean alone, as on a tree without the module")
    args = ap.parse_args()
    if args.untouched:
        for v in [v for v in VARIANTS if v.startswith("stein")]:
            del VARIANTS[v]
    if not torch.cuda.is_available():
        sys.exit("time_stein_closure.py measures on the GPU only")
    lines = [f"# tools/time_stein_closure.py -- {args.label} -- sqfa_amd.logdet "
             f"{'present' if logdet is not None else 'absent'} -- {torch.cuda.get_device_name(0)}",
             f"# ms per closure inside fit() (device events): median [min .. max] over {tj.FITS} fits; closures per fit",
             f"# {'C':>4} {'D':>4} {'K':>3} dtype   {'variant':<19} {'ms per closure':<30} closures"]
    print("\n".join(lines), flush=True)
    sizes = (tj.SIZES[2],) if args.quick else tj.SIZES
    for C, D, K, dtype in sizes:
        scatters = tj.statistics(C, D, dtype)["covariances"]
        times = {v: [] for v in VARIANTS}
        calls = {}
        for v in VARIANTS:
            one_fit(v, D, K, dtype, scatters)     # untimed: libraries, allocator, symmetry check of the statistics
        for _ in range(tj.FITS):
            for v in VARIANTS:
                ms, calls[v] = one_fit(v, D, K, dtype, scatters)
                times[v].append(ms)
        for v in VARIANTS:
            line = f"  {C:>4} {D:>4} {K:>3} {str(dtype)[6:]:<7} {v:<19} {tj.fmt(times[v]):<30} {calls[v]}"
            print(line, flush=True)
            lines.append(line)
        del scatters
        torch.cuda.empty_cache()
    if logdet is not None:
        logdet.STEIN_FUSED_CLOSURE = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
