"""ms per loss+gradient closure of SQFA with bhattacharyya / hellinger / mahalanobis_sq / mahalanobis as distance_fun:

  (a) generic   the fitting loop's generic closure: get_class_distances (GaussPairTerms + element-wise chain), validity
                check on the host, tril gather + mean, autograd backward
  (b) fused     _fused_closure_loss (projection -> noise -> ClassPairLoss) + backward, eager
  (c) graph     the same, captured once in a HIP graph and replayed
  pairs         the pair stage alone on the (C,K) / (C,K,K) feature statistics: sqfa_gauss_pair_terms forward + backward
                (Q and LD with unit upstream gradients: the two launches the fused call replaces, without the element-wise
                chain between them) next to one sqfa_gauss_pairwise_loss call

    python tools/time_gauss_closure.py [--out profiles/gauss_closure_time.txt] [--label NAME] [--quick]

On a tree without the fused path (no distances.GAUSS_FUSED_CLOSURE) only (a) and the two-launch pair stage are reported: run it
there for the baseline.  Sizes (C, D, K): (1000, 784, 16) (300, 784, 16) (30, 784, 16) (10, 784, 4) (300, 784, 32); float32 and
float64.  Statistics: 0.7 x a common covariance + 0.3 x a per-class Wishart (overlapping classes), means 0.3 randn,
feature_noise 0.01.  Timing: after 5 warm-up calls, 7 rounds of `reps` calls between device events (reps sized so that a
round lasts ~50 ms or more); reported: median ms per call and [min .. max] over the rounds (the run-to-run spread);
(a) and (b)/(c) alternate within one process."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sqfa_amd
from sqfa_amd import _native, distances

DEV = "cuda:0"
OPS = ("bhattacharyya", "hellinger", "mahalanobis_sq", "mahalanobis")
SIZES = ((1000, 784, 16), (300, 784, 16), (30, 784, 16), (10, 784, 4), (300, 784, 32))
HAS_FUSED = hasattr(distances, "GAUSS_FUSED_CLOSURE")


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
    mu = 0.3 * torch.randn(C, D, generator=g, device=DEV, dtype=torch.float32).to(dtype)
    return {"means": mu, "covariances": cov}


def timed(fn, target_ms=50.0, rounds=7, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = int(max(5, min(200, target_ms / max(a.elapsed_time(b), 1e-3))))
    out = []
    for _ in range(rounds):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def fmt(t):
    return "      -      " if t is None else f"{t[0]:7.3f} [{t[1]:.3f} .. {t[2]:.3f}]"


def closures(model, stats):
    prepared = model._prepare_statistics(stats)
    (param,) = list(model.parameters())
    C = stats["means"].shape[0]
    rows, cols = (t.to(DEV) for t in torch.tril_indices(C, C, offset=-1))

    def generic():
        param.grad = None
        Dm = model.get_class_distances(prepared, regularized=True)
        if torch.isnan(Dm).any() or torch.isinf(Dm).any():   # the loop's check_distances_valid: two host synchronisations
            raise ValueError("non-finite distances")
        (-Dm[rows, cols].mean()).backward()

    def fused():
        param.grad = None
        loss, _flags = model._fused_closure_loss(prepared)
        loss.backward()

    return generic, fused


def graphed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def pair_stage(fmu, fcov, kind):
    def two_launch():
        Q, LD, _, _ = _native.hip_gauss_terms(fmu, fcov, fmu, fcov)
        ones = torch.ones_like(Q)
        _native.hip_gauss_terms(fmu, fcov, fmu, fcov, ones, ones if kind <= 1 else None, want_outputs=False, want_grad=True)

    def one_call():
        _native.hip_gauss_pairwise_loss(fmu, fcov, kind, 1e-6, -1.0)

    return two_launch, (one_call if HAS_FUSED else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--quick", action="store_true", help="first and fourth size only (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_gauss_closure.py measures on the GPU only")
    lines = [f"# tools/time_gauss_closure.py -- {args.label} -- fused path {'present' if HAS_FUSED else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             "# ms per call: median [min .. max over 7 rounds]",
             f"# {'C':>4} {'D':>4} {'K':>3} dtype   {'operator':<15} {'(a) generic':<26} {'(b) fused eager':<26} {'(c) fused graph':<26} "
             f"{'pairs: terms fwd+bwd':<26} {'pairs: fused call':<26}"]
    print("\n".join(lines), flush=True)
    sizes = (SIZES[0], SIZES[3]) if args.quick else SIZES
    for C, D, K in sizes:
        for dtype in (torch.float32, torch.float64):
            stats = statistics(C, D, dtype)
            for kind, op in enumerate(("bhattacharyya", "hellinger", "mahalanobis_sq", "mahalanobis")):
                torch.manual_seed(1)
                model = sqfa_amd.model.SQFA(n_dim=D, n_filters=K, feature_noise=0.01, distance_fun=getattr(distances, op))
                model = (model.double() if dtype == torch.float64 else model).to(DEV)
                generic, fused = closures(model, stats)
                t_b = t_c = None
                if HAS_FUSED:
                    distances.GAUSS_FUSED_CLOSURE = False
                t_a = timed(generic)
                if HAS_FUSED:
                    distances.GAUSS_FUSED_CLOSURE = True
                    t_b = timed(fused)
                    t_c = timed(graphed(fused))
                    distances.GAUSS_FUSED_CLOSURE = False
                    t_a2 = timed(generic)   # (a) again after (b), (c): alternated; the slower-looking pair is not hidden
                    distances.GAUSS_FUSED_CLOSURE = True
                    t_a = (0.5 * (t_a[0] + t_a2[0]), min(t_a[1], t_a2[1]), max(t_a[2], t_a2[2]))
                with torch.no_grad():
                    fs = model._feature_statistics(stats, True)
                    fmu, fcov = fs["means"].contiguous(), fs["covariances"].contiguous()
                two, one = pair_stage(fmu, fcov, kind)
                t_two = timed(two)
                t_one = timed(one) if one is not None else None
                line = (f"  {C:>4} {D:>4} {K:>3} {str(dtype)[6:]:<7} {op:<15} {fmt(t_a):<26} {fmt(t_b):<26} {fmt(t_c):<26} "
                        f"{fmt(t_two):<26} {fmt(t_one):<26}")
                print(line, flush=True)
                lines.append(line)
            del stats
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
