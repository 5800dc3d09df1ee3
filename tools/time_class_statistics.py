"""ms and peak memory of statistics.class_statistics on the GPU: (a) the parent commit's module (--parent FILE, a copy of its
sqfa_amd/statistics.py: `git show HEAD~1:sqfa_amd/statistics.py > FILE`), (b) this tree with NATIVE_CLASS_STATISTICS off,
(c) this tree native.  The variants alternate inside every repeat, after a warm-up of each, so that they see the same
clock and neighbours; a call is timed with device events around it and ends in a synchronise.  Peak memory is
torch.cuda.max_memory_allocated over one call minus what was allocated before it (the points and labels).

    python tools/time_class_statistics.py [--parent FILE] [--repeats 7] [--out profiles/class_statistics_time.txt]
"""
import argparse
import importlib.util
import os
import statistics as pystat
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sqfa_amd import _native, statistics  # noqa: E402

SHAPES = [  # name, C, D, N, ragged, dtype, estimators
    ("c3-like ragged", 1000, 784, 60000, True, torch.float32, ("empirical", "oas")),
    ("c3-like ragged", 1000, 784, 60000, True, torch.float64, ("empirical",)),
    ("c1-like", 10, 784, 60000, False, torch.float32, ("empirical", "oas")),
    ("c5-like", 100, 3072, 50000, False, torch.float32, ("empirical", "oas")),
]


def make_points(C, D, N, ragged, dtype, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if ragged:
        w = torch.rand(C, generator=g) ** 2 + 0.05
        y = torch.multinomial(w / w.sum(), N, replacement=True, generator=g)
        y[:C] = torch.arange(C)            # every class occurs
    else:
        y = torch.arange(N) % C
        y = y[torch.randperm(N, generator=g)]
    y = y.to(dev)
    X = torch.randn(N, D, generator=torch.Generator(device=dev).manual_seed(seed), device=dev, dtype=dtype)
    X += 0.3 * torch.randn(C, D, generator=torch.Generator(device=dev).manual_seed(seed + 1), device=dev, dtype=dtype)[y]
    return X, y


def load_parent(path):
    spec = importlib.util.spec_from_file_location("parent_statistics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def one_call(fn, X, y, estimator):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn(X, y, estimator)
    t1.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return t0.elapsed_time(t1), peak, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_statistics_time.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing is timed without one"
    dev = torch.device("cuda:0")

    def switched(native):
        def fn(X, y, estimator):
            statistics.NATIVE_CLASS_STATISTICS = native
            try:
                return statistics.class_statistics(X, y, estimator=estimator)
            finally:
                statistics.NATIVE_CLASS_STATISTICS = True
        return fn

    variants = []
    if args.parent:
        parent = load_parent(args.parent)
        variants.append(("(a) parent", lambda X, y, e: parent.class_statistics(X, y, estimator=e)))
    variants += [("(b) switch off", switched(False)), ("(c) native", switched(True))]

    lines = [f"# tools/time_class_statistics.py -- {torch.cuda.get_device_name(0)} -- class_statistics(points, labels), one call:",
             f"# ms: median [min .. max] over {args.repeats} repeats (variants alternate inside a repeat, one warm-up each);",
             "# peak: max_memory_allocated during the call beyond the inputs, GB; outputs alone are means + cov + second.",
             "# vs (b): rel_err of (c)'s second moments against (b)'s; sym: (c)'s second moments equal their transposes exactly",
             "#    C     D      N dtype   estimator  variant          ms                          peak GB  outputs GB"]
    for name, C, D, N, ragged, dtype, estimators in SHAPES:
        X, y = make_points(C, D, N, ragged, dtype, dev)
        out_gb = (2 * C * D * D + C * D) * X.element_size() / 1e9
        for est in estimators:
            ms = {v: [] for v, _ in variants}
            peak = {}
            for v, fn in variants:                      # warm-up
                one_call(fn, X, y, est)
            for _ in range(args.repeats):
                for v, fn in variants:
                    t, p, out = one_call(fn, X, y, est)
                    ms[v].append(t)
                    peak[v] = max(peak.get(v, 0), p)
                    del out
            for v, _ in variants:
                lines.append(f"  {C:5d} {D:5d} {N:6d} {str(dtype)[6:]:8s} {est:10s} {v:15s} "
                             f"{pystat.median(ms[v]):9.3f} [{min(ms[v]):9.3f} .. {max(ms[v]):9.3f}]  {peak[v] / 1e9:7.2f}  {out_gb:7.2f}")
            ref = switched(False)(X, y, est)["second_moments"]
            nat = switched(True)(X, y, est)["second_moments"]
            err = float((nat - ref).norm() / ref.norm())
            sym = bool(torch.equal(nat, nat.transpose(1, 2)))
            verdict = bool(_native._is_symmetric_batch(nat))
            lines.append(f"#   {name}: (c) vs (b) rel_err {err:.2e}; sym {sym}; _is_symmetric_batch {verdict}")
            print("\n".join(lines[-len(variants) - 1:]), flush=True)
            del ref, nat
        del X, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
