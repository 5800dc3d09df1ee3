"""OAS shrinkage in points mode: what it costs per closure, and what the coefficient pass costs once per fit.

Table 1, ms per closure inside fit() of SecondMomentsSQFA / affine_invariant from a statistics.ClassPoints:

  empirical   ClassPoints(X, y)                     sqfa_class_feature_moments and its backward
  oas         ClassPoints(X, y, estimator="oas")    the shrunk entries: one (K,K) Gram of F, one (C,K,K) reduction and K
                                                    virtual rows more per closure

Two fits from the same start, of E1 and E2 epochs, are timed with device events from call to return, and the closures of
each (evaluations of the fitting loop's graph runner) are counted:  ms = (t(E2) - t(E1)) / (closures(E2) - closures(E1)),
so that set-up, warm-up closures and the graph capture cancel (tools/time_point_closure.py).  The variants alternate inside
every repeat after one warm-up each; median [min .. max] over the repeats.  On a tree whose ClassPoints takes no estimator
(the parent commit) only `empirical` is timed: run it there twice for the spread that this commit's `empirical` must lie in.

Table 2, the coefficient pass: one _native.class_shrinkage call (the means are there already) against one
class_statistics(X, y, "oas") call, device events, and the peak of allocated memory of one call beyond the inputs.

    python tools/time_point_oas.py [--repeats 7] [--out profiles/point_oas_time.txt] [--label NAME] [--shapes 0,1,2,3]
                                   [--no-dense]
    python tools/time_point_oas.py --trace     # a few closures' worth of native calls per shape, nothing timed: the
                                               # program of a rocprofv3 --kernel-trace --stats run of its own
"""
import argparse
import contextlib
import inspect
import io
import os
import statistics as pystat
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sqfa_amd  # noqa: E402
from sqfa_amd import _native, _optim, statistics  # noqa: E402

HAS_OAS = "estimator" in inspect.signature(statistics.ClassPoints.__init__).parameters
DEV = torch.device("cuda:0")
SHAPES = [  # C, D, K, N, dtype: the README's points table
    (1000, 784, 16, 60000, torch.float32),
    (1000, 784, 16, 60000, torch.float64),
    (100, 3072, 16, 50000, torch.float32),
    (10, 784, 16, 60000, torch.float32),
]
E1, E2 = 2, 6


def make_points(C, D, N, dtype, seed=0):
    """Balanced classes, unit noise around class offsets of 0.3 (tools/time_point_closure.py)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = (torch.arange(N) % C)[torch.randperm(N, generator=g)].to(DEV)
    X = torch.randn(N, D, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV, dtype=dtype)
    X += 0.3 * torch.randn(C, D, generator=torch.Generator(device=DEV).manual_seed(seed + 1), device=DEV, dtype=dtype)[y]
    return X, y


def make_model(D, K, dtype):
    torch.manual_seed(1)
    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=D, n_filters=K, feature_noise=0.01)
    return (model.double() if dtype == torch.float64 else model).to(DEV)


class CountClosures:
    """Counts the evaluations of the fitting loop's graph runner (one per closure) while active."""

    def __enter__(self):
        self.n, self.saved = 0, _optim.GraphRunner.run
        counter = self

        def run(runner, *a, **k):
            counter.n += 1
            return counter.saved(runner, *a, **k)

        _optim.GraphRunner.run = run
        return self

    def __exit__(self, *exc):
        _optim.GraphRunner.run = self.saved
        return False


def event_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def timed_fit(D, K, dtype, epochs, data):
    model = make_model(D, K, dtype)
    with CountClosures() as count:
        ms, _ = event_ms(lambda: model.fit(data_statistics=data, max_epochs=epochs, show_progress=False, atol=0.0))
        return ms, count.n


def ms_per_closure(D, K, dtype, data):
    t1, n1 = timed_fit(D, K, dtype, E1, data)
    t2, n2 = timed_fit(D, K, dtype, E2, data)
    return (t2 - t1) / max(n2 - n1, 1)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def spread(values):
    return f"{pystat.median(values):8.3f} [{min(values):8.3f} .. {max(values):8.3f}]"


def trace_driver(shapes):
    """Five closures' worth of native calls per shape and variant, for a kernel trace."""
    for C, D, K, N, dtype in shapes:
        X, y = make_points(C, D, N, dtype)
        F = (torch.randn(K, D, device=DEV, dtype=dtype) / D ** 0.5).contiguous()
        G, g = torch.randn(C, K, K, device=DEV, dtype=dtype), torch.randn(C, K, device=DEV, dtype=dtype)
        for est in (("empirical", "oas") if HAS_OAS else ("empirical",)):
            cp = statistics.ClassPoints(X, y, estimator=est) if HAS_OAS else statistics.ClassPoints(X, y)
            for _ in range(5):
                zc = _native.class_feature_moments(cp, F, True, 0.01)[0]
                _native.class_feature_moments_backward(cp, zc, G, g, *((F,) if est == "oas" else ()))
        torch.cuda.synchronize()
        del X, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_oas_time.txt"))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--no-dense", action="store_true", help="table 2 without the dense class_statistics call")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing is timed without one"
    shapes = [SHAPES[int(i)] for i in args.shapes.split(",")]
    if args.trace:
        return trace_driver(shapes)
    variants = ("empirical", "oas") if HAS_OAS else ("empirical",)
    lines = [f"# tools/time_point_oas.py -- {args.label} -- ClassPoints(estimator=) {'present' if HAS_OAS else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             f"# table 1: ms per closure inside fit() (smsqfa / affine_invariant, from a ClassPoints): median [min .. max] over "
             f"{args.repeats} repeats, device events, variants alternating inside a repeat",
             "#     C     D   K      N dtype   variant     ms per closure"]
    print("\n".join(lines), flush=True)
    table2 = ["# table 2: the coefficient pass, once per fit: ms per call, median [min .. max], and peak of allocated memory of one "
              "call beyond the inputs",
              "#     C     D      N dtype   call                          ms per call                    peak MB"]
    for C, D, K, N, dtype in shapes:
        X, y = make_points(C, D, N, dtype)
        with contextlib.redirect_stdout(io.StringIO()):      # the loop's "Reached max_epochs" lines
            data = {v: (statistics.ClassPoints(X, y, estimator=v) if HAS_OAS else statistics.ClassPoints(X, y)) for v in variants}
            ms = {v: [] for v in variants}
            for v in variants:                               # warm-up
                ms_per_closure(D, K, dtype, data[v])
            for _ in range(args.repeats):
                for v in variants:
                    ms[v].append(ms_per_closure(D, K, dtype, data[v]))
        for v in variants:
            line = f"  {C:5d} {D:5d} {K:3d} {N:6d} {str(dtype)[6:]:7s} {v:10s} {spread(ms[v])}"
            print(line, flush=True)
            lines.append(line)
        cp = data["empirical"]
        del data
        calls = {}
        if HAS_OAS:
            calls["class_shrinkage"] = lambda: _native.class_shrinkage(cp.points, cp.order, cp.class_start, cp.means, C)
        if not args.no_dense:
            calls["class_statistics(oas)"] = lambda: statistics.class_statistics(X, y, estimator="oas")
        times = {k: [] for k in calls}
        for k in calls:                                      # warm-up
            calls[k]()
        for _ in range(args.repeats):
            for k in calls:
                times[k].append(event_ms(calls[k])[0])
        for k in calls:
            line = (f"  {C:5d} {D:5d} {N:6d} {str(dtype)[6:]:7s} {k:24s} {spread(times[k])}  {peak_of(calls[k]) / 1e6:10.2f}")
            print(line, flush=True)
            table2.append(line)
        del X, y, cp, calls
        torch.cuda.empty_cache()
    print("\n".join(table2), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines + table2) + "\n")


if __name__ == "__main__":
    main()
