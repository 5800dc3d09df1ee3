"""ms per closure inside fit() and peak memory of a fit from labelled points, dense statistics against points mode:

  dense    fit(X=X, y=y): class_statistics once ((C,D,D) tensors), every closure projects them
  points   fit(X=X, y=y, statistics="points"): statistics.ClassPoints, every closure reads the points twice

for SecondMomentsSQFA / affine_invariant and SQFA / fisher_rao_lower_bound.

ms per closure: the statistics are built first (not timed); two fits from the same start, of E1 and E2 epochs, are timed
from call to return with the device drained, and the closures of each (evaluations of the fitting loop's graph runner) are
counted:  ms = (t(E2) - t(E1)) / (closures(E2) - closures(E1)), so that set-up, warm-up closures and the graph capture
cancel.  The variants alternate inside every repeat after one warm-up fit each; median [min .. max] over the repeats.
peak: torch.cuda.max_memory_allocated over one whole fit(X=X, y=y, ...) of E1 epochs beyond what was allocated before it
(the points and labels), statistics included.  On a tree without the points mode (the parent commit) only dense is timed.

    python tools/time_point_closure.py [--repeats 7] [--out profiles/point_closure_time.txt] [--label NAME] [--quick]
                                       [--shapes 0,1,2]
"""
import argparse
import os
import statistics as pystat
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sqfa_amd  # noqa: E402
from sqfa_amd import _optim, statistics  # noqa: E402

HAS_POINTS = hasattr(statistics, "ClassPoints")
DEV = torch.device("cuda:0")
SHAPES = [  # C, D, K, N, dtype
    (1000, 784, 16, 60000, torch.float32),
    (1000, 2048, 32, 60000, torch.float32),
    (100, 3072, 16, 50000, torch.float32),
    (10, 784, 16, 60000, torch.float32),
    (1000, 784, 16, 60000, torch.float64),
]
MODELS = [("smsqfa", "affine_invariant"), ("sqfa", "fisher_rao_lower_bound")]
E1, E2 = 2, 6


def make_points(C, D, N, dtype, seed=0):
    """Balanced classes, unit noise around class offsets of 0.3 (tools/time_class_statistics.py)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = (torch.arange(N) % C)[torch.randperm(N, generator=g)].to(DEV)
    X = torch.randn(N, D, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV, dtype=dtype)
    X += 0.3 * torch.randn(C, D, generator=torch.Generator(device=DEV).manual_seed(seed + 1), device=DEV, dtype=dtype)[y]
    return X, y


def make_model(kind, D, K, dtype):
    torch.manual_seed(1)
    cls = sqfa_amd.model.SQFA if kind == "sqfa" else sqfa_amd.model.SecondMomentsSQFA
    model = cls(n_dim=D, n_filters=K, feature_noise=0.01)
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


def timed_fit(kind, D, K, dtype, epochs, **data):
    model = make_model(kind, D, K, dtype)
    torch.cuda.synchronize()
    with CountClosures() as count:
        t0 = time.perf_counter()
        model.fit(max_epochs=epochs, show_progress=False, atol=0.0, **data)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, count.n


def ms_per_closure(kind, D, K, dtype, data):
    t1, n1 = timed_fit(kind, D, K, dtype, E1, data_statistics=data)
    t2, n2 = timed_fit(kind, D, K, dtype, E2, data_statistics=data)
    return (t2 - t1) / max(n2 - n1, 1)


def peak_of_fit(kind, D, K, dtype, X, y, **kw):
    model = make_model(kind, D, K, dtype)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    model.fit(X=X, y=y, max_epochs=E1, show_progress=False, **kw)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_closure_time.txt"))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--quick", action="store_true", help="first and fourth shape only, 3 repeats (rehearsal)")
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into SHAPES (long runs in parts)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing is timed without one"
    shapes = [SHAPES[0], SHAPES[3]] if args.quick else [SHAPES[int(i)] for i in args.shapes.split(",")]
    repeats = 3 if args.quick else args.repeats
    lines = [f"# tools/time_point_closure.py -- {args.label} -- points mode {'present' if HAS_POINTS else 'absent'} -- "
             f"{torch.cuda.get_device_name(0)}",
             f"# ms per closure inside fit(): median [min .. max] over {repeats} repeats (variants alternate inside a repeat);",
             "# peak GB: max_memory_allocated over fit(X=X, y=y) beyond the points, statistics included; points GB: N D elements",
             "#     C     D   K      N dtype   model   variant   ms per closure               peak GB  points GB  one (C,D,D) GB"]
    print("\n".join(lines), flush=True)
    import contextlib
    import io
    for C, D, K, N, dtype in shapes:
        X, y = make_points(C, D, N, dtype)
        esz = X.element_size()
        for kind, op in MODELS:
            with contextlib.redirect_stdout(io.StringIO()):      # the loop's "Reached max_epochs" lines
                dense = statistics.class_statistics(X, y)
                data = {"dense": dense if kind == "sqfa" else dense["second_moments"]}
                del dense
                if HAS_POINTS:
                    data["points"] = statistics.ClassPoints(X, y)
                ms = {v: [] for v in data}
                for v in data:                                   # warm-up
                    ms_per_closure(kind, D, K, dtype, data[v])
                for _ in range(repeats):
                    for v in data:
                        ms[v].append(ms_per_closure(kind, D, K, dtype, data[v]))
                del data
                torch.cuda.empty_cache()
                peak = {"dense": peak_of_fit(kind, D, K, dtype, X, y)}
                if HAS_POINTS:
                    peak["points"] = peak_of_fit(kind, D, K, dtype, X, y, statistics="points")
            for v in ms:
                line = (f"  {C:5d} {D:5d} {K:3d} {N:6d} {str(dtype)[6:]:7s} {kind:7s} {v:8s} "
                        f"{pystat.median(ms[v]):8.3f} [{min(ms[v]):8.3f} .. {max(ms[v]):8.3f}]  {peak[v] / 1e9:7.3f}  "
                        f"{N * D * esz / 1e9:8.3f}  {C * D * D * esz / 1e9:8.3f}")
                print(line, flush=True)
                lines.append(line)
        del X, y
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
