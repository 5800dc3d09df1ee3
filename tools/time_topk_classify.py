"""Timing of the top-k predictions and the label's rank (sqfa_amd.classify: predict_topk, label_rank, topk_accuracy) on the
six rows of the README's classification table.

    python tools/time_topk_classify.py [--parent TREE] [--out profiles/topk_classify_time.txt]
    python tools/time_topk_classify.py --once      (three predict_topk(5) and label_rank calls at the first row, for a kernel trace)

Device events, the median [min .. max] of 7 runs with the variants alternating inside every run; every child process under
a time limit of its own:
  (a) native predict of the PARENT commit (a built checkout at TREE), two runs, each in a fresh process
  (b) the same on this commit, measured the same way: two fresh processes, alternating with (a)'s
  (c) predict_topk(k=5)            (d) label_rank            (e) topk_accuracy
  (f) what gives (c) without it: scores(Z) + torch.topk(5)
  (g) what gives (d) without it: scores(Z) + gather + compare + sum
and the peak memory beyond the inputs of (c), (d), (f), (g).
Gate 1: (c) faster than (f) and (d) faster than (g) by more than the spread of the two, and smaller in peak memory, at every
row.  Gate 2: (b) within [min .. max] of (a).  Reported: (c) / (b), (d) / (b); the flop model says 1 and 1 + 16 / C."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(60000, 1000, 16, "float32"), (60000, 1000, 16, "float64"), (10000, 10, 16, "float32"), (50000, 100, 16, "float32"),
        (60000, 300, 32, "float32"), (20000, 100, 64, "float32")]
RUNS = 7
CHILD_SECONDS = 240
TOP = 5


def problem(N, C, K, dtype, device="cuda:0"):
    g = torch.Generator().manual_seed(N + C + K)
    A = torch.randn(C, K, K + 3, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2) / (K + 3) + 0.05 * torch.eye(K, dtype=torch.float64)
    mu = torch.randn(C, K, generator=g, dtype=torch.float64)
    y = torch.arange(N) % C
    Z = mu[y] + torch.einsum("nij,nj->ni", torch.linalg.cholesky(cov)[y], torch.randn(N, K, generator=g, dtype=torch.float64))
    dt = getattr(torch, dtype)
    return Z.to(device, dt), y.to(device), mu.to(device, dt), cov.to(device, dt)


def measure(variants):
    """{name: (median, min, max) ms} of callables, alternating inside every run (one warm-up run first)."""
    times = {name: [] for name in variants}
    for run in range(RUNS + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            if run:
                times[name].append(start.elapsed_time(stop))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def peak_bytes(fn):
    """The rise of the allocator's peak over what is allocated before the call (the inputs and the classifier)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def scorer_only():
    """predict on whichever sqfa_amd is importable: one JSON line per row."""
    from sqfa_amd import classify
    for N, C, K, dtype in ROWS:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        out = measure({"predict": lambda: clf.predict(Z)})
        print(json.dumps({"row": [N, C, K, dtype], "predict": out["predict"]}), flush=True)


def scorer_runs(trees, count=2):
    """{tree: [run, ...]}: `count` runs per tree, alternating between the trees, a fresh process each (the tree's package
    and library)."""
    runs = {tree: [] for tree in trees}
    for _ in range(count):
        for tree in trees:
            env = dict(os.environ, PYTHONPATH=tree)
            env.pop("SQFA_HIP_LIBRARY", None)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--scorer-only"], env=env, cwd=tree, check=True,
                                 capture_output=True, text=True, timeout=CHILD_SECONDS)
            rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
            runs[tree].append({tuple(r["row"]): r for r in rows})
    return runs


def once():
    sys.path.insert(0, ROOT)
    from sqfa_amd import classify
    N, C, K, dtype = ROWS[0]
    Z, y, mu, cov = problem(N, C, K, dtype)
    clf = classify.GaussianClassifier(mu, cov)
    for _ in range(3):
        clf.predict(Z)
        clf.predict_topk(Z, TOP)
        clf.label_rank(Z, y)
    torch.cuda.synchronize()


def fmt(ms):
    return f"{ms[0]:9.3f} [{ms[1]:.3f} .. {ms[2]:.3f}] ms"


def faster(native, other):
    """native is faster than other by more than the spread of the two: the intervals [min .. max] do not meet."""
    return native[2] < other[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_classify_time.txt"))
    ap.add_argument("--scorer-only", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.scorer_only:
        return scorer_only()
    if args.once:
        return once()
    sys.path.insert(0, ROOT)
    from sqfa_amd import classify
    parent = os.path.abspath(args.parent) if args.parent else None
    scorer = scorer_runs(([parent] if parent else []) + [ROOT])
    parents, ours = scorer.get(parent, []) if parent else [], scorer[ROOT]
    lines = [f"# tools/time_topk_classify.py -- {torch.cuda.get_device_name(0)} -- torch {torch.__version__}",
             f"# ms per call (device events): median [min .. max] over {RUNS} runs, variants alternating inside every run.",
             "# (a) parent commit and (b) this commit: predict alone, a fresh process per run, the two trees alternating;",
             f"# (c) predict_topk(k={TOP}), (d) label_rank, (e) topk_accuracy, (f) scores + torch.topk({TOP}), (g) scores + gather +",
             "# compare + sum: this commit, one process.  Gate 1: (c) < (f) and (d) < (g) beyond the spread of the two, in time",
             "# and in peak memory beyond the inputs.  Gate 2: (b) within [min .. max] of (a)."]
    for N, C, K, dtype in ROWS:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        assert clf._use_topk_native(Z)
        classes = torch.arange(C, device=Z.device)[None]

        def by_topk():
            return torch.topk(clf.scores(Z), TOP, dim=1)[1]

        def by_count():
            S = clf.scores(Z)
            s_y = S.gather(1, y[:, None])
            return ((S > s_y) | ((S == s_y) & (classes < y[:, None]))).sum(1)

        agree_top = float((clf.predict_topk(Z, TOP) == by_topk()).all(1).double().mean())   # torch.topk may order ties otherwise
        agree_rank = float((clf.label_rank(Z, y) == by_count()).double().mean())
        out = measure({"predict": lambda: clf.predict(Z), "predict_topk": lambda: clf.predict_topk(Z, TOP),
                       "label_rank": lambda: clf.label_rank(Z, y), "topk_accuracy": lambda: clf.topk_accuracy(Z, y),
                       "by_topk": by_topk, "by_count": by_count})
        b, c, d, e, f, g = (out[k] for k in ("predict", "predict_topk", "label_rank", "topk_accuracy", "by_topk", "by_count"))
        mem = {name: peak_bytes(fn) / 1e6 for name, fn in (("c", lambda: clf.predict_topk(Z, TOP)), ("d", lambda: clf.label_rank(Z, y)),
                                                           ("f", by_topk), ("g", by_count))}
        lines.append(f"N={N} C={C} K={K} {dtype}: predict_topk equals scores + torch.topk on {agree_top:.4%} of the samples, "
                     f"label_rank equals the count on the scores on {agree_rank:.4%}")
        lo = min(r[(N, C, K, dtype)]["predict"][1] for r in parents) if parents else None
        hi = max(r[(N, C, K, dtype)]["predict"][2] for r in parents) if parents else None
        for i, run in enumerate(parents):
            lines.append(f"    (a) parent run {i + 1}: predict {fmt(run[(N, C, K, dtype)]['predict'])}")
        for i, run in enumerate(ours):
            med = run[(N, C, K, dtype)]["predict"]
            verdict = "" if lo is None else f"   gate 2: {'within' if lo <= med[0] <= hi else 'OUTSIDE'} [{lo:.3f} .. {hi:.3f}]"
            lines.append(f"    (b) this   run {i + 1}: predict {fmt(med)}{verdict}")
        flops = 2.0 * N * C * K * K
        lines.append(f"    (b) predict, this process           {fmt(b)}")
        lines.append(f"    (c) predict_topk(k={TOP})               {fmt(c)}   (c) / (b) {c[0] / b[0]:.2f}   "
                     f"{flops / c[0] / 1e9:.1f} TF of 2 N C K^2   peak {mem['c']:.1f} MB")
        lines.append(f"    (d) label_rank                      {fmt(d)}   (d) / (b) {d[0] / b[0]:.2f}   model {1 + 16 / C:.2f}   "
                     f"peak {mem['d']:.1f} MB")
        lines.append(f"    (e) topk_accuracy                   {fmt(e)}   (e) / (d) {e[0] / d[0]:.2f}")
        verdict = "holds" if faster(c, f) and mem["c"] < mem["f"] else "FAILS"
        lines.append(f"    (f) scores + torch.topk({TOP})           {fmt(f)}   (f) / (c) {f[0] / c[0]:.1f}   peak {mem['f']:.1f} MB   "
                     f"gate 1 {verdict}")
        verdict = "holds" if faster(d, g) and mem["d"] < mem["g"] else "FAILS"
        lines.append(f"    (g) scores + gather, compare, sum   {fmt(g)}   (g) / (d) {g[0] / d[0]:.1f}   peak {mem['g']:.1f} MB   "
                     f"gate 1 {verdict}")
        print("\n".join(lines[-(7 + len(parents) + len(ours)):]), flush=True)
        del Z, y, mu, cov, clf, classes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
