"""Timing of the nested Gaussian classifiers (sqfa_amd.classify: nested_predict, nested_log_evidence, nested_log_loss) on
the six rows of the README's classification table.

    python tools/time_nested_classify.py [--parent TREE] [--out profiles/nested_classify_time.txt]
    python tools/time_nested_classify.py --once      (three nested_predict calls at the first row, for a kernel trace)

Device events, the median [min .. max] of 7 runs with the variants alternating inside every run; every child process under
a time limit of its own:
  (a) native predict of the PARENT commit (a built checkout at TREE), two runs, each in a fresh process
  (b) the same on this commit, measured the same way: two fresh processes, alternating with (a)'s
  (c) nested_predict            (d) nested_log_evidence            (e) nested_log_loss
  (f) what gives the same figure without them: K GaussianClassifiers on contiguous leading slices of the statistics and
      the samples, each constructed and ``predict``ed
Gate 1: (c) faster than (f) at every row.  Gate 2: (b) within [min .. max] of (a).  Reported: (c) / (b), (d) / (c).
Flop model: 2 N C K^2 for the product of (b) and of (c); (f) sums 2 N C k^2 over k: about K / 3 products."""
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
        clf.nested_predict(Z)
    torch.cuda.synchronize()


def fmt(ms):
    return f"{ms[0]:9.3f} [{ms[1]:.3f} .. {ms[2]:.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_classify_time.txt"))
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
    lines = [f"# tools/time_nested_classify.py -- {torch.cuda.get_device_name(0)} -- torch {torch.__version__}",
             f"# ms per call (device events): median [min .. max] over {RUNS} runs, variants alternating inside every run.",
             "# (a) parent commit and (b) this commit: predict alone, a fresh process per run, the two trees alternating;",
             "# (c) nested_predict, (d) nested_log_evidence, (e) nested_log_loss, (f) K sliced classifiers constructed and",
             "# predicted: this commit, one process.  Gate 1: (c) < (f).  Gate 2: (b) within [min .. max] of (a)."]
    for N, C, K, dtype in ROWS:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        assert clf._use_nested_native(Z)

        def sliced():
            out = []
            for k in range(1, K + 1):
                part = classify.GaussianClassifier(mu[:, :k].contiguous(), cov[:, :k, :k].contiguous())
                out.append(part.predict(Z[:, :k].contiguous()))
            return out

        nested, loop = clf.nested_predict(Z), torch.stack(sliced(), 1)
        agree = float((nested == loop).double().mean())
        out = measure({"predict": lambda: clf.predict(Z), "nested_predict": lambda: clf.nested_predict(Z),
                       "nested_log_evidence": lambda: clf.nested_log_evidence(Z),
                       "nested_log_loss": lambda: clf.nested_log_loss(Z, y), "sliced": sliced})
        b, c, d, e, f = (out[k] for k in ("predict", "nested_predict", "nested_log_evidence", "nested_log_loss", "sliced"))
        lines.append(f"N={N} C={C} K={K} {dtype}: nested_predict and the K sliced classifiers agree on {agree:.4%} of (n, k)")
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
        lines.append(f"    (c) nested_predict                  {fmt(c)}   (c) / (b) {c[0] / b[0]:.2f}   "
                     f"{flops / c[0] / 1e9:.1f} TF of 2 N C K^2")
        lines.append(f"    (d) nested_log_evidence             {fmt(d)}   (d) / (c) {d[0] / c[0]:.2f}")
        lines.append(f"    (e) nested_log_loss                 {fmt(e)}   (e) / (d) {e[0] / d[0]:.2f}")
        verdict = "holds" if c[0] < f[0] else "FAILS"
        lines.append(f"    (f) K sliced classifiers            {fmt(f)}   (f) / (c) {f[0] / c[0]:.1f}   gate 1 {verdict}")
        print("\n".join(lines[-(6 + len(parents) + len(ours)):]), flush=True)
        del Z, y, mu, cov, clf, nested, loop
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
