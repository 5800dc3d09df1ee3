"""Timing of the native Gaussian log-loss (sqfa_amd.classify) on the six rows of the README's classification table.

    python tools/time_log_loss.py [--parent TREE] [--out profiles/log_loss_time.txt]
    python tools/time_log_loss.py --once            (five loss-plus-gradient calls at the first row, for a kernel trace)

Device events, the median [min .. max] of 7 runs with the variants alternating inside every run:
  (a) native predict and log_evidence of the PARENT commit (a built checkout at TREE), two runs, each in a fresh process
  (b) the same on this commit, measured the same way: two fresh processes, alternating with (a)'s
  (c) native log_loss, forward (factor pass not included: the classifier is built once)
  (d) native loss plus all three gradients (gaussian_log_loss + backward: factor pass, forward, backward)
  (e) the torch expression, loss plus backward, with its peak memory next to (d)'s
Flop model: 2 N C K^2 per product; the forward is one product, the backward recomputes y (twice in the class-owned pass)
and adds two products of the same size."""
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
    """{name: (median, min, max) ms, peak bytes} of callables, alternating inside every run (one warm-up run first)."""
    times = {name: [] for name in variants}
    peaks = {}
    for run in range(RUNS + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            if run:
                times[name].append(start.elapsed_time(stop))
            peaks[name] = torch.cuda.max_memory_allocated() - before
    return {name: dict(ms=(statistics.median(t), min(t), max(t)), peak=peaks[name]) for name, t in times.items()}


def scorer_only():
    """predict and log_evidence on whichever sqfa_amd is importable: one JSON line per row."""
    from sqfa_amd import classify
    for N, C, K, dtype in ROWS:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        out = measure({"predict": lambda: clf.predict(Z), "log_evidence": lambda: clf.log_evidence(Z)})
        print(json.dumps({"row": [N, C, K, dtype], "predict": out["predict"]["ms"], "log_evidence": out["log_evidence"]["ms"]}),
              flush=True)


def scorer_runs(trees, count=2):
    """{tree: [run, ...]}: `count` runs per tree, alternating between the trees, a fresh process each (the tree's package
    and library)."""
    runs = {tree: [] for tree in trees}
    for _ in range(count):
        for tree in trees:
            env = dict(os.environ, PYTHONPATH=tree)
            env.pop("SQFA_HIP_LIBRARY", None)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--scorer-only"], env=env, cwd=tree, check=True,
                                 capture_output=True, text=True, timeout=300)
            rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
            runs[tree].append({tuple(r["row"]): r for r in rows})
    return runs


def once():
    sys.path.insert(0, ROOT)
    from sqfa_amd import classify
    N, C, K, dtype = ROWS[0]
    Z, y, mu, cov = problem(N, C, K, dtype)
    leaves = [t.clone().requires_grad_() for t in (Z, mu, cov)]
    for _ in range(5):
        for t in leaves:
            t.grad = None
        classify.gaussian_log_loss(leaves[0], y, leaves[1], leaves[2]).backward()
    torch.cuda.synchronize()


def fmt(ms):
    return f"{ms[0]:9.3f} [{ms[1]:.3f} .. {ms[2]:.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_loss_time.txt"))
    ap.add_argument("--scorer-only", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.scorer_only:
        return scorer_only()
    if args.once:
        return once()
    sys.path.insert(0, ROOT)
    from sqfa_amd import classify
    scorer = scorer_runs(([args.parent] if args.parent else []) + [ROOT])
    parents, ours = scorer.get(args.parent, []) if args.parent else [], scorer[ROOT]
    lines = [f"# tools/time_log_loss.py -- {torch.cuda.get_device_name(0)} -- torch {torch.__version__}",
             f"# ms per call (device events): median [min .. max] over {RUNS} runs, variants alternating inside every run;",
             "# peak = bytes allocated above the inputs during the call.  (a) parent commit and (b) this commit: predict and",
             "# log_evidence alone, a fresh process per run, the two trees alternating; (c)-(e) this commit, one process"]
    for N, C, K, dtype in ROWS:
        Z, y, mu, cov = problem(N, C, K, dtype)
        clf = classify.GaussianClassifier(mu, cov)
        leaves = [t.clone().requires_grad_() for t in (Z, mu, cov)]

        def loss_and_gradients():
            for t in leaves:
                t.grad = None
            classify.gaussian_log_loss(leaves[0], y, leaves[1], leaves[2]).backward()

        def torch_loss_and_gradients():
            classify.NATIVE_LOG_LOSS = False
            try:
                loss_and_gradients()
            finally:
                classify.NATIVE_LOG_LOSS = True

        out = measure({"log_evidence": lambda: clf.log_evidence(Z), "log_loss": lambda: clf.log_loss(Z, y),
                       "native": loss_and_gradients, "torch": torch_loss_and_gradients})
        flops = 2.0 * N * C * K * K
        lines.append(f"N={N} C={C} K={K} {dtype}:")
        for i, run in enumerate(parents):
            r = run[(N, C, K, dtype)]
            lines.append(f"    (a) parent run {i + 1}: predict {fmt(r['predict'])}   log_evidence {fmt(r['log_evidence'])}")
        for i, run in enumerate(ours):
            r = run[(N, C, K, dtype)]
            lines.append(f"    (b) this   run {i + 1}: predict {fmt(r['predict'])}   log_evidence {fmt(r['log_evidence'])}")
        c, d, e = out["log_loss"], out["native"], out["torch"]
        lines.append(f"    (c) native log_loss, forward        {fmt(c['ms'])}   peak {c['peak'] / 1e6:10.2f} MB   "
                     f"{c['ms'][0] / out['log_evidence']['ms'][0]:.2f} x log_evidence")
        lines.append(f"    (d) native loss + three gradients   {fmt(d['ms'])}   peak {d['peak'] / 1e6:10.2f} MB   "
                     f"{d['ms'][0] / c['ms'][0]:.2f} x (c) (flop model: 1 + 3), {4 * flops / d['ms'][0] / 1e9:.1f} TF of 4 x 2 N C K^2")
        lines.append(f"    (e) torch loss + backward           {fmt(e['ms'])}   peak {e['peak'] / 1e6:10.2f} MB   "
                     f"(e) / (d): {e['ms'][0] / d['ms'][0]:.1f} x in time, {e['peak'] / max(d['peak'], 1):.0f} x in peak memory")
        print("\n".join(lines[-(4 + len(parents) + len(ours)):]), flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
