"""Developer aid: time the fused loss+gradient of the LDS pair kernel (64 < m <= 128) against the register kernel at
m = 64 and against the reference's algorithm written as a torch-ROCm expression on the same GPU (whitening by eigh,
conjugation, eigvalsh, autograd: oracle/reference_path.py).

    python tools/time_pairs_lds.py            # all legs
    python tools/time_pairs_lds.py --quick    # one repetition, for a profiler run
"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from oracle import reference_path  # noqa: E402
from sqfa_amd import _native  # noqa: E402


def statistics(C, m, dtype, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((C, 3 * m, m)).astype(np.float32)
    S = np.einsum("cnm,cnk->cmk", X, X, dtype=np.float64) / (3 * m) + 0.02 * np.eye(m)
    return torch.tensor(S, dtype=dtype, device="cuda")


def best_time(f, reps, warmup=1):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def native(C, m, dtype, reps):
    S = statistics(C, m, dtype)
    P = C * (C - 1) // 2
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    call = lambda: _native.hip_pair_backend(S, None, scale=1.0, eps=1e-6, sqrt_mode=True, weights=None,
                                            uniform_weight=-1.0 / P, shard=(0, 1), want_loss=True, want_grad=True,
                                            want_dist=False, want_eig=False)
    with _native.policies(sweep_counter=cnt):
        out = call()
        torch.cuda.synchronize()
    sweeps = cnt[0].item() / max(cnt[1].item(), 1)
    t = best_time(call, reps)
    return t, sweeps, out["loss"].item(), out["nonfinite"].tolist()


def reference(C, m, dtype, reps):
    S = statistics(C, m, dtype)
    f = lambda: reference_path.pairwise_loss_and_grad(S)
    t = best_time(f, reps)
    return t, f()[0].item()


def main():
    quick = "--quick" in sys.argv
    reps = 1 if quick else 5
    print(f"# {torch.cuda.get_device_name(0)}; times are the best of {reps} after one warm-up call", flush=True)
    for C, m in ((1000, 64), (1000, 65), (1000, 72)):
        t, sw, loss, fl = native(C, m, torch.float32, reps)
        print(f"native    C={C} m={m} float32: {t * 1e3:9.2f} ms  avg sweeps {sw:.2f}  loss {loss:.6f} flags {fl}",
              flush=True)
    for dtype in (torch.float32, torch.float64):
        for m in (65, 96, 128):
            t, sw, loss, fl = native(100, m, dtype, reps)
            name = str(dtype)[6:]
            print(f"native    C=100 m={m} {name}: {t * 1e3:9.2f} ms  avg sweeps {sw:.2f}  loss {loss:.6f} flags {fl}",
                  flush=True)
            tr, lr = reference(100, m, dtype, 1 if quick else 3)
            print(f"reference C=100 m={m} {name}: {tr * 1e3:9.2f} ms  loss {lr:.6f}  (native {tr / t:.1f}x faster)",
                  flush=True)


if __name__ == "__main__":
    main()
