"""Per-step GPU time of one pair evaluation under each launch policy (sqfa_airm_options::launch_policy), same library, same
process, the policies ALTERNATING so that clock drift hits both alike:
    python tools/time_launch_policy.py [C m [rounds [steps]]]          (default: the headline, C=1000 m=16, 6 rounds of 200 steps)
Prints, per policy (-1 separate launches, 0 fused), the ms per step of every round and their mean; HIP events around the steps.
profiles/pair_step_overhead.txt holds its output next to the bench.py headline runs of both builds."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sqfa_amd import _native  # noqa: E402


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    g = torch.Generator().manual_seed(0)
    X = torch.randn(C, 4 * m, m, generator=g)
    S = (torch.einsum("cnm,cnk->cmk", X, X) / (4 * m) + 0.05 * torch.eye(m)).to("cuda:0")
    P = C * (C - 1) // 2

    def step():
        return _native.hip_pair_backend(S, None, scale=1.0, eps=_native.EPSILON, sqrt_mode=True, weights=None,
                                        uniform_weight=-1.0 / P, shard=(0, 1), want_loss=True, want_grad=True,
                                        want_dist=False, want_eig=False)

    times = {-1: [], 0: []}
    for _ in range(300):   # the chip reaches its sustained clock
        step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for policy in (-1, 0):
            with _native.policies(launch=policy):
                for _ in range(20):
                    step()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    out = step()
                b.record()
                torch.cuda.synchronize()
                times[policy].append(a.elapsed_time(b) / steps)
    assert out["nonfinite"].tolist() == [0, 0]
    print(f"C={C} m={m}: {rounds} alternating rounds of {steps} steps, ms per step")
    for policy, name in ((-1, "separate launches (-1)"), (0, "fused launches (0)    ")):
        t = times[policy]
        print(f"  {name}: " + " ".join(f"{v:.4f}" for v in t) + f"   mean {sum(t) / len(t):.4f}  min {min(t):.4f}  max {max(t):.4f}")
    d = [x - y for x, y in zip(times[-1], times[0])]
    print(f"  separate - fused per round (us): " + " ".join(f"{1e3 * v:.1f}" for v in d) + f"   mean {1e3 * sum(d) / len(d):.1f}")


if __name__ == "__main__":
    main()
