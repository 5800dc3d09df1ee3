"""One SHA-256 per output tensor of the Gaussian class factors, scores, log-loss and log-loss backward, through the C ABI of
the library that SQFA_HIP_LIBRARY selects (default: this tree's), on seeded inputs generated on the CPU.  A change that must
leave every bit alone is checked by the diff of two runs, each a process of its own:

    SQFA_HIP_LIBRARY=/path/to/other/libsqfa_hip.so python tools/ab_classify_bits.py > a.txt && \\
    python tools/ab_classify_bits.py > b.txt && diff a.txt b.txt

Cases: float32 and float64, with and without means, uniform priors and given priors that include a zero, and shapes that take
every KB = ceil(K / 16), both staging variants (4 classes per stage up to K = 32, one above), split and unsplit classes and
samples, one 16-sample tile and several per wave, and a partial workgroup.
"""
import ctypes
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sqfa_amd import _lib, _native  # noqa: E402

SHAPES = [(1, 1, 1), (3, 3, 17), (17, 4, 257), (37, 16, 1000), (37, 17, 1000), (9, 33, 300), (4, 48, 100), (5, 64, 200),
          (300, 16, 2000), (5, 3, 65537)]   # (C, K, N)
DEV = "cuda:0"
TALLY = {"tensors": 0, "nan": 0}


def report(case, name, t):
    a = t.detach().cpu().contiguous().numpy()
    TALLY["tensors"] += 1
    TALLY["nan"] += int(a.dtype.kind == "f" and bool(np.isnan(a).any()))
    print(f"{case} {name} {tuple(a.shape)} {a.dtype} {hashlib.sha256(a.tobytes()).hexdigest()}")


def inputs(C, K, N, dtype, means, priors, seed):
    """Class Gaussians with condition numbers up to ~100, samples drawn around their class means: all on the CPU in float64,
    rounded once to the dtype."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((C, K, 2 * K + 2))
    cov = np.einsum("cka,cla->ckl", A, A) / (2 * K + 2) * rng.uniform(0.5, 2.0, (C, 1, 1)) + 0.05 * np.eye(K)
    mu = 1.5 * rng.standard_normal((C, K)) if means else None
    labels = rng.integers(0, max(1, C - 1) if priors else C, N)   # given priors: the last class has prior 0 and no label
    Z = np.einsum("nkl,nl->nk", np.linalg.cholesky(cov)[labels], rng.standard_normal((N, K)))
    if means:
        Z = Z + mu[labels]
    log_priors = None
    if priors:
        w = rng.uniform(0.2, 1.0, C)
        if C > 1:
            w[C - 1] = 0.0
        with np.errstate(divide="ignore"):
            log_priors = torch.tensor(np.log(w / w.sum()), dtype=torch.float64, device=DEV)
    to = lambda a: None if a is None else torch.tensor(a, dtype=dtype, device=DEV).contiguous()
    return to(Z), torch.tensor(labels, dtype=torch.int64, device=DEV), to(mu), to(cov), log_priors


def workspace(query, *args):
    nbytes = query(*args)
    assert nbytes > 0, query.__name__
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV), nbytes   # whatever is read before it is written is NaN


def run_case(lib, C, K, N, dtype, means, priors, seed):
    case = f"C{C}-K{K}-N{N}-{'f32' if dtype == torch.float32 else 'f64'}-{'means' if means else 'zeromean'}-" \
           f"{'priors' if priors else 'uniform'}"
    Z, y, mu, cov, lp = inputs(C, K, N, dtype, means, priors, seed)
    code, P = _native._dtype_code(Z), _native._ptr
    new = lambda *shape, dt=dtype: torch.empty(shape, dtype=dt, device=DEV)
    with _native._on_stream(Z.device) as stream:
        W, offset, bad = new(C, K, K), new(C, dt=torch.float64), new(1, dt=torch.int32)
        _lib.check(lib.sqfa_gauss_class_factors(P(mu), P(cov), P(lp), C, K, code, P(W), P(offset), P(bad), stream), "factors")
        for name, t in (("W", W), ("offsets", offset), ("bad", bad)):
            report(case, "factors." + name, t)

        ws, nbytes = workspace(lib.sqfa_gauss_scores_workspace_bytes, N, C, K, code)
        S, A, B, E, cnt = new(N, C), new(N, dt=torch.int64), new(N), new(N), new(1, dt=torch.int32)
        _lib.check(lib.sqfa_gauss_scores(P(Z), N, P(mu), P(W), P(offset), C, K, code, P(S), P(A), P(B), P(E), P(cnt), P(ws),
                                         nbytes, stream), "scores")
        for name, t in (("scores", S), ("argmax", A), ("best", B), ("logsumexp", E), ("counter", cnt)):
            report(case, "scores." + name, t)

        ws, nbytes = workspace(lib.sqfa_gauss_log_loss_workspace_bytes, N, C, K, code)
        loss, ll, lse, flags = new(1), new(N), new(N), new(3, dt=torch.int32)
        _lib.check(lib.sqfa_gauss_log_loss(P(Z), P(y), N, P(mu), P(W), P(offset), C, K, code, P(loss), P(ll), P(lse), P(flags),
                                           P(ws), nbytes, stream), "log_loss")
        for name, t in (("loss", loss), ("label_log_proba", ll), ("logsumexp", lse), ("flags", flags)):
            report(case, "log_loss." + name, t)

        up = torch.tensor([0.7], dtype=dtype, device=DEV)
        wanted = ("Z", "means", "cov") if means else ("Z", "cov")
        for subset in [wanted] + [(g,) for g in wanted]:
            ws, nbytes = workspace(lib.sqfa_gauss_log_loss_backward_workspace_bytes, N, C, K, code)
            g = {"Z": new(N, K) if "Z" in subset else None, "means": new(C, K) if "means" in subset else None,
                 "cov": new(C, K, K) if "cov" in subset else None}
            _lib.check(lib.sqfa_gauss_log_loss_backward(P(Z), P(y), N, P(mu), P(W), P(offset), C, K, code, P(lse), P(up),
                                                        P(g["Z"]), P(g["means"]), P(g["cov"]), P(ws), nbytes, stream),
                       "backward")
            for name in subset:
                report(case, f"backward[{'+'.join(subset)}].grad_{name}", g[name])
    torch.cuda.synchronize()


if __name__ == "__main__":
    library = _lib.load()
    cases = itertools.product(SHAPES, (torch.float32, torch.float64), (True, False), (False, True))
    for seed, ((C, K, N), dtype, means, priors) in enumerate(cases):
        run_case(library, C, K, N, dtype, means, priors, seed)
    print(f"# tensors {TALLY['tensors']}, holding a NaN {TALLY['nan']}")
