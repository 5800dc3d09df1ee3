"""Every host-side decision of the pairwise C ABI as a text table: tilings, workspace sizes, and the return code and
message of each argument rejection -- the affine-invariant, Bures-Wasserstein and SPD-function entry points, the four fused
class-pair losses (Gaussian, log-Euclidean, Jeffreys, Stein), the Gaussian class factors and scores, the Gaussian log-loss
and its backward (both workspace queries, sqfa_gauss_log_loss_layout, the rejections).  Needs no GPU (without
one the library assumes 256 CUs, the MI355X's count; every call below is rejected before it launches anything).  The check is
the diff of two runs:

    SQFA_HIP_LIBRARY=/path/to/other/libsqfa_hip.so python tools/host_decisions.py > a.txt
    python tools/host_decisions.py > b.txt && diff a.txt b.txt
"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sqfa_amd import _lib  # noqa: E402

NA = (2, 7, 30, 100, 300, 1000)
NB = (0, 7, 1000)
M = (1, 4, 5, 8, 12, 16, 17, 20, 24, 32, 33, 40, 48, 64, 65, 96, 128, 129)
SHARDS = (1, 2, 8)
POLICIES = (-1, 0, 1)


def sizes(lib):
    for nA, nB, m, dtype in itertools.product(NA, NB, M, (_lib.SQFA_F32, _lib.SQFA_F64)):
        out = [ctypes.c_int(-1) for _ in range(5)]
        rc = lib.sqfa_airm_tiling(nA, nB, m, dtype, *[ctypes.byref(v) for v in out])
        print(f"nA={nA} nB={nB} m={m} dtype={dtype}: tiling rc={rc} {[v.value for v in out]}"
              f" airm_ws={lib.sqfa_airm_workspace_bytes(nA, nB, m, dtype)} bw_ws={lib.sqfa_bw_workspace_bytes(nA, nB, m, dtype)}")
        for shards, policy in itertools.product(SHARDS, POLICIES):
            print(f"  shards={shards} policy={policy}:"
                  f" airm_ws={lib.sqfa_airm_workspace_bytes_sharded(nA, nB, m, dtype, shards, policy)}"
                  f" bw_ws={lib.sqfa_bw_workspace_bytes_sharded(nA, nB, m, dtype, shards, policy)}")
    for n, m, dtype in itertools.product(NA, M, (_lib.SQFA_F32, _lib.SQFA_F64)):
        print(f"spd n={n} m={m} dtype={dtype}: ws={lib.sqfa_spd_function_workspace_bytes(n, m, dtype)}")


def rejections(lib):
    """Host memory stands in for the device pointers: a rejected call never touches them."""
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    opts = _lib.AirmOptions(0, 0, None, 0)

    # name -> (A, nA, B, nB, m, dtype, shard_index, shard_count, workspace, workspace_bytes)
    def case(A=ptr, nA=30, B=None, nB=0, m=16, dtype=_lib.SQFA_F32, shard=(0, 1), ws=ptr, ws_bytes=1 << 40):
        return A, nA, B, nB, m, dtype, shard[0], shard[1], ws, ws_bytes

    cases = {
        "null A": case(A=None),
        "null workspace": case(ws=None),
        "bad dtype": case(dtype=7),
        "B without nB": case(B=ptr, nB=0),
        "nB without B": case(B=None, nB=7),
        "shard index": case(shard=(2, 2)),
        "shard count": case(shard=(0, 0)),
        "self mode, one class": case(nA=1),
        "m=129": case(m=129),
    }
    for m, dtype, nB in itertools.product((16, 40, 96), (_lib.SQFA_F32, _lib.SQFA_F64), (0, 7)):
        cases[f"airm workspace one byte short m={m} dtype={dtype} nB={nB}"] = case(
            m=m, dtype=dtype, B=ptr if nB else None, nB=nB, ws_bytes=lib.sqfa_airm_workspace_bytes_sharded(30, nB, m, dtype, 1, 0) - 1)
        cases[f"bw workspace one byte short m={m} dtype={dtype} nB={nB}"] = case(
            m=m, dtype=dtype, B=ptr if nB else None, nB=nB, ws_bytes=lib.sqfa_bw_workspace_bytes_sharded(30, nB, m, dtype, 1, 0) - 1)

    def report(fn, name, rc):
        print(f"{fn} [{name}]: rc={rc} error={lib.sqfa_hip_last_error().decode()!r}")

    for name, (A, nA, B, nB, m, dtype, si, sc, ws, nbytes) in cases.items():
        if not name.startswith("bw workspace"):
            args = (A, nA, B, nB, m, dtype, 1.0, 1e-6, 1, None, 1.0, si, sc, ptr, ptr, None, None, None, None, ws, nbytes, None)
            report("sqfa_airm_pairwise", name, lib.sqfa_airm_pairwise(*args))
            report("sqfa_airm_pairwise_opt", name, lib.sqfa_airm_pairwise_opt(*args, ctypes.byref(opts)))
            if sc == 1:  # the eigenvalue backward takes no shard
                report("sqfa_airm_eigenvalues_backward", name,
                       lib.sqfa_airm_eigenvalues_backward(A, nA, B, nB, m, dtype, ptr, ptr, None, ws, nbytes, None, None))
        if not name.startswith("airm workspace"):
            report("sqfa_bw_pairwise", name,
                   lib.sqfa_bw_pairwise(A, nA, B, nB, m, dtype, 1e-6, 1, None, 1.0, si, sc, ptr, ptr, None, None, None, ws, nbytes,
                                        None, None))
    report("sqfa_airm_eigenvalues_backward", "null eig_weights",
           lib.sqfa_airm_eigenvalues_backward(ptr, 30, None, 0, 16, 0, None, ptr, None, ptr, 1 << 40, None, None))

    def spd(S=ptr, n=30, m=16, dtype=_lib.SQFA_F32, kind=0, U=ptr, ws=ptr, ws_bytes=1 << 40):
        return lib.sqfa_spd_function(S, n, m, dtype, kind, None, U, ptr, ws, ws_bytes, None)

    report("sqfa_spd_function", "null S", spd(S=None))
    report("sqfa_spd_function", "null workspace", spd(ws=None))
    report("sqfa_spd_function", "bad dtype", spd(dtype=7))
    report("sqfa_spd_function", "bad kind", spd(kind=9))
    report("sqfa_spd_function", "m=65", spd(m=65))
    report("sqfa_spd_function", "m=129", spd(m=129))
    for m, dtype in itertools.product((16, 40, 64), (_lib.SQFA_F32, _lib.SQFA_F64)):
        report("sqfa_spd_function", f"workspace one byte short m={m} dtype={dtype}",
               spd(m=m, dtype=dtype, ws_bytes=lib.sqfa_spd_function_workspace_bytes(30, m, dtype) - 1))
    report("sqfa_spd_function_backward", "m=65", lib.sqfa_spd_function_backward(ptr, ptr, ptr, 30, 65, 0, 0, ptr, None))


CP_N = (1, 2, 1000)
CP_M = (1, 16, 17, 32, 33, 64, 65)
CP_QUERIES = ("sqfa_gauss_pairwise_workspace_bytes", "sqfa_log_euclidean_workspace_bytes", "sqfa_jeffreys_workspace_bytes",
              "sqfa_stein_workspace_bytes")


def class_pair_sizes(lib):
    for n, m, dtype in itertools.product(CP_N, CP_M, (_lib.SQFA_F32, _lib.SQFA_F64, 7)):
        print(f"class pairs n={n} m={m} dtype={dtype}: " + " ".join(f"{q}={getattr(lib, q)(n, m, dtype)}" for q in CP_QUERIES))
    for N, C, K, dtype in itertools.product((0, 1, 64, 1000, 100000, 1 << 40), (0, 1, 3, 37, 1000), (0, 1, 16, 17, 64, 65),
                                            (_lib.SQFA_F32, _lib.SQFA_F64, 7)):
        print(f"scores N={N} C={C} K={K} dtype={dtype}: ws={lib.sqfa_gauss_scores_workspace_bytes(N, C, K, dtype)}")


def class_pair_rejections(lib):
    """The four fused class-pair losses, the class factors and the class scores: every call is rejected before a launch."""
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    BIG = 1 << 40

    def report(fn, name, rc):
        print(f"{fn} [{name}]: rc={rc} error={lib.sqfa_hip_last_error().decode()!r}")

    # one caller per entry point over the same keywords; `mode` is sqrt_mode, or the Gaussian kind
    def stein(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_stein_pairwise_loss(S, n, m, dtype, mode, 1e-6, None, 1.0, ptr, gcov, None, None, ws, nbytes, None)

    def jeffreys(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_jeffreys_pairwise_loss(mu, S, n, m, dtype, mode, 1e-6, None, 1.0, ptr, gmu, gcov, None, None, ws, nbytes, None)

    def log_euclidean(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_log_euclidean_pairwise_loss(S, n, m, dtype, mode, 1e-6, 1.0, ptr, gcov, None, None, ws, nbytes, None)

    def log_euclidean_w(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_log_euclidean_pairwise_loss_weighted(S, n, m, dtype, mode, 1e-6, ptr, 1.0, ptr, gcov, None, None, ws, nbytes, None)

    def gauss(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_gauss_pairwise_loss(mu, S, n, m, dtype, mode, 1e-6, 1.0, ptr, gmu, gcov, None, None, ws, nbytes, None)

    def gauss_w(S=ptr, mu=ptr, n=7, m=16, dtype=0, mode=1, gmu=None, gcov=None, ws=ptr, nbytes=BIG):
        return lib.sqfa_gauss_pairwise_loss_weighted(mu, S, n, m, dtype, mode, 1e-6, ptr, 1.0, ptr, gmu, gcov, None, None, ws, nbytes, None)

    entries = {
        "sqfa_stein_pairwise_loss": (stein, "sqfa_stein_workspace_bytes"),
        "sqfa_jeffreys_pairwise_loss": (jeffreys, "sqfa_jeffreys_workspace_bytes"),
        "sqfa_log_euclidean_pairwise_loss": (log_euclidean, "sqfa_log_euclidean_workspace_bytes"),
        "sqfa_log_euclidean_pairwise_loss_weighted": (log_euclidean_w, "sqfa_log_euclidean_workspace_bytes"),
        "sqfa_gauss_pairwise_loss": (gauss, "sqfa_gauss_pairwise_workspace_bytes"),
        "sqfa_gauss_pairwise_loss_weighted": (gauss_w, "sqfa_gauss_pairwise_workspace_bytes"),
    }
    # single faults, then several at once: the later ones show the order of the checks (a case that some entry point has
    # nothing against also has a null workspace)
    cases = {
        "null matrices": dict(S=None),
        "null means": dict(mu=None, ws=None),
        "n=1": dict(n=1),
        "m=0": dict(m=0),
        "bad dtype": dict(dtype=7),
        "mode=2": dict(mode=2, ws=None),
        "mode=9": dict(mode=9),
        "mode=-1": dict(mode=-1),
        "gmu without gcov": dict(gmu=ptr, ws=None),
        "gcov without gmu": dict(gcov=ptr, ws=None),
        "gmu without means": dict(mu=None, gmu=ptr, gcov=ptr, ws=None),
        "m=65": dict(m=65),
        "null workspace": dict(ws=None),
        "no bytes": dict(nbytes=0),
        "null matrices, bad dtype": dict(S=None, dtype=7),
        "bad dtype, mode=9": dict(dtype=7, mode=9),
        "mode=9, gmu without gcov": dict(mode=9, gmu=ptr),
        "gmu without gcov, m=65": dict(gmu=ptr, m=65),
        "m=65, null workspace": dict(m=65, ws=None),
        "bad dtype, m=65, null workspace": dict(dtype=7, m=65, ws=None),
    }
    for fn, (call, query) in entries.items():
        for name, kw in cases.items():
            report(fn, name, call(**kw))
        for n, m, dtype in itertools.product(CP_N, CP_M, (_lib.SQFA_F32, _lib.SQFA_F64)):
            need = getattr(lib, query)(n, m, dtype)
            report(fn, f"workspace one byte short n={n} m={m} dtype={dtype}", call(n=n, m=m, dtype=dtype, nbytes=max(need, 1) - 1))

    def factors(mu=ptr, cov=ptr, C=3, K=16, dtype=0, W=ptr, offset=ptr, bad=ptr):
        return lib.sqfa_gauss_class_factors(mu, cov, None, C, K, dtype, W, offset, bad, None)

    for name, kw in {"null covariances": dict(cov=None), "null factors": dict(W=None), "null offsets": dict(offset=None),
                     "null counter": dict(bad=None), "C=0": dict(C=0), "K=0": dict(K=0), "bad dtype": dict(dtype=7),
                     "K=65": dict(K=65), "bad dtype, K=65": dict(dtype=7, K=65), "C=0, K=65": dict(C=0, K=65)}.items():
        report("sqfa_gauss_class_factors", name, factors(**kw))

    def scores(Z=ptr, N=17, W=ptr, offset=ptr, C=3, K=16, dtype=0, argmax=ptr, best=ptr, counter=ptr, ws=ptr, nbytes=BIG):
        return lib.sqfa_gauss_scores(Z, N, ptr, W, offset, C, K, dtype, None, argmax, best, None, counter, ws, nbytes, None)

    for name, kw in {"null samples": dict(Z=None), "null factors": dict(W=None), "null offsets": dict(offset=None),
                     "null counter": dict(counter=None), "N=0": dict(N=0), "C=0": dict(C=0), "K=0": dict(K=0),
                     "bad dtype": dict(dtype=7), "best without argmax": dict(argmax=None), "K=65": dict(K=65),
                     "too many tiles": dict(N=1 << 40), "too many classes": dict(C=(1 << 31) - 2),
                     "null workspace": dict(ws=None), "no bytes": dict(nbytes=0),
                     "bad dtype, best without argmax": dict(dtype=7, argmax=None),
                     "best without argmax, K=65": dict(argmax=None, K=65), "K=65, null workspace": dict(K=65, ws=None)}.items():
        report("sqfa_gauss_scores", name, scores(**kw))
    for N, C, K, dtype in itertools.product((17, 1000), (3, 37), (16, 64), (_lib.SQFA_F32, _lib.SQFA_F64)):
        need = lib.sqfa_gauss_scores_workspace_bytes(N, C, K, dtype)
        report("sqfa_gauss_scores", f"workspace one byte short N={N} C={C} K={K} dtype={dtype}",
               scores(N=N, C=C, K=K, dtype=dtype, nbytes=need - 1))


# (N, C, K) of the Gaussian log-loss: the SHAPES of tests/test_gpu_log_loss.py, the timing tools' large cases, and both
# sides of every split -- classes split (few sample tiles) and not, samples split and not, the slab bound (many classes,
# K = 64), the cap of 1024 sample splits (one class, many tiles), and sizes that are refused
LL_GRID = [(N, C, K) for C, K, N in ((1, 1, 1), (2, 1, 65), (3, 3, 17), (17, 4, 257), (37, 16, 1000), (37, 17, 1000),
                                     (130, 5, 513), (9, 33, 300), (5, 64, 200), (4, 48, 100), (300, 16, 2000), (5, 3, 65537))] + \
          [(60000, 1000, 16), (60000, 1000, 32), (60000, 1000, 64), (65536, 300, 16), (65537, 300, 16), (1000, 300, 16),
           (256, 5, 3), (257, 5, 3), (2000, 5, 3), (1000, 100000, 64), (10 ** 6, 10, 64), (10 ** 6, 1, 1), (10 ** 6, 1000, 16),
           (64 * 1023, 5, 3), (64 * 1024, 5, 3), (64 * 1024, 1000, 16), (64 * 63, 1000, 16), (64 * 64, 1000, 16),
           (64 * 64 + 1, 1000, 16), (64 * 70, 57, 16), (64 * 70, 61, 16), (0, 3, 3), (17, 0, 3), (17, 3, 0), (17, 3, 65),
           (1 << 40, 3, 3), (17, (1 << 31) - 2, 3)]


def log_loss_sizes(lib):
    for (N, C, K), dtype in itertools.product(LL_GRID, (_lib.SQFA_F32, _lib.SQFA_F64, 7)):
        out = [ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_longlong(-1)]
        rc = lib.sqfa_gauss_log_loss_layout(N, C, K, dtype, *[ctypes.byref(v) for v in out])
        print(f"log-loss N={N} C={C} K={K} dtype={dtype}: layout rc={rc} {[v.value for v in out]}"
              f" forward_ws={lib.sqfa_gauss_log_loss_workspace_bytes(N, C, K, dtype)}"
              f" backward_ws={lib.sqfa_gauss_log_loss_backward_workspace_bytes(N, C, K, dtype)}"
              f" scores_ws={lib.sqfa_gauss_scores_workspace_bytes(N, C, K, dtype)}")
    print(f"log-loss layout [null outputs]: rc={lib.sqfa_gauss_log_loss_layout(17, 3, 3, 0, None, None, None, None)}")


def log_loss_rejections(lib):
    """sqfa_gauss_log_loss and sqfa_gauss_log_loss_backward: every call is rejected before a launch."""
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    BIG = 1 << 40

    def report(fn, name, rc):
        print(f"{fn} [{name}]: rc={rc} error={lib.sqfa_hip_last_error().decode()!r}")

    def forward(Z=ptr, labels=ptr, N=17, mu=ptr, W=ptr, offset=ptr, C=3, K=16, dtype=0, loss=ptr, ll=None, lse=ptr, flags=ptr,
                ws=ptr, nbytes=BIG):
        return lib.sqfa_gauss_log_loss(Z, labels, N, mu, W, offset, C, K, dtype, loss, ll, lse, flags, ws, nbytes, None)

    def backward(Z=ptr, labels=ptr, N=17, mu=ptr, W=ptr, offset=ptr, C=3, K=16, dtype=0, lse=ptr, up=None, gZ=ptr, gmu=ptr,
                 gcov=ptr, ws=ptr, nbytes=BIG):
        return lib.sqfa_gauss_log_loss_backward(Z, labels, N, mu, W, offset, C, K, dtype, lse, up, gZ, gmu, gcov, ws, nbytes,
                                                None)

    # single faults, then several at once: the later ones show the order of the checks
    shared = {"null samples": dict(Z=None), "null labels": dict(labels=None), "null factors": dict(W=None),
              "null offsets": dict(offset=None), "null logsumexp": dict(lse=None), "N=0": dict(N=0), "N=-1": dict(N=-1),
              "C=0": dict(C=0), "K=0": dict(K=0), "bad dtype": dict(dtype=7), "K=65": dict(K=65), "K=128": dict(K=128),
              "too many tiles": dict(N=1 << 40), "too many classes": dict(C=(1 << 31) - 2), "null workspace": dict(ws=None),
              "no bytes": dict(nbytes=0), "null labels, bad dtype": dict(labels=None, dtype=7),
              "null labels, K=65": dict(labels=None, K=65), "bad dtype, K=65": dict(dtype=7, K=65),
              "K=65, null workspace": dict(K=65, ws=None), "K=65, no bytes": dict(K=65, nbytes=0),
              "too many tiles, null workspace": dict(N=1 << 40, ws=None),
              "bad dtype, K=65, null workspace": dict(dtype=7, K=65, ws=None)}
    only_forward = {"null loss": dict(loss=None), "null flags": dict(flags=None), "no means": dict(mu=None, ws=None),
                    "null loss, bad dtype": dict(loss=None, dtype=7)}
    only_backward = {"no gradient": dict(gZ=None, gmu=None, gcov=None), "grad_means without means": dict(mu=None),
                     "no means, no grad_means": dict(mu=None, gmu=None, ws=None), "upstream": dict(up=ptr, ws=None),
                     "bad dtype, no gradient": dict(dtype=7, gZ=None, gmu=None, gcov=None),
                     "no gradient, grad_means without means": dict(mu=None, gZ=None, gmu=None, gcov=None),
                     "no gradient, K=65": dict(gZ=None, gmu=None, gcov=None, K=65),
                     "grad_means without means, K=65": dict(mu=None, K=65),
                     "grad_means without means, null workspace": dict(mu=None, ws=None)}
    for fn, call, query, own in (("sqfa_gauss_log_loss", forward, lib.sqfa_gauss_log_loss_workspace_bytes, only_forward),
                                 ("sqfa_gauss_log_loss_backward", backward, lib.sqfa_gauss_log_loss_backward_workspace_bytes,
                                  only_backward)):
        for name, kw in {**shared, **own}.items():
            report(fn, name, call(**kw))
        for (N, C, K), dtype in itertools.product(LL_GRID, (_lib.SQFA_F32, _lib.SQFA_F64)):
            need = query(N, C, K, dtype)
            if need:
                report(fn, f"workspace one byte short N={N} C={C} K={K} dtype={dtype}",
                       call(N=N, C=C, K=K, dtype=dtype, nbytes=need - 1))


if __name__ == "__main__":
    library = _lib.load()
    print(f"# version {library.sqfa_hip_version()} arch {library.sqfa_hip_arch().decode()} max_dim {library.sqfa_hip_max_dim()}")
    sizes(library)
    rejections(library)
    class_pair_sizes(library)
    class_pair_rejections(library)
    log_loss_sizes(library)
    log_loss_rejections(library)
