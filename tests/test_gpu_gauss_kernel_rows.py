"""GPU tests of every row of the Gaussian pair kernels' dispatch (sqfa_amd/csrc/gauss_pair_kernel.hip), in its three
modes (plain: sqfa_gauss_pair_terms; pre-pass + fused: sqfa_gauss_pairwise_loss), against the float64 oracle of
tests/gauss_oracle.py (pinned to the reference's recorded outputs by tests/test_gauss_oracle.py).

    m                          kernel                                   variants
    1..4, 5..8, 9..12, 13..16  gauss_pair_reg_kernel<T, M=4/8/12/16>    EXACT (m == M and 16-byte aligned covariances: vector
                               (one pair per lane, 64 pairs per wave,   row loads) or padded (identity padding by selects,
                               256 per round)                           scalar loads)
    17..32, 33..64             gauss_pair_kernel<T, G=32/64>            ng lane groups per workgroup, from an LDS budget,
                               (LDS, G lanes per pair)                  reduced to a power of two >= nB when nB < ng

Which K reaches which instantiation here (both dtypes each):
    K = 5, 7         M=8 padded             K = 8    M=8 EXACT   (K = 8 unaligned: M=8 padded)
    K = 9, 10, 11    M=12 padded            K = 12   M=12 EXACT  (K = 12 unaligned: M=12 padded)
    K = 13, 15       M=16 padded            K = 16 unaligned: M=16 padded
    K = 17, 18, 24, 31, 32   G=32 (32: no idle lane)
    K = 34, 40, 48, 63, 64   G=64 (64: no idle lane)
    K = 5 / 10 / 15 at n = 142 (n*n >= 20000): padded by the HOST (_native) to 8 / 12 / 16, so M=8 / 12 / 16 EXACT with
    identity-padded data and gradients sliced back; at n = 141 the kernel pads.

Tolerances (the rule of tests/test_gpu_gauss_closure.py, no new constant): float64 kernel against the float64 oracle
1e-9 (values) / 1e-8 (gradients; Hellinger gradients 1e-6).  float32: max(1e-5, 5 x dev) with dev = rel_err(the oracle
expression evaluated in float32 torch, the same in float64), measured here per quantity on the same float32-rounded
inputs: the reference's own float32 deviation, never anything the kernel returned.  The float64 side always sees the
dtype-rounded inputs.  Two native calls that must agree "to rounding" (aligned against unaligned covariances) are held
to the same bounds as each of them against the oracle.

Inputs: gauss_oracle.inputs(C, K, seed = 1000 C + K), built on the CPU; the oracle runs on the CPU and every
reference is computed once per (shape, kind, dtype) and shared."""
import functools

import pytest
import torch

import gauss_oracle
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = gauss_oracle.EPS
KINDS = {0: "bhattacharyya", 1: "hellinger", 2: "mahalanobis_sq", 3: "mahalanobis"}
DTYPES = [torch.float64, torch.float32]
QUANTITIES = ("loss", "gmu", "gcov", "D")   # the order gauss_oracle._full_expression returns them in


def _weight(C):
    return -1.0 / (C * (C - 1) // 2)


@functools.lru_cache(maxsize=None)
def _stats(C, K, dtype):
    """dtype-rounded means and covariances of the case (C, K), on the CPU."""
    mu, cov = gauss_oracle.inputs(C, K, 1000 * C + K)
    return mu.to(dtype), cov.to(dtype)


def _deviation(evaluate, dtype):
    """(float64 reference, float32 deviation of the oracle per quantity or None) of evaluate(dtype) -> tuple of tensors."""
    ref = evaluate(torch.float64)
    if dtype == torch.float64:
        return ref, None
    return ref, tuple(rel_err(lo, hi) for lo, hi in zip(evaluate(torch.float32), ref))


@functools.lru_cache(maxsize=None)
def _fused_reference(C, K, kind, dtype):
    mu, cov = _stats(C, K, dtype)
    ref, dev = _deviation(lambda dt: gauss_oracle._full_expression(mu, cov, kind, _weight(C), dtype=dt), dtype)
    return dict(zip(QUANTITIES, ref)), (dict(zip(QUANTITIES, dev)) if dev is not None else None)


def _tol(dtype, dev, what, gradient, kind=None):
    if dtype == torch.float64:
        return (1e-6 if kind == 1 else 1e-8) if gradient else 1e-9
    return max(1e-5, 5 * dev[what])


def _native_fused(mu, cov, kind, weight, want_grad=True, want_dist=True):
    from sqfa_amd import _native
    out = _native.hip_gauss_pairwise_loss(mu, cov, kind, EPS, weight, want_grad=want_grad, want_dist=want_dist)
    torch.cuda.synchronize()
    return out


def _check_fused(C, K, kind, dtype, label, cov_dev=None):
    """The fused entry on the case (C, K) against the oracle: loss, dist (both triangles), gmu, gcov, flags, symmetry,
    diagonal, forward-only call, repeatability.  Returns the native outputs."""
    ref, dev = _fused_reference(C, K, kind, dtype)
    if kind == 1:   # a condition on the inputs: a saturated Hellinger distance has no gradient left to check
        off = ~torch.eye(C, dtype=torch.bool)
        assert ref["D"][off].max().item() < 0.99
    mu, cov = _stats(C, K, dtype)
    mu = mu.to(DEV)
    cov = cov.to(DEV) if cov_dev is None else cov_dev
    out = _native_fused(mu, cov, kind, _weight(C))
    assert out["nonfinite"].tolist() == [0, 0]
    assert out["gmu"].shape == (C, K) and out["gcov"].shape == (C, K, K) and out["dist"].shape == (C, C)
    assert out["gmu"].is_contiguous() and out["gcov"].is_contiguous()
    errs = {"loss": rel_err(out["loss"].cpu(), ref["loss"]), "D": rel_err(out["dist"].cpu(), ref["D"]),
            "gmu": rel_err(out["gmu"].cpu(), ref["gmu"]), "gcov": rel_err(out["gcov"].cpu(), ref["gcov"])}
    print(f"gauss-rows {label} C={C} K={K} {KINDS[kind]} {str(dtype)[6:]}", {k: f"{v:.2e}" for k, v in errs.items()},
          "dev", {k: f"{v:.2e}" for k, v in dev.items()} if dev else None)
    assert errs["loss"] <= _tol(dtype, dev, "loss", False)
    assert errs["D"] <= _tol(dtype, dev, "D", False)
    assert errs["gmu"] <= _tol(dtype, dev, "gmu", True, kind)
    assert errs["gcov"] <= _tol(dtype, dev, "gcov", True, kind)
    assert torch.equal(out["gcov"], out["gcov"].transpose(1, 2))         # full symmetric matrices, bitwise
    diag = out["dist"].diagonal()
    if kind in (0, 2):
        assert torch.equal(diag, torch.zeros_like(diag))
    else:
        assert torch.allclose(diag, torch.full_like(diag, EPS ** 0.5), rtol=1e-6, atol=0)
    fwd = _native_fused(mu, cov, kind, _weight(C), want_grad=False, want_dist=False)
    assert torch.equal(fwd["loss"], out["loss"]) and fwd["gmu"] is None and fwd["gcov"] is None and fwd["dist"] is None
    assert fwd["nonfinite"].tolist() == [0, 0]
    again = _native_fused(mu, cov, kind, _weight(C))
    for name in ("loss", "gmu", "gcov", "dist"):
        assert torch.equal(again[name], out[name]), name
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. fused entry, every row
ROW_CASES = [(9, K) for K in (5, 7, 8, 9, 11, 12, 13, 15)] + [(7, K) for K in (18, 24, 31, 32, 34, 48, 63, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("C,K", ROW_CASES)
def test_fused_rows(C, K, kind, dtype):
    _check_fused(C, K, kind, dtype, "rows")


# ---------------------------------------------------------------------------------------------------------------------
# b. class-count edges: wave (64) and round (256) boundaries of the register kernels, fewer classes than lane groups and
# many passes per group on the LDS kernels.  Kind 0 needs the pre-pass and Sbar^-1, kind 3 neither.
COUNT_CASES = ([(n, 8) for n in (2, 3, 63, 64, 65, 255, 256, 257)] + [(n, 7) for n in (2, 65, 257)]
               + [(n, 17) for n in (2, 3, 5, 257)] + [(n, 32) for n in (2, 3)] + [(n, 40) for n in (2, 3)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("n,K", COUNT_CASES)
def test_fused_class_counts(n, K, kind, dtype):
    _check_fused(n, K, kind, dtype, "counts")


# ---------------------------------------------------------------------------------------------------------------------
# plain path: Q, LD and the gradient of sum(WQ * Q) + sum(WLD * LD)

def _plain_reference(muA, covA, muB, covB, WQ, WLD, dtype):
    """Oracle of the plain path on CPU tensors of `dtype`; B None: the self case (one shared batch).  Returns
    ((Q, LD, gmuA, gcovA[, gmuB, gcovB]) in float64, the float32 deviation of each or None)."""
    def evaluate(dt):
        leaves = [t.detach().to(dt).requires_grad_(True) for t in ((muA, covA) if muB is None else (muA, covA, muB, covB))]
        Q, LD = gauss_oracle.pair_terms(*(leaves if muB is not None else leaves + leaves), dtype=dt)
        loss = sum((W.to(dt) * T).sum() for W, T in ((WQ, Q), (WLD, LD)) if W is not None)
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        return (Q.detach(), LD.detach()) + tuple(torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves))
    return _deviation(evaluate, dtype)


def _plain_tol(dtype, dev, idx):
    if dtype == torch.float64:
        return 1e-9 if idx < 2 else 1e-8
    return max(1e-5, 5 * dev[idx])


def _check_plain_self(C, K, dtype, label, cov_dev=None):
    """_native.GaussPairTerms in the self case with non-symmetric upstream weights, against autograd of the oracle."""
    from sqfa_amd import _native
    mu, cov = _stats(C, K, dtype)
    g = torch.Generator().manual_seed(7000 * C + K)
    WQ = torch.randn(C, C, generator=g, dtype=torch.float64).to(dtype)
    WLD = torch.randn(C, C, generator=g, dtype=torch.float64).to(dtype)
    ref, dev = _plain_reference(mu, cov, None, None, WQ, WLD, dtype)
    mu_d = mu.to(DEV).requires_grad_(True)
    cov_d = (cov.to(DEV) if cov_dev is None else cov_dev).requires_grad_(True)
    Q, LD = _native.GaussPairTerms.apply(mu_d, cov_d, mu_d, cov_d, True)
    gmu, gcov = torch.autograd.grad((WQ.to(DEV) * Q).sum() + (WLD.to(DEV) * LD).sum(), (mu_d, cov_d))
    torch.cuda.synchronize()
    assert gmu.shape == (C, K) and gcov.shape == (C, K, K) and gmu.is_contiguous() and gcov.is_contiguous()
    got = (Q.detach(), LD.detach(), gmu, gcov)
    errs = [rel_err(a.cpu(), b) for a, b in zip(got, ref)]
    print(f"gauss-rows {label} plain C={C} K={K} {str(dtype)[6:]}", dict(zip(("Q", "LD", "gmu", "gcov"), (f"{e:.2e}" for e in errs))),
          "dev", [f"{v:.2e}" for v in dev] if dev else None)
    for idx, e in enumerate(errs):
        assert e <= _plain_tol(dtype, dev, idx), ("Q", "LD", "gmu", "gcov")[idx]
    assert torch.equal(gcov, gcov.transpose(1, 2))
    return got, dev


# ---------------------------------------------------------------------------------------------------------------------
# c. host padding threshold: n*n = 19881 (the kernel pads) and 20164 (the host pads to 8 / 12 / 16 and slices back)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("K", [5, 10, 15])
@pytest.mark.parametrize("n", [141, 142])
def test_host_padding_threshold(n, K, kind, dtype, monkeypatch):
    from sqfa_amd import _native
    padded_to = []
    pad = _native._pad_gauss

    def spy(mu, cov, M):
        padded_to.append(M)
        return pad(mu, cov, M)

    monkeypatch.setattr(_native, "_pad_gauss", spy)
    _check_fused(n, K, kind, dtype, "padding")
    # each is compared with its own oracle; which side of the threshold pads is part of what is checked
    assert set(padded_to) == (set() if n == 141 else {(K + 3) // 4 * 4})
    if kind == 0:   # the plain path has no kinds: once per (n, K, dtype)
        _check_plain_self(n, K, dtype, "padding")


# ---------------------------------------------------------------------------------------------------------------------
# d. covariances that are not 16-byte aligned: the launcher falls back from EXACT (vector row loads) to the padded variant
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 12, 16])
def test_unaligned_covariances(K, dtype):
    C = 9
    mu, cov = _stats(C, K, dtype)
    aligned = cov.to(DEV)
    buf = torch.empty(C * K * K + 1, dtype=dtype, device=DEV)
    shifted = buf[1:].view(C, K, K)
    shifted.copy_(aligned)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0 and aligned.data_ptr() % 16 == 0
    _, dev = _fused_reference(C, K, 0, dtype)
    out_a = _check_fused(C, K, 0, dtype, "aligned")
    out_u = _check_fused(C, K, 0, dtype, "unaligned", cov_dev=shifted)
    assert rel_err(out_u["loss"].cpu(), out_a["loss"].cpu()) <= _tol(dtype, dev, "loss", False)
    assert rel_err(out_u["dist"].cpu(), out_a["dist"].cpu()) <= _tol(dtype, dev, "D", False)
    assert rel_err(out_u["gmu"].cpu(), out_a["gmu"].cpu()) <= _tol(dtype, dev, "gmu", True, 0)
    assert rel_err(out_u["gcov"].cpu(), out_a["gcov"].cpu()) <= _tol(dtype, dev, "gcov", True, 0)
    got_a, pdev = _check_plain_self(C, K, dtype, "aligned")
    got_u, _ = _check_plain_self(C, K, dtype, "unaligned", cov_dev=shifted.detach())
    for idx, (u, a) in enumerate(zip(got_u, got_a)):
        assert rel_err(u.cpu(), a.cpu()) <= _plain_tol(dtype, pdev, idx), idx


# ---------------------------------------------------------------------------------------------------------------------
# e. plain entry, cross batches, every row: nB = 70 spans two waves of the register kernel, nB = 2 lies below ng on the
# LDS rows; the three upstream combinations; the B side through the swapped call GaussPairTerms.backward makes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nA,nB", [(3, 70), (7, 2), (66, 5)])
@pytest.mark.parametrize("K", [5, 9, 12, 13, 24, 32, 48, 64])
def test_plain_rows_cross(K, nA, nB, dtype):
    from sqfa_amd import _native
    mu, cov = _stats(nA + nB, K, dtype)
    muA, covA, muB, covB = mu[:nA], cov[:nA], mu[nA:], cov[nA:]
    g = torch.Generator().manual_seed(9000 * nA + 100 * nB + K)
    WQ = torch.randn(nA, nB, generator=g, dtype=torch.float64).to(dtype)
    WLD = torch.randn(nA, nB, generator=g, dtype=torch.float64).to(dtype)
    dA, dcA, dB, dcB = (t.to(DEV) for t in (muA, covA, muB, covB))
    Q, LD, none_mu, none_cov = _native.hip_gauss_terms(dA, dcA, dB, dcB)
    assert none_mu is None and none_cov is None and Q.shape == LD.shape == (nA, nB)
    for label, wq, wld in (("gQ+gLD", WQ, WLD), ("gQ", WQ, None), ("gLD", None, WLD)):
        ref, dev = _plain_reference(muA, covA, muB, covB, wq, wld, dtype)
        gq = wq.to(DEV) if wq is not None else None
        gld = wld.to(DEV) if wld is not None else None
        no_Q, no_LD, gmuA, gcovA = _native.hip_gauss_terms(dA, dcA, dB, dcB, gq, gld, want_outputs=False, want_grad=True)
        _, _, gmuB, gcovB = _native.hip_gauss_terms(dB, dcB, dA, dcA, gq.t() if gq is not None else None,
                                                    gld.t() if gld is not None else None, want_outputs=False, want_grad=True)
        torch.cuda.synchronize()
        assert no_Q is None and no_LD is None
        assert gmuA.shape == (nA, K) and gcovA.shape == (nA, K, K) and gmuB.shape == (nB, K) and gcovB.shape == (nB, K, K)
        got = (Q, LD, gmuA, gcovA, gmuB, gcovB)
        names = ("Q", "LD", "gmuA", "gcovA", "gmuB", "gcovB")
        errs = [rel_err(a.cpu(), b) for a, b in zip(got, ref)]
        print(f"gauss-rows cross K={K} nA={nA} nB={nB} {label} {str(dtype)[6:]}", dict(zip(names, (f"{e:.2e}" for e in errs))),
              "dev", [f"{v:.2e}" for v in dev] if dev else None)
        for idx, e in enumerate(errs):
            assert e <= _plain_tol(dtype, dev, idx), (label, names[idx])
        assert torch.equal(gcovA, gcovA.transpose(1, 2)) and torch.equal(gcovB, gcovB.transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# f. a class that is not positive definite, on the rows no other test reaches: "yields NaN and is counted, never a fault"
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("K", [12, 24, 64])
def test_non_spd_class_rows(K, kind, dtype):
    C = 6
    P = C * (C - 1) // 2
    mu, cov = _stats(C, K, dtype)
    bad = cov.clone()
    bad[3] = -4.0 * bad[3]
    out = _native_fused(mu.to(DEV), bad.to(DEV), kind, _weight(C))
    n_nan, n_inf = out["nonfinite"].tolist()
    assert n_nan >= 1 and n_nan + n_inf <= P
    assert torch.isnan(out["loss"])
    _check_fused(C, K, kind, dtype, "after-non-spd")
