"""GPU test of the single autograd node of the fused class-pair losses, _native.ClassPairLoss: for every family of
_native.PAIR_FAMILIES it returns the loss, the flags and the gradients of the family's hip_*_pairwise_loss call bit for bit,
its backward scales exactly those gradients by the upstream gradient, and an absent leading input (the means of the
means-free losses) gets None.

Sizes: n = 2, m = 1 (one pair, the smallest valid call) and n = 3, m = 5 (an odd size below every padding threshold).
No tolerance anywhere: both sides are the same native call on the same inputs, and the kernels are bitwise reproducible."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
SIZES = [(2, 1), (3, 5)]
DTYPES = [torch.float32, torch.float64]
# (family, with means): Jeffreys runs with and without
CASES = [("gauss", True), ("log_euclidean", False), ("jeffreys", True), ("jeffreys", False)]


def _modes(family):
    from sqfa_amd import _lib
    if family == "gauss":
        return [_lib.SQFA_GAUSS_BHATTACHARYYA, _lib.SQFA_GAUSS_HELLINGER, _lib.SQFA_GAUSS_MAHALANOBIS_SQ,
                _lib.SQFA_GAUSS_MAHALANOBIS]
    return [False, True]


def _direct_call(family, mu, cov, mode, weight, W):
    """The family's hip_*_pairwise_loss on the same inputs, as (loss, flags, gmu or None, gcov)."""
    from sqfa_amd import _native
    if family == "gauss":
        out = _native.hip_gauss_pairwise_loss(mu, cov, mode, EPS, weight, pair_weights=W)
    elif family == "log_euclidean":
        out = _native.hip_log_euclidean_pairwise_loss(cov, mode, EPS, weight, pair_weights=W)
        return out["loss"], out["nonfinite"], None, out["gS"]
    else:
        out = _native.hip_jeffreys_pairwise_loss(mu, cov, mode, EPS, weight, pair_weights=W)
    return out["loss"], out["nonfinite"], out["gmu"], out["gcov"]


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,m", SIZES)
@pytest.mark.parametrize("family,means", CASES, ids=[f"{f}-{'means' if mm else 'nomeans'}" for f, mm in CASES])
def test_node_equals_the_native_call(family, means, n, m, dtype, weighted):
    from sqfa_amd import _native
    g = torch.Generator().manual_seed(100 * n + m)
    A = torch.randn(n, m, m + 2, generator=g, dtype=torch.float64)
    cov = (A @ A.transpose(1, 2) / (m + 2) + 0.1 * torch.eye(m, dtype=torch.float64)).to(dtype).to(DEV)
    mu = (0.3 * torch.randn(n, m, generator=g, dtype=torch.float64)).to(dtype).to(DEV) if means else None
    W = None
    if weighted:
        raw = torch.rand(n, n, generator=g, dtype=torch.float64) + 0.1
        W = _native.normalized_pair_weights(raw + raw.t(), n, dtype, DEV)
    weight = -1.0 / (n * (n - 1) // 2)
    upstream = torch.tensor(-1.75, dtype=dtype, device=DEV)
    for mode in _modes(family):
        case = (family, means, n, m, dtype, weighted, mode)
        loss_ref, flags_ref, gmu_ref, gcov_ref = _direct_call(family, mu, cov, mode, weight, W)
        assert (gmu_ref is not None) == means, case
        mu_in = mu.clone().requires_grad_(True) if means else None
        cov_in = cov.clone().requires_grad_(True)
        loss, flags = _native.ClassPairLoss.apply(mu_in, cov_in, family, mode, EPS, weight, W)
        assert torch.equal(loss, loss_ref) and torch.equal(flags, flags_ref), case
        assert flags.tolist() == [0, 0] and bool(torch.isfinite(loss)), case
        assert not flags.requires_grad, case
        inputs = ([mu_in] if means else []) + [cov_in]
        refs = ([gmu_ref] if means else []) + [gcov_ref]
        # upstream gradient 1: the gradients of the native call themselves
        for got, ref in zip(torch.autograd.grad(loss, inputs, retain_graph=True), refs):
            assert torch.equal(got, ref), case
        # the node's backward as it stands: g * those gradients, None for the absent means and for the static arguments
        out = loss.grad_fn.apply(upstream, None)
        assert isinstance(out, tuple) and len(out) == 7 and all(o is None for o in out[2:]), case
        if means:
            assert torch.equal(out[0], upstream * gmu_ref), case
        else:
            assert out[0] is None, case
        assert torch.equal(out[1], upstream * gcov_ref), case
        # and through the autograd engine
        for got, ref in zip(torch.autograd.grad(loss, inputs, grad_outputs=upstream), refs):
            assert torch.equal(got, upstream * ref), case
