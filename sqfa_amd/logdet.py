"""Log-det family: the Stein divergence between SPD matrices, also called the Jensen-Bregman log-det divergence or
S-divergence (Cherian et al.; Sra), one of the two objectives of Harandi et al., "From manifold to manifold: geometry-aware
dimensionality reduction for SPD matrices".

    S(A, B) = logdet((A + B)/2) - 1/2 logdet A - 1/2 logdet B

    stein(A, B)[i, j]   = S(A_i, B_j)            batches of SPD matrices (nA,K,K), (nB,K,K) -> (nA,nB); for ``SecondMomentsSQFA``
    stein_root(A, B)    = sqrt(S + 1e-6)          sqrt(S) is a metric (Sra 2012)

``S`` needs Cholesky factors only: no eigen-decomposition per pair.  It equals twice the Bhattacharyya distance of the
zero-mean Gaussians N(0, A), N(0, B).

Numerical limit: ``S`` is second order in the difference of the two matrices while each log-determinant is first order, so
the three-log form loses digits for close matrices (float32, K = 4: relative error 3e-6 at S = 2e-2, 8e-4 at 2e-4, 4e-2 at
2e-6) and comes out negative for near-equal ones (float32, classes 1e-3 apart at condition number 1e3: about -2e-5 where
the true value is 1e-6).  ``S >= 0`` mathematically, so a negative result is clamped to 0 with derivative 0
(``distances.clamp_nonnegative``; NaN stays NaN), here and in the kernel alike: the root never sees a negative argument
and the gradient never pulls two such classes together.  ``distances.bhattacharyya`` shares limit and clamp.

Called directly the operators are plain torch expressions (``torch.logdet``, as the torch expression of
``distances.bhattacharyya``; NaN where a determinant is negative): any device and dtype, differentiable by autograd, results
(nA, nB) with unit batch dimensions squeezed as the operators of ``sqfa_amd.distances``.  As ``SecondMomentsSQFA``'s
``distance_fun`` in ``fit()`` the closure runs through one native fused pass, ``sqfa_stein_pairwise_loss``
(stein_kernel.hip, captured in a HIP graph by the fitting loop), under ``STEIN_FUSED_CLOSURE``: the "stein" family of
``distances.class_pair_spec``.  The operators are SPD-batch operators: on ``SQFA`` (dict statistics) there is no fused
closure for them.
"""
import torch

from .distances import (EPSILON, _batch_of_matrices, _family_spec, _squeeze_pairs, clamp_nonnegative,
                        register_class_pair)

__all__ = ["stein", "stein_root"]

# rows of A evaluated at once: bounds the (rows, nB, K, K) temporary of a direct call to about this many elements
_CHUNK_ELEMENTS = 1 << 24


def _stein_matrix(A, B):
    """(nA,nB) Stein divergences of the batches A (nA,K,K), B (nB,K,K)."""
    ldA, ldB = torch.logdet(A), torch.logdet(B)
    nA, nB, K = A.shape[0], B.shape[0], A.shape[-1]
    rows = max(1, _CHUNK_ELEMENTS // max(1, nB * K * K))
    out = []
    for a in range(0, nA, rows):
        mid = 0.5 * (A[a:a + rows, None] + B[None])
        out.append(clamp_nonnegative(torch.logdet(mid) - 0.5 * (ldA[a:a + rows, None] + ldB[None])))
    return out[0] if len(out) == 1 else torch.cat(out)


def stein(A, B):
    """Stein divergence logdet((A_i + B_j)/2) - (logdet A_i + logdet B_j)/2, clamped at 0 from below:
    (nA,K,K),(nB,K,K) -> (nA,nB)."""
    return _squeeze_pairs(_stein_matrix(_batch_of_matrices(A), _batch_of_matrices(B)))


def stein_root(A, B):
    """sqrt(stein + 1e-6)."""
    return torch.sqrt(stein(A, B) + EPSILON)


# As SecondMomentsSQFA's distance_fun: per-class Cholesky -> one pass over the class pairs that factors every pair's mean
# matrix -> per-class finish, one native call (_native.ClassPairLoss, family "stein").  False restores the fitting loop's
# generic closure.
STEIN_FUSED_CLOSURE = True
register_class_pair("stein", lambda: STEIN_FUSED_CLOSURE, {stein: ("spd", False), stein_root: ("spd", True)})


def fused_spec(fn):
    """(input kind "spd", sqrt_mode) when `fn` is an operator the native Stein pass evaluates (the "stein" family of
    distances.class_pair_spec), else None; None for everything when the switch is off."""
    return _family_spec(fn, "stein")
