"""Kullback-Leibler family: the Jeffreys divergence (symmetric Kullback-Leibler divergence) between Gaussians.

With the precisions ``P_c = inv(Sigma_c)`` and ``delta = mu_i - mu_j``

    J_ij = KL(i||j) + KL(j||i)
         = 1/2 [tr(P_j Sigma_i) + tr(P_i Sigma_j) - 2K + delta^T (P_i + P_j) delta]            (textbook form)
         = -1/2 <P_i - P_j, Sigma_i - Sigma_j> + 1/2 delta^T (P_i + P_j) delta                  (explicit-difference form)

    jeffreys(sA, sB)[i, j]     = J_ij            dicts with 'means' (n,K) and 'covariances' (n,K,K); for ``SQFA``
    jeffreys_root(sA, sB)      = sqrt(J + 1e-6)
    jeffreys_spd(A, B)[i, j]   = J_ij, delta = 0  batches of SPD matrices; for ``SecondMomentsSQFA``
    jeffreys_spd_root(A, B)    = sqrt(J + 1e-6)

The explicit-difference form is the one evaluated, everywhere: the two traces of the textbook form are each about K and
cancel the digits that matter when two classes are close (in float32, two classes 1e-3 apart: 3e-3 relative error against
3e-6).  With the precisions in hand a pair costs O(K^2); no per-pair factorisation.  ``J >= 0`` mathematically: a rounded
negative value (not seen on the close, ill-conditioned classes of the tests) is clamped to 0 with derivative 0, by
``distances.clamp_nonnegative`` here and by the same rule in the kernel.

Called directly the operators are plain torch expressions: any device and dtype, differentiable by autograd, results
(nA, nB) with unit batch dimensions squeezed as the operators of ``sqfa_amd.distances``.  As a model's ``distance_fun`` in
``fit()`` the closure runs through one native fused pass, ``sqfa_jeffreys_pairwise_loss`` (jeffreys_kernel.hip, captured in
a HIP graph by the fitting loop), under ``JEFFREYS_FUSED_CLOSURE``: the "jeffreys" family of ``distances.class_pair_spec``,
the registry ``model._closure_plan`` asks.  The operators are deliberately not in ``distances._FUSED``: they are no
pair-kernel operators.
"""
import torch

from .distances import (EPSILON, _batch_of_matrices, _family_spec, _gaussian_inputs, _squeeze_pairs, clamp_nonnegative,
                        register_class_pair)

__all__ = ["jeffreys", "jeffreys_root", "jeffreys_spd", "jeffreys_spd_root"]

# rows of A evaluated at once: bounds the (rows, nB, K, K) temporary of a direct call to about this many elements
_CHUNK_ELEMENTS = 1 << 24


def _jeffreys_matrix(muA, covA, muB, covB):
    """(nA,nB) Jeffreys divergences in the explicit-difference form; mu* None: zero means."""
    PA, PB = torch.linalg.inv(covA), torch.linalg.inv(covB)
    nA, nB, K = covA.shape[0], covB.shape[0], covA.shape[-1]
    rows = max(1, _CHUNK_ELEMENTS // max(1, nB * K * K))
    out = []
    for a in range(0, nA, rows):
        dP = PA[a:a + rows, None] - PB[None]
        dS = covA[a:a + rows, None] - covB[None]
        J = -0.5 * (dP * dS).sum(dim=(-2, -1))
        if muA is not None:
            delta = muA[a:a + rows, None] - muB[None]
            sP = PA[a:a + rows, None] + PB[None]
            J = J + 0.5 * torch.einsum("abk,abkl,abl->ab", delta, sP, delta)
        out.append(clamp_nonnegative(J))      # J >= 0 mathematically: a rounded negative one is 0 with derivative 0
    return out[0] if len(out) == 1 else torch.cat(out)


def jeffreys(statistics_A, statistics_B):
    """Jeffreys divergence KL(i||j) + KL(j||i) between Gaussians N(mu_i, Sigma_i), N(mu_j, Sigma_j): dicts with 'means'
    (n,K) and 'covariances' (n,K,K) -> (nA,nB)."""
    muA, covA, muB, covB = _gaussian_inputs(statistics_A, statistics_B)
    return _squeeze_pairs(_jeffreys_matrix(muA, covA, muB, covB))


def jeffreys_root(statistics_A, statistics_B):
    """sqrt(jeffreys + 1e-6)."""
    return torch.sqrt(jeffreys(statistics_A, statistics_B) + EPSILON)


def jeffreys_spd(A, B):
    """Jeffreys divergence between the zero-mean Gaussians of SPD matrices: (nA,K,K),(nB,K,K) -> (nA,nB)."""
    return _squeeze_pairs(_jeffreys_matrix(None, _batch_of_matrices(A), None, _batch_of_matrices(B)))


def jeffreys_spd_root(A, B):
    """sqrt(jeffreys_spd + 1e-6)."""
    return torch.sqrt(jeffreys_spd(A, B) + EPSILON)


# As a model's distance_fun: per-class precisions -> one pass over the class pairs -> per-class chain rule through the
# inverse, one native call (_native.ClassPairLoss, family "jeffreys").  False restores the fitting loop's generic closure.
JEFFREYS_FUSED_CLOSURE = True
register_class_pair("jeffreys", lambda: JEFFREYS_FUSED_CLOSURE,
                    {jeffreys: ("gaussian", False), jeffreys_root: ("gaussian", True),
                     jeffreys_spd: ("spd", False), jeffreys_spd_root: ("spd", True)})


def fused_spec(fn):
    """(input kind "gaussian" | "spd", sqrt_mode) when `fn` is an operator the native Jeffreys pass evaluates (the "jeffreys"
    family of distances.class_pair_spec), else None; None for everything when the switch is off."""
    return _family_spec(fn, "jeffreys")
