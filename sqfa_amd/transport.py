"""Optimal-transport distances between SPD matrices and Gaussians, on the native pair kernels.

The reference's tutorial (docs/source/tutorials/distances.md:127-178, 460-491) builds two ``distance_fun``s on top of
the package: ``bw_distance_sq`` / ``bw_distance`` (Bures-Wasserstein, for ``SecondMomentsSQFA``) and
``wasserstein_distance`` (2-Wasserstein between Gaussians, for ``SQFA``).  This module provides them as operators of
this package, evaluated by ``sqfa_bw_pairwise`` (include/sqfa_hip.h): the affine-invariant pair kernels with a second
spectral function, forward and closed-form backward, nothing of size (nA, nB, m, m) formed.

    bw2(A, B) = tr A + tr B - 2 sum_k sqrt(lambda_k(A B))
    bures_wasserstein_sq(A, B)[i, j] = bw2(A_i, B_j)                  (raw: may be a tiny negative number from rounding)
    bures_wasserstein(A, B)          = sqrt(|bw2| + 1e-6)
    wasserstein_sq(sA, sB)[i, j]     = |mu_i - mu_j|^2 + bw2(Sigma_i, Sigma_j)
    wasserstein(sA, sB)              = sqrt(|wasserstein_sq| + 1e-6)

Results are (nA, nB) with unit batch dimensions squeezed, as the other operators of ``sqfa_amd.distances``.  The
tutorial's functions return the transpose (nB, nA); the two agree in the self case (A is B) that the models use.
GPU tensors only (CPU tensors raise RuntimeError); matrix sizes up to 128 (NotImplementedError above).

``bures_wasserstein[_sq]`` are fusable: ``SecondMomentsSQFA(distance_fun=transport.bures_wasserstein)`` evaluates its
closure as one loss + gradient launch chain on the Bures-Wasserstein kernels (single node / HIP graph).  ``wasserstein``
runs on the autograd path (mean term in torch, covariance term on the kernels).
"""
import torch

from . import _native
from .distances import EPSILON, _batch_of_matrices, _fusable, _gaussian_inputs, _squeeze_pairs

__all__ = ["bures_wasserstein_sq", "bures_wasserstein", "wasserstein_sq", "wasserstein"]


def _bw_matrix(A, B, sqrt_mode, same):
    A3 = _batch_of_matrices(A)
    if same and A3.shape[0] >= 2:
        D, _flag = _native.PairDistanceMatrix.apply(A3, None, 1.0, EPSILON, sqrt_mode, "bw")
    else:
        B3 = _batch_of_matrices(B)
        D, _flag = _native.PairDistanceMatrix.apply(A3, B3, 1.0, EPSILON, sqrt_mode, "bw")
    return D


@_fusable("spd", 1.0, False, "bw")
def bures_wasserstein_sq(A, B):
    """Squared Bures-Wasserstein distance tr A_i + tr B_j - 2 tr (A_i^1/2 B_j A_i^1/2)^1/2: (nA,m,m),(nB,m,m) -> (nA,nB)
    (tutorial's bw_distance_sq, transposed)."""
    return _squeeze_pairs(_bw_matrix(A, B, False, A is B))


@_fusable("spd", 1.0, True, "bw")
def bures_wasserstein(A, B):
    """Bures-Wasserstein distance sqrt(|bw2| + 1e-6) (tutorial's bw_distance, transposed)."""
    return _squeeze_pairs(_bw_matrix(A, B, True, A is B))


def wasserstein_sq(statistics_A, statistics_B):
    """Squared 2-Wasserstein distance between Gaussians N(mu_i, Sigma_i), N(mu_j, Sigma_j): dicts with 'means' (n,m) and
    'covariances' (n,m,m) -> (nA,nB)."""
    muA, covA, muB, covB = _gaussian_inputs(statistics_A, statistics_B)
    same = (statistics_A["means"] is statistics_B["means"]
            and statistics_A["covariances"] is statistics_B["covariances"])
    bw2 = _bw_matrix(covA, covB, False, same)
    dmu = torch.sum((muA[:, None] - muB[None, :]) ** 2, dim=-1)
    return _squeeze_pairs(dmu + bw2)


def wasserstein(statistics_A, statistics_B):
    """2-Wasserstein distance sqrt(|wasserstein_sq| + 1e-6) (tutorial's wasserstein_distance, transposed)."""
    return torch.sqrt(torch.abs(wasserstein_sq(statistics_A, statistics_B)) + EPSILON)
