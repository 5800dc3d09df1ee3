"""sqfa_amd -- Supervised Quadratic Feature Analysis with an MI355X-native training core.

Same sub-modules and public names as the reference package ``sqfa`` (model, distances,
linalg, statistics, constraints, _optim); the pairwise affine-invariant distance path is
implemented by hand-written HIP kernels behind the C ABI in include/sqfa_hip.h.  ``transport`` adds the
Bures-Wasserstein / Wasserstein distances of the reference's tutorial on the same kernels; ``divergences`` adds the
Jeffreys (symmetric Kullback-Leibler) divergence with its own native fused closure; ``logdet`` the Stein (Jensen-Bregman
log-det) divergence with its own; ``classify`` scores and classifies samples with the class Gaussians in feature space
(QDA) on native kernels.
"""
from . import _optim, classify, constraints, distances, divergences, linalg, logdet, model, parallel, statistics, transport  # noqa: F401

__all__ = ["model", "distances", "linalg", "statistics", "constraints", "parallel", "transport", "divergences", "logdet",
           "classify"]
__version__ = "0.1.0"
