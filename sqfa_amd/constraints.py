"""Filter parametrizations (reference: src/sqfa/constraints.py).  O(K*D) elementwise torch."""
import torch
import torch.nn as nn
from torch.nn.utils import parametrize
from torch.nn.utils.parametrizations import _Orthogonal, _OrthMaps

__all__ = ["Sphere", "Identity", "FixedFilters", "Orthogonal", "orthogonal"]

# constraint="orthogonal": the Householder map of torch's parametrization through the HIP kernels (_native.OrthogonalFilters)
# wherever they apply.  False restores torch's own forward (tril, column norms, householder_product, sign, base @ Q)
# everywhere, and with it the generic chain closure for orthogonal models.
NATIVE_ORTHOGONAL = True


def __dir__():
    return __all__


class Sphere(nn.Module):
    """Each filter (row) is scaled to unit Euclidean norm (reference: constraints.py:17-54)."""

    def forward(self, X):
        return X / torch.linalg.vector_norm(X, dim=-1, keepdim=True)

    def right_inverse(self, S):
        return S


class Identity(nn.Module):
    """No constraint; exists so every model has a parametrization (reference: constraints.py:58-92)."""

    def forward(self, X):
        return X

    def right_inverse(self, S):
        return S


class FixedFilters(nn.Module):
    """The first ``n_row_fixed`` rows receive no gradient (reference: constraints.py:95-141)."""

    def __init__(self, n_row_fixed):
        super().__init__()
        self.n_row_fixed = n_row_fixed

    def forward(self, X):
        k = self.n_row_fixed
        return torch.cat([X[:k].detach(), X[k:]], dim=0)

    def right_inverse(self, X):
        return X


class Orthogonal(_Orthogonal):
    """torch's orthogonal parametrization (reference: src/sqfa/model.py:416-431 registers
    torch.nn.utils.parametrizations.orthogonal) -- same `original` parameter, `base` buffer, right_inverse and random
    numbers at registration -- whose forward runs on the native kernels for the Householder map of a wide (K,D) GPU
    parameter (K <= 64, K < D, float32/float64).  Square filters (matrix_exp), CPU tensors and K > 64 keep torch's forward."""

    def native_base(self, X):
        """The `base` matrix when the native map applies to the raw parameter X, else None."""
        from . import _native
        base = getattr(self, "base", None)
        if (NATIVE_ORTHOGONAL and self.orthogonal_map == _OrthMaps.householder and torch.is_tensor(X)
                and _native.orthogonal_supported(X, base)):
            return base
        return None

    def forward(self, X):
        base = self.native_base(X)
        if base is None:
            return super().forward(X)
        from . import _native
        return _native.OrthogonalFilters.apply(X, base)


def orthogonal(module, name="filters"):
    """Register `Orthogonal` on module.<name> the way torch.nn.utils.parametrizations.orthogonal registers its own
    class (default map: matrix_exp for a square tensor, householder otherwise; trivialization on)."""
    weight = getattr(module, name)
    orth_map = _OrthMaps.matrix_exp if weight.size(-2) == weight.size(-1) or weight.is_complex() else _OrthMaps.householder
    parametrize.register_parametrization(module, name, Orthogonal(weight, orth_map, use_trivialization=True), unsafe=True)
    return module
