"""The compact-WY restatement of the orthogonal parametrization (tests/orthogonal_oracle.py: forward and hand-derived
backward, the formulation the HIP kernels implement) against torch's _Orthogonal and its autograd, CPU float64."""
import numpy as np
import pytest

import orthogonal_oracle as oo
from conftest import rel_err

SHAPES = [(1, 4), (2, 8), (3, 8), (9, 64), (17, 68), (64, 68)]


@pytest.mark.parametrize("signs", oo.SIGNS)
@pytest.mark.parametrize("K,D", SHAPES)
def test_oracle_matches_torch_orthogonal(K, D, signs):
    X, base, R = oo.make_case(K, D, signs)
    F_ref, g_ref = oo.torch_reference(X, base, R)
    F = oo.forward(X, base)
    g = oo.backward(X, base, R)
    assert rel_err(F, F_ref) <= 1e-12
    assert rel_err(g, g_ref) <= 1e-12
    assert np.abs(F @ F.T - np.eye(K)).max() < 1e-12
    dead = np.tril_indices(K, 0, D)   # X[i, d] with d <= i: on and above the diagonal of X^T
    assert (g[dead] == 0).all() and (g_ref[dead] == 0).all()


def test_upper_entries_are_ignored():
    X, base, R = oo.make_case(9, 64, "mixed")
    Y = X.copy()
    Y[np.tril_indices(9, -1, 64)] = 7.0
    assert np.array_equal(oo.forward(X, base), oo.forward(Y, base))
    assert np.array_equal(oo.backward(X, base, R), oo.backward(Y, base, R))
