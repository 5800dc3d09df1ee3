"""The class-statistics oracle (tests/class_statistics_oracle.py) against the reference's recorded outputs, and the
inputs of the float32 tests against the project's bound on the torch path (run on the CPU): an input that the torch
expression itself cannot hold to 2e-5 would be too hard for the metric."""
import numpy as np
import pytest
import torch

import class_statistics_oracle as oracle
from conftest import load_golden, rel_err
from model_cases import ragged_points
from sqfa_amd import statistics


@pytest.mark.parametrize("estimator", ["empirical", "oas"])
def test_oracle_matches_the_reference_outputs(estimator):
    G5, G5C = load_golden("g5_quirks.npz"), load_golden("g5c_class_statistics.npz")
    st = oracle.class_statistics(G5["pts_X"], G5["pts_y"], estimator=estimator)
    for k, v in st.items():
        assert rel_err(v, G5[f"class_stats_{estimator}_{k}"]) < 1e-13, k
    X, y = ragged_points()
    st = oracle.class_statistics(X, y, estimator=estimator)
    for k, v in st.items():
        assert rel_err(v, G5C[f"{estimator}_{k}"]) < 1e-13, k


def test_oracle_nan_pattern_of_empty_and_singleton_classes():
    X = np.arange(12.0).reshape(4, 3)
    st = oracle.class_statistics(X, np.array([0, 0, 0, 2]), n_classes=4)
    assert np.isfinite(st["means"][[0, 2]]).all() and np.isnan(st["means"][[1, 3]]).all()
    assert np.isfinite(st["covariances"][0]).all() and np.isnan(st["covariances"][1:]).all()


@pytest.mark.parametrize("estimator", ["empirical", "oas"])
def test_float32_inputs_are_within_reach_of_the_metric(estimator):
    """The torch path in float32 on the CPU meets 2e-5 with margin on every input of the float32 GPU tests."""
    inputs = [oracle.far_means(), oracle.ragged_small(dtype=np.float32), 
              oracle.ragged_small(C=5, D=100, seed=300, empty=(), lo=3, hi=75),
              oracle.ragged_small(C=5, D=132, seed=332, empty=(), lo=3, hi=75)]
    inputs += [oracle.tails(D) for D in ([1] if estimator == "empirical" else []) + [3, 5, 17, 63, 65, 100, 132]]
    for X, y in inputs:
        X = X.astype(np.float32)
        ref = oracle.class_statistics(X, y, estimator=estimator)
        st = statistics.class_statistics(torch.tensor(X), torch.tensor(y), estimator=estimator)
        errs = oracle.check_against(st, ref, 2e-5)
        assert max(errs.values()) < 5e-6, errs
