"""ClassStatisticsAccumulator on the CPU (the torch form of the formulas the GPU kernels use) against the float64
oracle: ragged_points-style data, C = 37, D = 13, two classes never seen, both estimators, float64, 1e-11."""
import numpy as np
import pytest
import torch

import class_statistics_oracle as oracle
from sqfa_amd import statistics
from sqfa_amd.statistics import ClassStatisticsAccumulator

C, D, TOL = 37, 13, 1e-11
ESTIMATORS = ["empirical", "oas"]


@pytest.fixture(scope="module")
def data():
    X, y = oracle.ragged_small(C, D)
    ref = {est: oracle.class_statistics(X, y, n_classes=C, estimator=est) for est in ESTIMATORS}
    return torch.tensor(X), torch.tensor(y), ref


def new():
    return ClassStatisticsAccumulator(C, D, dtype=torch.float64)


def test_exported():
    assert "ClassStatisticsAccumulator" in statistics.__all__


@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_one_update_with_all_the_data(data, estimator):
    X, y, ref = data
    acc = new().update(X, y)
    oracle.check_against(acc.finalize(estimator), ref[estimator], TOL)
    assert torch.equal(acc.counts, torch.bincount(y, minlength=C))
    # and it is what class_statistics gives for the classes that one can see (it stops at the largest label)
    st = statistics.class_statistics(X, y, estimator=estimator)
    n = st["covariances"].shape[0]
    fin = acc.finalize(estimator)
    for k in st:
        assert torch.allclose(fin[k][:n], st[k], rtol=1e-10, atol=1e-12, equal_nan=True), k


@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_seven_uneven_batches_with_classes_missing(data, estimator):
    X, y, ref = data
    acc = new()
    absent = 0
    for sl in oracle.uneven_batches(len(y)):
        absent += C - len(torch.unique(y[sl]))
        acc.update(X[sl], y[sl])
    assert absent > 2 * 7      # beyond the two classes that no batch has
    oracle.check_against(acc.finalize(estimator), ref[estimator], TOL)


@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_merge_of_two_halves(data, estimator):
    X, y, ref = data
    h = len(y) // 2
    a, b = new().update(X[:h], y[:h]), new().update(X[h:], y[h:])
    merged = a.merge(b)
    oracle.check_against(merged.finalize(estimator), ref[estimator], TOL)
    assert torch.equal(merged.counts, torch.bincount(y, minlength=C))
    assert torch.equal(merged._m2, merged._m2.transpose(1, 2))


def test_merge_with_an_empty_accumulator_changes_nothing(data):
    X, y, _ = data
    a = new().update(X, y)
    means, m2 = a._means.clone(), a._m2.clone()
    a.merge(new())
    assert torch.equal(a._means, means) and torch.equal(a._m2, m2)
    b = new().merge(a)
    assert torch.equal(b._means, means) and torch.equal(b._m2, m2)


def test_label_out_of_range(data):
    X, y, _ = data
    for bad in (C, -1):
        yb = y.clone()
        yb[3] = bad
        with pytest.raises(ValueError, match="labels must lie in"):
            new().update(X, yb)


def test_finalize_before_any_update_is_nan():
    for estimator in ESTIMATORS:
        fin = new().finalize(estimator)
        assert all(torch.isnan(v).all() for v in fin.values())
        assert fin["means"].shape == (C, D) and fin["covariances"].shape == (C, D, D)


def test_float_labels_and_estimator_check(data):
    X, y, ref = data
    acc = new().update(X, y.double())
    oracle.check_against(acc.finalize(), ref["empirical"], TOL)
    with pytest.raises(ValueError, match="estimator"):
        acc.finalize("ledoit")
