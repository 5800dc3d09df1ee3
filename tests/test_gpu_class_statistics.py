"""GPU tests of the native class statistics (sqfa_class_moments, sqfa_class_moments_update / _finalize) against the
float64 oracle tests/class_statistics_oracle.py.  Bounds: the project's own for class statistics
(test_gpu_model.test_class_statistics_on_gpu_vs_reference): rel_err < 1e-11 in float64, < 2e-5 in float32.
Shapes are the smallest at which each mechanism can go wrong: the output tile is 64 x 64, a row chunk 32 rows."""
import gc

import numpy as np
import pytest
import torch

import class_statistics_oracle as oracle
import model_cases as mc
from conftest import rel_err
from sqfa_amd import _native, statistics
from sqfa_amd.statistics import ClassStatisticsAccumulator
from sqfa_amd._optim import _no_gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-5)]
ESTIMATORS = ["empirical", "oas"]
CODE = {"empirical": _native.COV_EMPIRICAL, "oas": _native.COV_OAS}


@pytest.fixture
def no_bmm(monkeypatch):
    """The torch path's batched GEMM raises: whatever passes ran the native kernels."""
    def refuse(*a, **k):
        raise AssertionError("torch.bmm called: the torch path ran")
    monkeypatch.setattr(torch, "bmm", refuse)


_refs = {}


def reference(name, make, estimator, n_classes=None):
    """(X, y, oracle statistics) of a named input, computed once per session and shared."""
    if name not in _refs:
        _refs[name] = (make(), {})
    (X, y), by_est = _refs[name]
    if estimator not in by_est:
        by_est[estimator] = oracle.class_statistics(X, y, n_classes=n_classes, estimator=estimator)
    return X, y, by_est[estimator]


def dev(X, y, dtype):
    return torch.tensor(X, dtype=dtype, device=DEV), torch.tensor(y, device=DEV)


def raw_moments(X, y, C, estimator, grouped=False):
    """_native.class_moments as a dict; grouped: the rows are sorted on the host and row_index is NULL."""
    order, class_start = _native.grouped_rows(y, C)
    if grouped:
        X, order = X[order].contiguous(), None
    means, cov, second = _native.class_moments(X, order, class_start, C, CODE[estimator], True)
    return {"means": means, "covariances": cov, "second_moments": second}


# ---- G5 and G5c through the kernels ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_reference_goldens_through_the_native_path(dtype, tol, no_bmm):
    """G5 and the ragged 1000-class G5c, both estimators, float labels: the reference's recorded outputs."""
    assert statistics.NATIVE_CLASS_STATISTICS
    mc.check_class_statistics_vs_reference(DEV, dtype, tol)


def test_switch_off_keeps_the_torch_path(monkeypatch, no_bmm):
    monkeypatch.setattr(statistics, "NATIVE_CLASS_STATISTICS", False)
    X, y = dev(mc.G5["pts_X"], mc.G5["pts_y"], torch.float64)
    with pytest.raises(AssertionError, match="torch path ran"):
        statistics.class_statistics(X, y)


# ---- column tails, the scalar path, empty and singleton classes ----------------------------------------------------------

TAIL_SIZES = oracle.TAIL_SIZES


def tails(D):
    return lambda: oracle.tails(D)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("D", [1, 3, 5, 17, 63, 65, 100, 132])
def test_column_tails_and_small_classes(D, dtype, tol, no_bmm):
    """One class per size in TAIL_SIZES (six classes, so that every listed size occurs).  D = 100 and 132 take the
    16-byte loads, the others one element per load; 65, 100 and 132 have several tiles, the last one partial.
    OAS from D = 3: for D = 1 the shrinkage coefficient is 0/0 by its own formula."""
    for estimator in ESTIMATORS if D >= 3 else ["empirical"]:
        Xn, yn, ref = reference(f"tails{D}", tails(D), estimator)
        X, y = dev(Xn, yn, dtype)
        st = statistics.class_statistics(X, y, estimator=estimator)
        # the NaN pattern: the empty class everywhere, the singleton in its matrices only
        assert torch.isnan(st["means"][0]).all() and torch.isfinite(st["means"][1:]).all()
        for k in ("covariances", "second_moments"):
            assert torch.isnan(st[k][:2]).all() and torch.isfinite(st[k][2:]).all()
        errs = oracle.check_against(st, ref, tol, what=(D, estimator))
        print(f"D={D} {dtype} {estimator}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


# ---- gather -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [17, 100])
def test_gather_grouped_and_unaligned_views_agree_bitwise(D, dtype):
    """Shuffled rows through row_index, the same rows grouped on the host with row_index NULL, and the same points as a
    view at an offset of one element (an unaligned base: one element per load): the same bits."""
    Xn, yn, ref = reference(f"tails{D}", tails(D), "empirical")
    X, y = dev(Xn, yn, dtype)
    C = len(TAIL_SIZES)
    buf = torch.empty(X.numel() + 1, dtype=dtype, device=DEV)
    shifted = buf[1:].view_as(X)
    shifted.copy_(X)
    assert shifted.data_ptr() % 16 != 0 and X.data_ptr() % 16 == 0 and shifted.is_contiguous()
    for estimator in ESTIMATORS:
        base = raw_moments(X, y, C, estimator)
        for other in (raw_moments(X, y, C, estimator, grouped=True), raw_moments(shifted, y, C, estimator)):
            for k in base:
                assert torch.equal(torch.nan_to_num(base[k], nan=-7.0), torch.nan_to_num(other[k], nan=-7.0)), (estimator, k)
    oracle.check_against(raw_moments(shifted, y, C, "empirical"), ref, 1e-11 if dtype == torch.float64 else 2e-5)


# ---- symmetry and reproducibility ---------------------------------------------------------------------------------------

def full_classes(D):
    return lambda: oracle.ragged_small(C=5, D=D, seed=200 + D, empty=(), lo=3, hi=75)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [100, 132])
def test_outputs_are_exactly_symmetric_and_reproducible(D, dtype):
    Xn, yn, _ = reference(f"full{D}", full_classes(D), "empirical")
    X, y = dev(Xn, yn, dtype)
    for estimator in ESTIMATORS:
        a = statistics.class_statistics(X, y, estimator=estimator)
        b = statistics.class_statistics(X, y, estimator=estimator)
        for k in ("covariances", "second_moments"):
            assert torch.isfinite(a[k]).all()
            assert torch.equal(a[k], a[k].transpose(1, 2)), (estimator, k)
        for k in a:
            assert torch.equal(a[k], b[k]), (estimator, k)
    acc, again = (ClassStatisticsAccumulator(5, D, dtype=dtype, device=DEV) for _ in range(2))
    for sl in oracle.uneven_batches(len(yn), parts=3):
        acc.update(X[sl], y[sl])
        again.update(X[sl], y[sl])
    assert torch.equal(acc._m2, acc._m2.transpose(1, 2)) and acc._m2.abs().sum() > 0
    assert torch.equal(acc._m2, again._m2) and torch.equal(acc._means, again._means)
    fin = acc.finalize("oas")
    assert torch.equal(fin["covariances"], fin["covariances"].transpose(1, 2))
    assert torch.equal(fin["second_moments"], fin["second_moments"].transpose(1, 2))


# ---- centring -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_class_means_a_hundred_standard_deviations_out_f32(estimator, no_bmm):
    """A raw-moment formulation misses 2e-5 here by two orders of magnitude; the torch path meets it on the CPU
    (test_class_statistics_oracle.test_float32_inputs_are_within_reach_of_the_metric)."""
    Xn, yn, ref = reference("far", oracle.far_means, estimator)
    X, y = dev(Xn, yn, torch.float32)
    errs = oracle.check_against(statistics.class_statistics(X, y, estimator=estimator), ref, 2e-5)
    print("far means:", errs)
    acc = ClassStatisticsAccumulator(4, 20, dtype=torch.float32, device=DEV)
    for sl in oracle.uneven_batches(len(yn)):
        acc.update(X[sl], y[sl])
    errs = oracle.check_against(acc.finalize(estimator), ref, 2e-5)
    print("far means, 7 batches:", errs)


# ---- the accumulator ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_accumulator_on_the_gpu(estimator, dtype, tol):
    """C = 37, D = 13 ragged data with two classes never seen: one update with everything against class_statistics,
    seven uneven batches (each lacks classes) against the oracle."""
    C, D = 37, 13
    Xn, yn, ref = reference("ragged37", lambda: oracle.ragged_small(C, D), estimator, n_classes=C)
    X, y = dev(Xn, yn, dtype)
    whole = ClassStatisticsAccumulator(C, D, dtype=dtype, device=DEV).update(X, y)
    fin = whole.finalize(estimator)
    oracle.check_against(fin, ref, tol)
    st = statistics.class_statistics(X, y, estimator=estimator)
    for k in st:
        ok = ~torch.isnan(st[k])
        assert torch.equal(ok, ~torch.isnan(fin[k]))
        assert rel_err(fin[k][ok].cpu(), st[k][ok].cpu()) < tol, k
    assert torch.equal(whole.counts.cpu(), torch.bincount(torch.tensor(yn), minlength=C))
    acc = ClassStatisticsAccumulator(C, D, dtype=dtype, device=DEV)
    absent = 0
    for sl in oracle.uneven_batches(len(yn)):
        absent += C - len(np.unique(yn[sl]))
        acc.update(X[sl], y[sl])
    assert absent > 2 * 7      # beyond the two classes that no batch has
    errs = oracle.check_against(acc.finalize(estimator), ref, tol)
    print(f"7 batches {dtype} {estimator}:", errs)
    # the CPU form of the same formulas, merged into the GPU state of the first half
    h = len(yn) // 2
    first = ClassStatisticsAccumulator(C, D, dtype=dtype, device=DEV).update(X[:h], y[:h])
    second = ClassStatisticsAccumulator(C, D, dtype=dtype).update(X[h:].cpu(), y[h:].cpu())
    oracle.check_against(first.merge(second).finalize(estimator), ref, tol)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_update_leaves_an_absent_class_untouched(dtype):
    C, D = 5, 100
    Xn, yn, _ = reference("full100", full_classes(100), "empirical")
    X, y = dev(Xn, yn, dtype)
    acc = ClassStatisticsAccumulator(C, D, dtype=dtype, device=DEV).update(X, y)
    means, m2, counts = acc._means.clone(), acc._m2.clone(), acc._counts.clone()
    keep = (y != 2) & (y != 4)
    acc.update(X[keep], y[keep])
    for c in (2, 4):
        assert torch.equal(acc._means[c], means[c]) and torch.equal(acc._m2[c], m2[c]) and acc._counts[c] == counts[c]
    for c in (0, 1, 3):
        assert acc._counts[c] == 2 * counts[c] and not torch.equal(acc._m2[c], m2[c])
    with pytest.raises(ValueError, match="labels must lie in"):
        acc.update(X, y + 1)


# ---- graph capture ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("estimator", ESTIMATORS)
def test_captured_call_equals_the_eager_one(estimator):
    Xn, yn, _ = reference("full100", full_classes(100), "empirical")
    X, y = dev(Xn, yn, torch.float32)
    order, class_start = _native.grouped_rows(y, 5)
    eager = _native.class_moments(X, order, class_start, 5, CODE[estimator], True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # torch no longer collects garbage before a capture, and a cyclic collection inside one that finalises device
    # tensors or an older graph aborts the process (_optim._no_gc): collect now, none while the stream captures
    gc.collect()
    with _no_gc(), torch.cuda.graph(graph):
        captured = _native.class_moments(X, order, class_start, 5, CODE[estimator], True)
    for t in captured:
        t.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


# ---- model level --------------------------------------------------------------------------------------------------------

def test_fit_from_points_with_the_switch_on_and_off(monkeypatch):
    """Two routes to the same fit (bounds of test_gpu_model.test_device_side_compact_lbfgs_matches_torch_lbfgs)."""
    C, D, K = 6, 16, 2
    Xn, yn = oracle.ragged_small(C=C, D=D, seed=77, empty=(), lo=30, hi=60)
    X, y = dev(Xn, yn, torch.float64)
    runs = {}
    for native in (True, False):
        monkeypatch.setattr(statistics, "NATIVE_CLASS_STATISTICS", native)
        model = mc.make_model("smsqfa", D, K, 0.01, "sphere", torch.float64, DEV)
        model.fit_pca(X=X)
        loss, _ = model.fit(X=X, y=y, max_epochs=2, show_progress=False, return_loss=True)
        runs[native] = (loss.numpy(), model.filters.detach().cpu().numpy())
    assert np.abs(runs[True][0] - runs[False][0]).max() < 1e-9
    assert rel_err(runs[True][1], runs[False][1]) < 1e-7


def test_native_statistics_pass_the_symmetry_check_exactly():
    """What decides whether a fit gets the packed projection: a native result is symmetric bit for bit, at any size."""
    Xn, yn, _ = reference("full132", full_classes(132), "empirical")
    X, y = dev(Xn, yn, torch.float32)
    st = statistics.class_statistics(X, y)
    assert _native._is_symmetric_batch(st["second_moments"]) and _native._is_symmetric_batch(st["covariances"])
    assert (st["second_moments"] - st["second_moments"].transpose(1, 2)).abs().max() == 0
