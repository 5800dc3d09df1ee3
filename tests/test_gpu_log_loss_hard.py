"""GPU tests of the native Gaussian log-loss and its gradients (gl_label_kernel, gl_sample_kernel, gl_sample_finish_kernel,
gl_class_kernel, gl_finish_kernel through sqfa_amd.classify.gaussian_log_loss, GaussianClassifier.label_log_proba and
.log_loss) per entry on the hard inputs of tests/log_loss_hard.py, with upstream 0.7: contested classes at condition numbers up
to 1e6, samples 6 sigma out, means 1e3 from the origin, data at scale 1e-4 and 1e4, confident classes (gradient rows 1e-10 of
the contested ones and below), six label layouts and the prior edges of classify_hard.

Matrix, both dtypes, N = 150 (3 sample tiles; C = 9: 3 class splits, C = 3: one group, unsplit), labels round-robin:
  contested   every K of classify_hard.SIZES, C in (9, 3);   confident   C = 9, every K >= 5 of them
  the other six levels   K in (5, 17, 33, 64), C = 9
Layouts on contested at K = 5, 33, C = 9: round-robin, sorted (N = 300: 2 sample splits, the second without a labelled sample
of the low classes), tile-label (every residual of a 16-sample tile the labelled one for one class), one-class, empty-classes
(classes 0 and 8 own no sample); mislabelled on confident (ll down to -90, P_n = 1 - tiny).  The five prior edges at
contested-c1e3, K = 5 (C = 37: 10 class splits; C = 3 with weights (0, 1e-300, 1)).

Per case: every entry of ll, gZ, gmu, gcov and the loss is within its bound against the long double truth (checked against
mpmath by tests/test_log_loss_hard.py):
  float32   the a priori first-order bound of the documented arithmetic (log_loss_hard's docstring), per entry
  float64   |err| <= max(1e-10, 5 x yardstick) x the entry's own scale A, the yardstick being the float64 torch-autograd
            oracle's error against the truth in the same metric, per case; never anything a kernel returned
ll <= 0; grad_cov exactly symmetric; grad_mu and grad_cov of every zero-weight class exactly zero, and no label refused;
log_loss() equals the loss of the differentiable call; for the layout cases the results are bitwise the same over two runs.
Worst error, its bound and the ratio are printed and recorded per quantity.  ACCURACY_DROPPED would list (level, dtype) whose
kernels miss a bound for a reason of arithmetic that the CPU model reproduces, with the measured ratio ("Log-loss on
hard inputs"); finiteness, symmetry and the exact zeros still hold for such a case.  It is empty: no case misses."""
import ctypes

import numpy as np
import pytest
import torch

import classify_hard as ch
import log_loss_hard as lh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"float32": torch.float32, "float64": torch.float64}
LD = np.longdouble
# (level or "priors", dtype) -> worst measured error / bound
ACCURACY_DROPPED = {}


def _ld(t):
    return t.detach().double().cpu().numpy().astype(LD)


def _run(ref, dtype):
    """One differentiable call with its backward and the two classifier calls: quantity -> device tensor."""
    from sqfa_amd import classify
    t = lambda a, g: torch.tensor(a, dtype=DTYPES[dtype], device=DEV, requires_grad=g)
    Z, mu, cov = t(ref["Z"], True), t(ref["mu"], True), t(ref["cov"], True)
    y = torch.tensor(ref["labels"], device=DEV)
    w = None if ref["weights"] is None else list(ref["weights"])
    loss = classify.gaussian_log_loss(Z, y, mu, cov, w)   # a refused label would raise here
    assert loss.dim() == 0 and loss.dtype == DTYPES[dtype]
    (lh.UPSTREAM * loss).backward()
    clf = classify.GaussianClassifier(mu.detach(), cov.detach(), w)
    assert clf._factors is not None, "the native factor pass did not run"
    ll = clf.label_log_proba(Z.detach(), y)
    value = clf.log_loss(Z.detach(), y)
    assert isinstance(value, float) and value == loss.item(), "log_loss() is not the loss of the differentiable call"
    return dict(ll=ll, loss=loss.detach().reshape(1), gZ=Z.grad, gmu=mu.grad, gcov=cov.grad)


def _check(ref, dtype, label, record_property):
    """Everything asked of one case but the accuracy, which is returned as the list of misses."""
    got = _run(ref, dtype)
    N, K = ref["Z"].shape
    C = ref["cov"].shape[0]
    assert got["ll"].shape == (N,) and got["gZ"].shape == (N, K) and got["gmu"].shape == (C, K)
    assert got["gcov"].shape == (C, K, K)
    for q, v in got.items():
        assert v.dtype == DTYPES[dtype] and torch.isfinite(v).all(), f"{label}: {q} is not finite"
    assert (got["ll"] <= 0).all(), label
    assert torch.equal(got["gcov"], got["gcov"].transpose(1, 2)), f"{label}: grad_cov is not exactly symmetric"
    zero = torch.tensor(np.isneginf(ref["log_priors"]), device=DEV)
    assert torch.count_nonzero(got["gmu"][zero]).item() == 0, f"{label}: grad_mu of a zero-weight class"
    assert torch.count_nonzero(got["gcov"][zero]).item() == 0, f"{label}: grad_cov of a zero-weight class"
    bounds = lh.bounds(ref, dtype)
    misses = []
    for q in lh.QUANTITIES:
        want, bound = np.asarray(ref[q]), np.asarray(bounds[q])
        err = np.abs(_ld(got[q]).reshape(want.shape) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0, err / bound)   # an exact value meets a bound of 0
        at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.ndim else ()
        print(f"log-loss-hard {label} {q}: worst err {float(err[at]):.3e} bound {float(bound[at]):.3e} "
              f"ratio {float(ratio[at]):.3f}")
        record_property(f"{q}_err", float(err[at]))
        record_property(f"{q}_bound", float(bound[at]))
        record_property(f"{q}_ratio", float(ratio[at]))
        if not ratio[at] <= 1:
            misses.append((label, q, float(err[at]), float(bound[at]), float(ratio[at])))
    return got, misses


def _layout(N, C, K, dtype):
    from sqfa_amd import _lib
    cs, gps, ss = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tps = ctypes.c_longlong()
    code = _lib.SQFA_F32 if dtype == "float32" else _lib.SQFA_F64
    assert _lib.load().sqfa_gauss_log_loss_layout(N, C, K, code, ctypes.byref(cs), ctypes.byref(gps), ctypes.byref(ss),
                                                  ctypes.byref(tps)) == 0
    return cs.value, ss.value


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_cases_run_split_and_unsplit(dtype):
    """C = 9 and C = 37 run with several class splits, C = 3 with one; N = 300 with two sample splits, N = 150 with one.  The
    number of class splits never exceeds the one the float32 bound of gZ counts."""
    for level, C, K, N, layout in lh.gpu_matrix() + lh.layout_cases():
        cs, ss = _layout(N, C, K, dtype)
        assert (cs > 1) == (C == 9) and cs <= lh.class_split_bound(C), (C, K, N, cs)
        assert ss == (2 if N == lh.N_SPLIT else 1), (C, K, N, ss)
    assert {N for _, _, _, N, _ in lh.layout_cases()} == {lh.N_SAMPLES, lh.N_SPLIT}
    cs, ss = _layout(lh.N_SAMPLES, 9, 33, dtype)
    assert (cs, ss) == (3, 1)
    for edge, (C, _) in ch.PRIOR_EDGES.items():
        cs, ss = _layout(lh.N_SAMPLES, C, lh.PRIOR_EDGE_K, dtype)
        assert (cs, ss) == ((10, 1) if C == 37 else (1, 1)) and cs <= lh.class_split_bound(C), (edge, cs, ss)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", lh.gpu_matrix(), ids=lambda c: f"{c[0]}-C{c[1]}-K{c[2]}")
def test_hard_log_loss(case, dtype, record_property):
    level, C, K, N, layout = case
    ref = lh.reference(level, C, K, N, layout)
    _, misses = _check(ref, dtype, f"{level} C={C} K={K} {dtype}", record_property)
    if (level, dtype) in ACCURACY_DROPPED:
        misses = []
    assert not misses, misses


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", lh.layout_cases(), ids=lambda c: f"{c[4]}-K{c[2]}")
def test_label_layouts(case, dtype, record_property):
    level, C, K, N, layout = case
    ref = lh.reference(level, C, K, N, layout)
    got, misses = _check(ref, dtype, f"layout {layout} {level} K={K} N={N} {dtype}", record_property)
    assert not misses, misses
    again = _run(ref, dtype)
    bits = lambda t: t.view(torch.int32 if dtype == "float32" else torch.int64)
    for q in lh.QUANTITIES:
        assert torch.equal(bits(got[q]), bits(again[q])), f"{layout} K={K} {dtype}: {q} differs between two runs"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("edge", list(ch.PRIOR_EDGES))
def test_prior_edges(edge, dtype, record_property):
    """Whole class splits, a whole lane quarter and all classes but one at zero weight; a class of weight 1e-300 that owns half
    of the labels."""
    ref = lh.prior_edge(edge)
    _, misses = _check(ref, dtype, f"priors {edge} {dtype}", record_property)
    if ("priors", dtype) in ACCURACY_DROPPED:
        misses = []
    assert not misses, misses
