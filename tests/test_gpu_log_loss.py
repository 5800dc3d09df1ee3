"""GPU tests of the native Gaussian log-loss and its gradients (sqfa_gauss_log_loss, sqfa_gauss_log_loss_backward through
sqfa_amd.classify) against the float64 torch-autograd oracle tests/log_loss_oracle.py.

Shapes (C, K, N): the boundary list of tests/test_gpu_classify.py (the forward runs the scores pass, and the sample-owned
backward pass has its geometry: the MFMA k-step of 4 and the 16-row block of K, K = 1, 3, 4, 5, 16, 17, 33, 48, 64 in all
four row-block variants with one and four classes per stage; 16 samples per wave and 64 per workgroup; classes in groups of
4; class splits below 1024 sample tiles).  The new kernels' own boundaries:
  label pass       64 samples per workgroup, one per lane (N = 1, 17, 65, 257, 65537: partial and several workgroups), the
                   lower triangle of W in a K-long loop (K = 1 ... 64), the reduction of the workgroups' sums (1 to 1025).
  sample-owned     the second product's contraction over the accumulator rows: every row block rb feeds the column blocks
                   kb <= rb (K = 17, 33, 48, 64: 2, 3, 4 blocks); split ((300, 16, 2000): 15 class splits, (9, 33, 300): 3
                   splits with one class per stage) and unsplit ((5, 3, 65537): 1025 tiles; C <= 4: one group); its finish,
                   one sample per lane like the label pass, sums 1 to 15 splits and adds the labelled class's term, which
                   carries the whole gradient where the classes are far apart ((9, 33, 300) at sep 1: a loss of 1e-11).
  class-owned      16-sample tiles dealt to 4 waves (N = 1: one wave works, 17: two, 100, 200: several tiles per wave and a
                   partial one), the blocks of M on and below the diagonal (1, 3, 6, 10 of them), sample splits from 17 tiles
                   on (N = 257: 2 splits; (5, 3, 65537): 257 splits; N <= 256: unsplit), the per-class finish (K^2 entries
                   over 256 threads: K = 16 exactly one each, K = 17 two, K = 64 sixteen).
The module asserts through sqfa_gauss_log_loss_layout that both passes run split and unsplit.

Tolerances, the project's convention: float64 error <= 1e-10 (1 + max |value|) for values and <= 1e-10 max |gradient| per
gradient tensor; float32 error <= max(1e-5 x that scale, 5 x the error of the same formula in float32 torch with autograd on
the same inputs), printed beside the observed error and their ratio.

Per entry as well (test_loss_and_gradients_match_the_oracle): every case with C N K^2 <= 2e7 is also held, entry by entry, to
the long double truth and the bounds of tests/log_loss_hard.py on the same inputs: in float32 the a priori bound of the
documented arithmetic, in float64 max(1e-10, 5 x the float64 oracle's own error) x the entry's scale.  The two cases at
(C, K, N) = (300, 16, 2000) are left to the rule above alone: their long double reference is too large for a quick test.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import classify_hard
import classify_oracle
import log_loss_hard
import log_loss_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
UPSTREAM = 0.7
SHAPES = [(1, 1, 1), (2, 1, 65), (3, 3, 17), (17, 4, 257), (37, 16, 1000), (37, 17, 1000), (130, 5, 513), (9, 33, 300),
          (5, 64, 200), (4, 48, 100), (300, 16, 2000), (5, 3, 65537)]
# (C, K, N, sep, means, priors): every shape with sep 1 and uniform priors, a few with sep 0, one with zero means, one with
# non-uniform priors that include a zero
CASES = [(C, K, N, 1.0, True, False) for C, K, N in SHAPES] + \
        [(C, K, N, 0.0, True, False) for C, K, N in [(3, 3, 17), (37, 17, 1000), (300, 16, 2000)]] + \
        [(9, 33, 300, 0.0, False, False), (37, 16, 1000, 1.0, True, True)]


def _ids(case):
    C, K, N, sep, means, priors = case
    return f"C{C}-K{K}-N{N}-sep{sep:g}" + ("" if means else "-zeromean") + ("-priors" if priors else "")


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    """The problem rounded to `dtype`, the float64 oracle on those numbers and, for float32, the same formula in float32
    torch with autograd."""
    out = dict(log_loss_oracle.case(*case, np_dtype=_np_dtype(dtype), upstream=UPSTREAM))
    out["torch32"] = None
    if dtype == torch.float32:
        out["torch32"] = log_loss_oracle.evaluate(out["Z"], out["labels"], out["mu"], out["cov"], out["w"], UPSTREAM,
                                                  dtype=torch.float32)
    return out


PER_ENTRY_LIMIT = 2e7   # C N K^2 of the long double reference


@functools.lru_cache(maxsize=None)
def _per_entry(case, dtype):
    """(truth, quantity -> per-entry bound) of log_loss_hard on the inputs of `_reference(case, dtype)`."""
    ref = _reference(case, dtype)
    C, K, N = case[:3]
    ev = log_loss_hard.evaluate(ref["Z"], ref["labels"], ref["mu"], ref["cov"], classify_hard.log_priors(ref["w"], C), UPSTREAM)
    if dtype == torch.float32:
        return ev, {q: ev["b_" + q] for q in log_loss_hard.QUANTITIES}
    # the float64 oracle's own error against the truth, on the same numbers; nothing a kernel returned
    tol = log_loss_hard.tolerances64(log_loss_hard.yardsticks(ev, ref["ref"]))
    return ev, {q: t * ev["A_" + q] for q, t in tol.items()}


def _check_per_entry(got, case, dtype):
    ev, bounds = _per_entry(case, dtype)
    for q, value in got.items():
        if value is None:
            continue   # zero means: no gradient of the means
        want, bound = np.asarray(ev[q]), np.asarray(bounds[q])
        value = value.detach().double().cpu().numpy() if torch.is_tensor(value) else np.float64(value)
        err = np.abs(value.astype(np.longdouble).reshape(want.shape) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0, err / bound)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.ndim else ()
        print(f"{q} per entry: worst err {float(err[at]):.3e} bound {float(bound[at]):.3e} ratio {float(ratio[at]):.3f}")
        assert ratio[at] <= 1, (q, at, float(err[at]), float(bound[at]))


def _device_inputs(ref, dtype, requires_grad=(True, True, True)):
    t = lambda a, g: None if a is None else torch.tensor(a, dtype=dtype, device=DEV, requires_grad=g)
    return (t(ref["Z"], requires_grad[0]), torch.tensor(ref["labels"], device=DEV), t(ref["mu"], requires_grad[1]),
            t(ref["cov"], requires_grad[2]), ref["w"])


def _check(got, ref, key, dtype, gradient):
    want = ref["ref"][key]
    got = np.asarray(got.detach().double().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    scale = np.abs(want).max() if gradient else 1 + np.abs(want).max()
    err = np.abs(got - want).max()
    if dtype == torch.float64:
        print(f"{key}: max error {err:.3e}, scale {scale:.3e}, relative {err / max(scale, 1e-300):.3e}")
        assert err <= 1e-10 * scale
    else:
        torch_err = np.abs(np.asarray(ref["torch32"][key], dtype=np.float64) - want).max()
        bound = max(1e-5 * scale, 5 * torch_err)
        print(f"{key}: max error {err:.3e}, bound {bound:.3e} (scale {scale:.3e}), float32 torch {torch_err:.3e}, "
              f"ratio to torch {err / max(torch_err, 1e-30):.2f}")
        assert err <= bound


def _layout(N, C, K, dtype):
    from sqfa_amd import _lib
    cs, gps, ss = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tps = ctypes.c_longlong()
    code = _lib.SQFA_F32 if dtype == torch.float32 else _lib.SQFA_F64
    assert _lib.load().sqfa_gauss_log_loss_layout(N, C, K, code, ctypes.byref(cs), ctypes.byref(gps), ctypes.byref(ss),
                                                  ctypes.byref(tps)) == 0
    return cs.value, gps.value, ss.value, tps.value


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_shapes_cover_both_sides_of_every_split(dtype):
    lay = {shape: _layout(shape[2], shape[0], shape[1], dtype) for shape in SHAPES}
    class_splits = {s: v[0] for s, v in lay.items()}
    sample_splits = {s: v[2] for s, v in lay.items()}
    print(lay)
    # the sample-owned pass: split with four classes per stage and with one, unsplit with several groups and with one
    assert class_splits[(300, 16, 2000)] > 1 and class_splits[(9, 33, 300)] > 1
    assert class_splits[(5, 3, 65537)] == 1 and lay[(5, 3, 65537)][1] == 2 and class_splits[(4, 48, 100)] == 1
    # the class-owned pass: unsplit, two splits, many splits
    assert sample_splits[(3, 3, 17)] == 1 and sample_splits[(5, 64, 200)] == 1 and sample_splits[(4, 48, 100)] == 1
    assert sample_splits[(17, 4, 257)] == 2 and sample_splits[(5, 3, 65537)] > 16
    assert all(sample_splits[s] > 1 for s in [(37, 16, 1000), (37, 17, 1000), (9, 33, 300), (300, 16, 2000)])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_loss_and_gradients_match_the_oracle(case, dtype):
    from sqfa_amd import classify
    ref = _reference(case, dtype)
    Z, y, mu, cov, w = _device_inputs(ref, dtype)
    loss = classify.gaussian_log_loss(Z, y, mu, cov, w)
    assert loss.dim() == 0 and loss.dtype == dtype and loss.requires_grad
    (UPSTREAM * loss).backward()
    _check(loss.item(), ref, "loss", dtype, gradient=False)
    _check(Z.grad, ref, "gZ", dtype, gradient=True)
    _check(cov.grad, ref, "gcov", dtype, gradient=True)
    if mu is not None:
        _check(mu.grad, ref, "gmu", dtype, gradient=True)
    assert torch.equal(cov.grad, cov.grad.transpose(1, 2)), "grad_cov is not exactly symmetric"
    clf = classify.GaussianClassifier(None if mu is None else mu.detach(), cov.detach(), w)
    assert clf._factors is not None
    ll = clf.label_log_proba(Z.detach(), y)
    assert ll.shape == (case[2],) and ll.dtype == dtype and not ll.requires_grad
    _check(ll, ref, "ll", dtype, gradient=False)
    assert (ll <= 0).all()
    value = clf.log_loss(Z.detach(), y)
    assert isinstance(value, float) and value == loss.item()
    if case[0] * case[2] * case[1] ** 2 <= PER_ENTRY_LIMIT:
        _check_per_entry(dict(loss=loss.item(), ll=ll, gZ=Z.grad, gmu=None if mu is None else mu.grad, gcov=cov.grad), case,
                         dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 100), (1, 33, 70)], ids=str)
def test_one_class_gives_exact_zeros(shape, dtype):
    from sqfa_amd import classify
    ref = _reference(shape + (1.0, True, False), dtype)
    Z, y, mu, cov, w = _device_inputs(ref, dtype)
    loss = classify.gaussian_log_loss(Z, y, mu, cov, w)
    loss.backward()
    assert loss.item() == 0.0
    for g in (Z.grad, mu.grad, cov.grad):
        assert torch.count_nonzero(g).item() == 0
    clf = classify.GaussianClassifier(mu.detach(), cov.detach())
    assert torch.count_nonzero(clf.label_log_proba(Z.detach(), y)).item() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[2], CASES[7], CASES[8], CASES[10], CASES[-2], CASES[-1]], ids=_ids)
def test_bits_do_not_depend_on_the_run_or_on_the_gradients_asked_for(case, dtype):
    from sqfa_amd import classify
    ref = _reference(case, dtype)
    bits = lambda t: t.view(torch.int32 if dtype == torch.float32 else torch.int64)

    def run(subset):
        Z, y, mu, cov, w = _device_inputs(ref, dtype, subset)
        loss = classify.gaussian_log_loss(Z, y, mu, cov, w)
        (UPSTREAM * loss).backward()
        return loss.detach(), Z.grad, None if mu is None else mu.grad, cov.grad

    full, again = run((True, True, True)), run((True, True, True))
    for a, b in zip(full, again):
        assert a is None and b is None or torch.equal(bits(a), bits(b))
    for i, subset in enumerate([(True, False, False), (False, True, False), (False, False, True)]):
        if full[i + 1] is None:
            continue   # zero means: no gradient of the means to ask for
        part = run(subset)
        assert torch.equal(bits(part[0]), bits(full[0]))
        assert torch.equal(bits(part[i + 1]), bits(full[i + 1]))
        assert all(part[k + 1] is None for k in range(3) if k != i)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bad_labels_and_samples_are_refused_and_the_process_stays_healthy(dtype):
    from sqfa_amd import classify
    case = (9, 5, 200, 1.0, True, True)
    ref = _reference(case, dtype)
    Z, y, mu, cov, w = _device_inputs(ref, dtype)
    clf = classify.GaussianClassifier(mu.detach(), cov.detach(), w)
    calls = [lambda Z, y: classify.gaussian_log_loss(Z, y, mu, cov, w), clf.label_log_proba, clf.log_loss]
    bad = y.clone()
    bad[[0, 63, 64, 199]] = torch.tensor([-1, 9, 2 ** 40, -2 ** 62], device=DEV)
    zero = y.clone()
    zero[[5, 70]] = torch.tensor([2, 8], device=DEV)   # the classes of prior 0
    Zn = Z.detach().clone()
    Zn[[0, 63, 64], [0, 1, 4]] = float("nan")
    for call in calls:
        with pytest.raises(ValueError, match=r"4 labels are outside \[0, 9\)"):
            call(Z, bad)
        with pytest.raises(ValueError, match="2 labels belong to a class with prior 0"):
            call(Z, zero)
        with pytest.raises(ValueError, match="3 samples have non-finite scores"):
            call(Zn, y)
        with pytest.raises(ValueError, match="labels must be integers"):
            call(Z, y.double())
        with pytest.raises(ValueError, match="labels must be integers"):
            call(Z, y[:-1])
    broken = cov.detach().clone()
    broken[1] = -broken[1]
    with pytest.raises(ValueError, match="1 of 9 classes"):
        classify.gaussian_log_loss(Z, y, mu, broken, w)
    # the three counts of one call, and its loss
    W, offset = clf._factors
    value, _, _, flags = classify._native_log_loss(Zn.contiguous(), bad, clf._means_native, W, offset)
    assert flags.tolist() == [3, 4, 0] and torch.isnan(value).all()
    value, _, _, flags = classify._native_log_loss(Z.detach().contiguous(), zero, clf._means_native, W, offset)
    assert flags.tolist() == [0, 0, 2] and torch.isnan(value).all()
    # a following valid call gives the oracle's result
    loss = classify.gaussian_log_loss(Z, y, mu, cov, w)
    (UPSTREAM * loss).backward()
    _check(loss.item(), ref, "loss", dtype, gradient=False)
    _check(Z.grad, ref, "gZ", dtype, gradient=True)
    _check(mu.grad, ref, "gmu", dtype, gradient=True)
    _check(cov.grad, ref, "gcov", dtype, gradient=True)


def test_the_native_path_is_taken_and_carries_gradients_to_leaves(monkeypatch):
    from sqfa_amd import classify
    ref = _reference((9, 5, 200, 1.0, True, False), torch.float64)
    Z, y, mu, cov, w = _device_inputs(ref, torch.float64, (False, False, False))

    def refuse(self):
        raise AssertionError("the torch factor path ran")

    monkeypatch.setattr(classify.GaussianClassifier, "_torch_factors", refuse)
    A = torch.randn(5, 5, dtype=torch.float64, device=DEV, requires_grad=True)   # a leaf behind every input
    loss = classify.gaussian_log_loss(Z @ A, y, mu @ A, A.T @ cov @ A, w)
    loss.backward()
    assert A.grad is not None and torch.isfinite(A.grad).all() and A.grad.abs().max() > 0
    clf = classify.GaussianClassifier(mu, cov)
    assert clf.log_loss(Z, y) > 0 and clf.label_log_proba(Z, y).shape == (200,)
    # the switch: the torch expression, which the patched factor path refuses
    monkeypatch.setattr(classify, "NATIVE_LOG_LOSS", False)
    with pytest.raises(AssertionError, match="torch factor path"):
        classify.gaussian_log_loss(Z.requires_grad_(), y, mu, cov, w)
    monkeypatch.undo()
    monkeypatch.setattr(classify, "NATIVE_LOG_LOSS", False)
    off = classify.gaussian_log_loss(Z, y, mu, cov, w)
    monkeypatch.undo()
    on = classify.gaussian_log_loss(Z, y, mu, cov, w)
    assert abs(on.item() - off.item()) <= 1e-10 * (1 + abs(off.item()))
    # K = 65: the torch expression, on the GPU
    Zb, yb, mub, covb = classify_oracle.problem(3, 65, 40, 1.0, seed=9)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)
    big = classify.gaussian_log_loss(t(Zb).requires_grad_(), torch.tensor(yb, device=DEV), t(mub), t(covb))
    want = log_loss_oracle.evaluate(Zb, yb, mub, covb)["loss"]
    assert big.requires_grad and abs(big.item() - want) <= 1e-10 * (1 + abs(want))


def test_nothing_of_size_n_by_c_is_formed():
    from sqfa_amd import _lib, classify
    C, K, N = 257, 16, 4096
    Z, labels, mu, cov = classify_oracle.problem(C, K, N, 1.0, seed=1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    Zt, y, mut, covt = t(Z).requires_grad_(), torch.tensor(labels, device=DEV), t(mu).requires_grad_(), t(cov).requires_grad_()
    classify.gaussian_log_loss(Zt[:64], y[:64], mut, covt).backward()   # the library and the allocator are warm
    Zt.grad = mut.grad = covt.grad = None
    lib = _lib.load()
    ws = max(lib.sqfa_gauss_log_loss_workspace_bytes(N, C, K, _lib.SQFA_F32),
             lib.sqfa_gauss_log_loss_backward_workspace_bytes(N, C, K, _lib.SQFA_F32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    classify.gaussian_log_loss(Zt, y, mut, covt).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    # the workspace, the factors and grad_cov (C, K, K), Z's copy and gradient (N, K), a few (N,) and (C,) vectors
    allowed = ws + 3 * C * K * K * 4 + 3 * N * K * 4 + 4 * N * 8 + (1 << 20)
    print(f"loss and gradients at (C, K, N) = ({C}, {K}, {N}): peak rise {rise} bytes, workspace {ws}, allowed {allowed}, "
          f"(N, C) float32 {N * C * 4}")
    assert rise < allowed and allowed < N * C * 4 + ws


@pytest.mark.parametrize("second_moments", [False, True], ids=["SQFA", "SecondMomentsSQFA"])
def test_feature_log_loss_matches_the_cpu(second_moments):
    """(C, D, K, N) = (5, 32, 4, 300) in float64: the value and the filter gradient on the GPU (native log-loss, the
    model's native backward paths) against the CPU (torch expressions throughout), to 1e-9 as
    test_gpu_classify.test_from_model_on_a_fitted_sqfa holds the scores: float64 rounding through F S F^T, a Cholesky
    factor of condition 10^2 and sums over 300 samples stays orders of magnitude below."""
    import copy

    import sqfa_amd
    from sqfa_amd import classify
    C, D, K, N = 5, 32, 4, 300
    g = torch.Generator().manual_seed(0)
    centres = 0.7 * torch.randn(C, D, generator=g, dtype=torch.float64)
    mix = torch.randn(C, D, D, generator=g, dtype=torch.float64) / D ** 0.5
    y = torch.arange(N) % C
    X = centres[y] + torch.einsum("nij,nj->ni", mix[y], torch.randn(N, D, generator=g, dtype=torch.float64))
    torch.manual_seed(1)
    cls = sqfa_amd.model.SecondMomentsSQFA if second_moments else sqfa_amd.model.SQFA
    cpu = cls(n_dim=D, n_filters=K, feature_noise=0.01).double()
    gpu = copy.deepcopy(cpu).to(DEV)
    want = classify.feature_log_loss(cpu, X, y)
    g_want, = torch.autograd.grad(want, list(cpu.parameters()))
    got = classify.feature_log_loss(gpu, X.to(DEV), y.to(DEV))
    g_got, = torch.autograd.grad(got, list(gpu.parameters()))
    err_v, err_g = abs(got.item() - want.item()), (g_got.cpu() - g_want).abs().max().item()
    print(f"feature_log_loss: value error {err_v:.3e}, filter gradient error {err_g:.3e} of {g_want.abs().max().item():.3e}")
    assert got.is_cuda and err_v <= 1e-9 * (1 + abs(want.item()))
    assert err_g <= 1e-9 * g_want.abs().max().item()
    losses, _ = classify.fit_log_loss(gpu, X.to(DEV), y.to(DEV), max_epochs=3)
    assert classify.feature_log_loss(gpu, X.to(DEV), y.to(DEV)).item() < want.item() and len(losses) >= 1
