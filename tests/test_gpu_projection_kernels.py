"""The projection-side closure kernels, each called straight through the C ABI on every dispatch variant, against the
float64 definition in tests/projection_oracle.py (pinned without a GPU by tests/test_projection_oracle.py).

Every output lives inside a larger buffer: payload pre-filled with NaN, margins with a sentinel; the payload must come back
finite, the margins untouched, and a second call bitwise equal.  Inputs are seeded and rounded to the dtype under test
before the oracle sees them.  The comparison is elementwise, |out - ref| <= 2 n u mag (projection_oracle.ratio() <= 2), n
the number of terms summed into the element and mag the expression with every term replaced by its absolute value; the
largest observed error / (n u mag) of each test is recorded (record_property "max_ratio").

Misaligned operands are made by slicing one element into a buffer one element too long (data_ptr() % 16 == 4 or 8), and
only for operands whose launcher checks the pointer and falls back: F of the forward product, T and G of the backward
product, T_out of the projection.  Psi is never misaligned here: sqfa_project_scatters refuses it with a status code
(tests/test_cabi.py), nothing is launched.

Launcher branch -> parametrization that takes it:

  launch_project / launch_project_w (project_kernel.hip), test_project
    NB = 1 / 2 / 3 / 4 (KC 128 / 64 / 32 / 32)   K in {1, 3, 4, 16} / {17, 20} / {33, 48} / {49, 64}
    16-byte T_out stores                         K % 4 == 0 with mis_out = 0;  scalar stores: K in {1, 3, 17, 33, 49}, or mis_out = 1
    D < KC, ragged last chunk (clamped row)      f32 D = 4 ... 68, 132 (K <= 16: KC = 128), 1028, 2052;  f64 D = 4, 36, 516, 1028
    ragged last stripe (clamped column)          f32 D = 4 ... 20, 68, 132, 1028, 2052;  f64 D = 4, 36, 516, 1028
    idle waves                                   every D below WV stripes: f32 D <= 1020 with WV = 16, D = 1028 (17 of 24), 2052 (33 of 36)
    nstripes <= 16 -> WV 16                      f32 D <= 1024;  f64 D <= 512
    nstripes <= 32 -> WV 8                       f32 D = 1028, 2048;  f64 D = 516, 1024
    else WV 4                                    f32 D = 2052;  f64 D = 1028
    K == D                                       (D, K) = (4, 4), (20, 20), (64, 64) f32;  (4, 4) f64

  launch_forward / SQFA_FWD (feature_kernels.hip), test_feature_scatters_ex
    NB = 1 / 2 / 3 / 4 (SPLIT 8 / 4 / 2 / 2)     K in {1, 15, 16} / {17, 32} / {33, 48} / {49, 63, 64}
    FV = true                                    D >= 16 with mis_f = 0
    FV = false, D < 16                           D in {4, 8, 12}
    FV = false, D >= 16 (misaligned F)           D in {16, ..., 144} with mis_f = 1
    groups < SPLIT (idle parts)                  D in {16, ..., 32} (1 or 2 groups), D = 4 ... 28 scalar steps < SPLIT at NB = 1
    D % 16 tail of 0 / 1 / 2 / 3 steps           D in {16, 32, 144} / {20, 132} / {8, 24} / {12, 28}
    epilogue: noise, border, corner, pitch K+1   noise in {0, 0.01} x means in {NULL, given}, all of the above

  launch_backward (feature_kernels.hip), test_feature_scatters_backward_ex, for NB = 1 / 2 / 3 / 4:
    TV SYM GV       K in {16 / 32 / 48 / 64}, ldg = K, sym = 1, nothing misaligned
    TV SYM          the same K with ldg = K + 1, or mis_g = 1
    TV              the same K with sym = 0 (any ldg)
    SYM             K in {1, 15 / 17 / 33 / 49} (K % 4 != 0), or K % 4 == 0 with mis_t = 1; sym = 1
    none            the same with sym = 0

  closure_glue.hip: test_sphere_forward, test_sphere_backward (one to four trips of the 256-thread loops: D = 1 ... 784;
    n_groups = 0 with extra only, every remainder of the 4-way unrolled sum: 1, 3, 4, 5, 7, 8, 64; norms / extra / gloss
    each NULL and given), test_embed_backward_means (more rows than the 64 threads never: K <= 64; K = 1 ... 64, C up to 70).

  test_chain: _native.closure_stage_project + closure_stage_backward (Sphere / Identity / orthogonal base, with and without
    means, K + 1 = 2 ... 65) against projection_oracle.stage (torch autograd on the plain float64 expression).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import projection_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 64           # elements on either side of an output (a multiple of 16 bytes in both dtypes)
SENTINEL = 777.25
DTYPES = ["f32", "f64"]
NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}


def _lib():
    from sqfa_amd import _lib as L
    return L


def _code(dt):
    return _lib().SQFA_F32 if dt == "f32" else _lib().SQFA_F64


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dt, mis=0):
    """Device tensor of the dtype under test holding `a`; mis = 1: one element into a buffer one element too long."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + mis, dtype=TORCH[dt], device=DEV)
    view = buf[mis:].view(a.shape)
    view.copy_(torch.from_numpy(a).to(TORCH[dt]))
    assert view.is_contiguous() and view.data_ptr() % 16 == (0 if not mis else buf.element_size())
    return view


class Guarded:
    """An output of `shape` inside a larger buffer: NaN payload between sentinel margins."""

    def __init__(self, shape, dt, mis=0):
        n = int(np.prod(shape))
        self.buf = torch.full((2 * MARGIN + n + mis,), SENTINEL, dtype=TORCH[dt], device=DEV)
        self.lo = MARGIN + mis
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == (0 if not mis else self.buf.element_size())

    def take(self):
        """The payload as float64 numpy, after checking it is finite and the margins are untouched; payload reset to NaN."""
        torch.cuda.synchronize()
        n = self.view.numel()
        assert bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + n:] == SENTINEL).all()), \
            "write outside the output"
        assert bool(torch.isfinite(self.view).all()), "an output element was not written (or is not finite)"
        out = self.view.detach().cpu().clone()
        self.view.fill_(float("nan"))
        return out


def run_twice(launch, *outs):
    """Launch, collect, launch again: both results bitwise equal.  Returns the float64 numpy payloads."""
    first = None
    for _ in range(2):
        launch()
        got = [o.take() for o in outs]
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert torch.equal(a, b), "two calls differ"
    return [g.double().numpy() for g in first]


def check(out, val, dt, worst):
    r = po.ratio(out, val, NP[dt])
    worst.append(r)
    assert r <= po.C_FACTOR, f"error / (n u magnitude) = {r:.3g} > {po.C_FACTOR}"


# ---- sqfa_project_scatters ----------------------------------------------------------------------------------------

K_ALL = [1, 3, 4, 16, 17, 20, 33, 48, 49, 64]
PROJECT_CASES = (
    [("f32", D, K) for D in (4, 8, 12, 20, 64, 68, 132) for K in K_ALL if K <= D]
    + [("f32", 1024, 16), ("f32", 1024, 49), ("f32", 1028, 3), ("f32", 1028, 33), ("f32", 2048, 4), ("f32", 2048, 64),
       ("f32", 2052, 17), ("f32", 2052, 20)]
    + [("f64", D, K) for D in (4, 36) for K in K_ALL if K <= D]
    + [("f64", 512, 16), ("f64", 512, 49), ("f64", 516, 3), ("f64", 516, 33), ("f64", 1024, 4), ("f64", 1024, 64),
       ("f64", 1028, 17), ("f64", 1028, 20)]
)


@functools.lru_cache(maxsize=4)
def _project_reference(dt, D, K):
    C = 3 if D <= 132 else 2
    c = po.case_project(C, D, K, NP[dt])
    return c, po.project(c["Psi"], c["F"])


@pytest.mark.parametrize("dt,D,K", PROJECT_CASES)
def test_project(dt, D, K, record_property):
    lib = _lib().load()
    c, ref = _project_reference(dt, D, K)
    C = c["Psi"].shape[0]
    Psi, F = dev(c["Psi"], dt), dev(c["F"], dt)
    assert Psi.data_ptr() % 16 == 0
    worst = []
    for mis_out in (0, 1):
        out = Guarded((C, D, K), dt, mis_out)
        launch = lambda: _lib().check(lib.sqfa_project_scatters(_ptr(F), K, D, _ptr(Psi), C, _code(dt), _ptr(out.view),
                                                                _stream()), "sqfa_project_scatters")
        (T,) = run_twice(launch, out)
        check(T, ref, dt, worst)
    record_property("max_ratio", max(worst))


# ---- sqfa_feature_scatters_ex -------------------------------------------------------------------------------------

FWD_K = [1, 15, 16, 17, 32, 33, 48, 49, 63, 64]
FWD_D = [4, 8, 12, 16, 20, 24, 28, 32, 132, 144]


@functools.lru_cache(maxsize=4)
def _forward_case(dt, C, D, K):
    return po.case_forward(C, D, K, NP[dt])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", FWD_D)
@pytest.mark.parametrize("K", FWD_K)
def test_feature_scatters_ex(K, D, dt, record_property):
    """C = 3 everywhere, and C = 1 as well at D in {4, 20, 144}."""
    lib = _lib().load()
    worst = []
    for C in ((1, 3) if D in (4, 20, 144) else (3,)):
        c = _forward_case(dt, C, D, K)
        T, m = dev(c["T"], dt), dev(c["m"], dt)
        for noise in (0.0, 0.01):
            for means in (None, m):
                ref = po.feature_scatters(c["F"], c["T"], float(po.rounded(noise, NP[dt])), None if means is None else c["m"])
                ld = K if means is None else K + 1
                for mis_f in (0, 1):
                    F = dev(c["F"], dt, mis_f)
                    out = Guarded((C, ld, ld), dt)
                    launch = lambda: _lib().check(lib.sqfa_feature_scatters_ex(_ptr(F), K, D, _ptr(T), C, _code(dt), noise,
                                                                               _ptr(means), _ptr(out.view), _stream()),
                                                  "sqfa_feature_scatters_ex")
                    (S,) = run_twice(launch, out)
                    check(S, ref, dt, worst)
                    if means is not None:      # border and corner are copies
                        assert np.array_equal(S[:, :K, K], c["m"]) and np.array_equal(S[:, K, :K], c["m"])
                        assert (S[:, K, K] == 1).all()
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,D", [(1, 4), (16, 20), (33, 132), (64, 144)])
def test_feature_scatters_plain_entry(K, D, dt, record_property):
    lib = _lib().load()
    c = _forward_case(dt, 3, D, K)
    ref = po.feature_scatters(c["F"], c["T"], 0.0)
    F, T = dev(c["F"], dt), dev(c["T"], dt)
    out = Guarded((3, K, K), dt)
    launch = lambda: _lib().check(lib.sqfa_feature_scatters(_ptr(F), K, D, _ptr(T), 3, _code(dt), _ptr(out.view), _stream()),
                                  "sqfa_feature_scatters")
    (S,) = run_twice(launch, out)
    worst = []
    check(S, ref, dt, worst)
    record_property("max_ratio", max(worst))


# ---- sqfa_feature_scatters_backward_ex ----------------------------------------------------------------------------

BWD_K = [1, 15, 16, 17, 32, 33, 48, 49, 64]
BWD_C = 3


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [4, 16, 40, 132])
@pytest.mark.parametrize("K", BWD_K)
def test_feature_scatters_backward_ex(K, D, dt, record_property):
    """Each partial sum against the oracle's group sum; groups without a class are exact zeros (n = 0 in the oracle)."""
    lib = _lib().load()
    C = BWD_C
    worst = []
    for ldg in (K, K + 1):
        for sym in (0, 1):
            c = po.case_backward(C, D, K, ldg, bool(sym), NP[dt])
            refs = {n: po.backward_partials(c["G"], c["T"], n) for n in (1, 3, C + 2)}    # C == 3
            for mis_t, mis_g in ((0, 0), (1, 0), (0, 1)):
                T, G = dev(c["T"], dt, mis_t), dev(c["G"], dt, mis_g)
                for n_groups in (1, 3, C, C + 2):
                    out = Guarded((n_groups, K, D), dt)
                    launch = lambda: _lib().check(
                        lib.sqfa_feature_scatters_backward_ex(_ptr(G), ldg, _ptr(T), C, D, K, _code(dt), n_groups, sym,
                                                              _ptr(out.view), _stream()), "sqfa_feature_scatters_backward_ex")
                    (P,) = run_twice(launch, out)
                    check(P, refs[n_groups], dt, worst)
                    assert not P[C:].any()
    record_property("max_ratio", max(worst))


def test_feature_scatters_backward_plain_entry(record_property):
    lib = _lib().load()
    C, D, K, dt = 5, 40, 17, "f32"
    c = po.case_backward(C, D, K, K, False, NP[dt])
    T, G = dev(c["T"], dt), dev(c["G"], dt)
    out = Guarded((2, K, D), dt)
    launch = lambda: _lib().check(lib.sqfa_feature_scatters_backward(_ptr(G), _ptr(T), C, D, K, _code(dt), 2, _ptr(out.view),
                                                                     _stream()), "sqfa_feature_scatters_backward")
    (P,) = run_twice(launch, out)
    worst = []
    check(P, po.backward_partials(c["G"], c["T"], 2), dt, worst)
    record_property("max_ratio", max(worst))


# ---- sqfa_sphere_forward / sqfa_sphere_backward / sqfa_embed_backward_means ------------------------------------------

SPHERE_D = [1, 4, 255, 256, 257, 784]
SPHERE_GROUPS = [0, 1, 3, 4, 5, 7, 8, 64]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", SPHERE_D)
@pytest.mark.parametrize("K", [1, 3])
def test_sphere_forward(K, D, dt, record_property):
    lib = _lib().load()
    c = po.case_sphere(K, D, 0, NP[dt])
    Fref, nref = po.sphere_forward(c["X"])
    X = dev(c["X"], dt)
    F, norms = Guarded((K, D), dt), Guarded((K,), dt)
    launch = lambda: _lib().check(lib.sqfa_sphere_forward(_ptr(X), K, D, _code(dt), _ptr(F.view), _ptr(norms.view), _stream()),
                                  "sqfa_sphere_forward")
    Fo, no = run_twice(launch, F, norms)
    worst = []
    check(no, nref, dt, worst)
    record_property("max_ratio_norms", worst[-1])
    check(Fo, Fref, dt, worst)
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", SPHERE_D)
@pytest.mark.parametrize("K", [1, 3])
def test_sphere_backward(K, D, dt, record_property):
    lib = _lib().load()
    worst = []
    for n_groups in SPHERE_GROUPS:
        c = po.case_sphere(K, D, n_groups, NP[dt])
        X, norms, partials, extra = (dev(c[k], dt) for k in ("X", "norms", "partials", "extra"))
        gloss = dev(np.array([c["gloss"]]), dt)
        for use_norms in (True, False):
            for use_extra in (True, False):
                for use_gloss in (True, False):
                    ref = po.sphere_backward(c["X"], c["norms"] if use_norms else None, c["partials"],
                                             c["extra"] if use_extra else None, c["gloss"] if use_gloss else None)
                    out = Guarded((K, D), dt)
                    launch = lambda: _lib().check(
                        lib.sqfa_sphere_backward(_ptr(X), _ptr(norms if use_norms else None), K, D, _code(dt), _ptr(partials),
                                                 n_groups, _ptr(extra if use_extra else None), _ptr(gloss if use_gloss else None),
                                                 _ptr(out.view), _stream()), "sqfa_sphere_backward")
                    (g,) = run_twice(launch, out)
                    check(g, ref, dt, worst)
    record_property("max_ratio", max(worst))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [1, 3, 70])
@pytest.mark.parametrize("K", [1, 5, 16, 63, 64])
def test_embed_backward_means(K, C, dt, record_property):
    """A general, non-symmetric gE."""
    lib = _lib().load()
    c = po.case_embed(C, K, NP[dt])
    assert K == 1 or not np.array_equal(c["gE"], c["gE"].transpose(0, 2, 1))
    gE, m = dev(c["gE"], dt), dev(c["m"], dt)
    out = Guarded((C, K), dt)
    launch = lambda: _lib().check(lib.sqfa_embed_backward_means(_ptr(gE), _ptr(m), C, K, _code(dt), _ptr(out.view), _stream()),
                                  "sqfa_embed_backward_means")
    (gm,) = run_twice(launch, out)
    worst = []
    check(gm, po.embed_backward_means(c["gE"], c["m"]), dt, worst)
    record_property("max_ratio", max(worst))


# ---- the chain ----------------------------------------------------------------------------------------------------

CHAIN_SHAPES = [(1, 8), (17, 68), (33, 132), (64, 132)]
CHAIN_C = 3


@functools.lru_cache(maxsize=2)
def _chain_reference(dt, K, D, kind, with_means):
    c = po.case_chain(K, D, CHAIN_C, kind, with_means, NP[dt])
    st = po.stage(c["X"], c["Psi"], c["means"], c["noise"], c["base"] if kind == "orthogonal" else kind, c["gS"], c["gloss"])
    return c, st


def _run_chain(c, dt, kind, out_S=None):
    from sqfa_amd import _native
    X, Psi, means, gS = (dev(c[k], dt) for k in ("X", "Psi", "means", "gS"))
    sphere = {"sphere": True, "identity": False}.get(kind)
    if sphere is None:
        sphere = dev(c["base"], dt)
    st = _native.closure_stage_project(X, Psi, means, c["noise"], sphere, out_S=out_S)
    grad = _native.closure_stage_backward(st, gS, torch.tensor(c["gloss"], dtype=TORCH[dt], device=DEV))
    torch.cuda.synchronize()
    return st["S"].detach().cpu().clone(), grad.detach().cpu().clone()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("with_means", [False, True])
@pytest.mark.parametrize("kind", po.CHAIN_KINDS)
@pytest.mark.parametrize("K,D", CHAIN_SHAPES)
def test_chain(K, D, kind, with_means, dt, record_property):
    """closure_stage_project + closure_stage_backward for a random symmetric upstream gradient and gloss = 3 against the
    stage oracle: S | E, and dL/dX from torch autograd on the plain float64 expression."""
    c, st = _chain_reference(dt, K, D, kind, with_means)
    S1, g1 = _run_chain(c, dt, kind)
    S2, g2 = _run_chain(c, dt, kind)
    assert torch.equal(S1, S2) and torch.equal(g1, g2)
    worst = []
    check(S1.double().numpy(), st["out"], dt, worst)
    record_property("max_ratio_S", worst[-1])
    check(g1.double().numpy(), po.Val(st["dX_autograd"], st["dX"].mag, st["dX"].n), dt, worst)
    record_property("max_ratio", max(worst))
    if kind == "orthogonal":     # exactly zero on and above the diagonal of X^T, as torch returns
        assert (g1.numpy()[np.tril_indices(K, 0, D)] == 0).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_chain_writes_into_a_given_buffer(dt, record_property):
    """out_S given (the slice of an all-gather buffer in a class-sharded evaluation): same values, nothing around it."""
    K, D = 17, 68
    c, st = _chain_reference(dt, K, D, "sphere", True)
    out = Guarded((CHAIN_C, K + 1, K + 1), dt)
    _, grad = _run_chain(c, dt, "sphere", out_S=out.view)
    S = out.take().double().numpy()
    worst = []
    check(S, st["out"], dt, worst)
    check(grad.double().numpy(), po.Val(st["dX_autograd"], st["dX"].mag, st["dX"].n), dt, worst)
    record_property("max_ratio", max(worst))
