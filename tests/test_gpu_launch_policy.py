"""sqfa_airm_options::launch_policy: a call made of the fused launches (0, the default) and the same call made of the separate
launches (-1) return the same BITS -- loss, both flags, both gradients, distances and eigenvalues.  The fused class prologue
(class_prologue_kernel: Cholesky factor, inverse, slab slot table and the class factor pass of the A side in one launch) is
the fused launch there is; the factor pass is forced on (class_factor=1), otherwise calls this small never reach it.

The fused launch exists on the rows up to m = 24 whose geometry has a factor pass (padded sizes 12, 16, 17, 20, 24, both element
types).  m=8 (no factor pass) and m=32 (above the limit) take the separate launches under either policy: their cases are
the issue's and pin that the policy changes nothing there, they cannot tell the two kernels apart.

The shapes are the smallest at which the packing of classes into workgroups can go wrong: one tile, a last workgroup with one
class (C=17, C=37: lane groups past the last class sweep a copy of it), several tile rows, narrowed tiles, every padded size
with the kernel (m=12 one column per lane, m=17 a lone column, m=20 and m=24 the 32-lane-wide elimination; m=24 float64 runs on
a 2-D pair row), sizes below their padded size (m=14 on 16, m=19 on 20, m=22 on 24: the identity fill and every `< m` guard),
both element types, cross mode (the A side alone takes the fused launch) and both lane geometries of a size."""
import gc

import numpy as np
import pytest
import torch

from sqfa_amd._optim import _no_gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("loss", "nonfinite", "gradA", "gradB", "dist", "eig")


def spd(rng, n, m):
    X = rng.standard_normal((n, 2 * m + 3, m))
    return np.einsum("cnm,cnk->cmk", X, X) / (2 * m + 3) + 0.05 * np.eye(m)


def bits(t):
    """The tensor's bit pattern (NaNs compare like any other value)."""
    t = t.detach().contiguous()
    return t if not t.is_floating_point() else t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def assert_same_bits(a, b, what=""):
    for name in OUTPUTS:
        if a[name] is None or b[name] is None:
            assert a[name] is None and b[name] is None, f"{what}{name}"
            continue
        assert torch.equal(bits(a[name]), bits(b[name])), f"{what}{name} differs between the launch policies"


def run(A, B, launch, *, geometry=0, sqrt_mode=True, weights=None, want_grad=True, want_dist=True, want_eig=True):
    from sqfa_amd import _native
    with _native.policies(class_factor=1, launch=launch, geometry=geometry):
        return _native.hip_pair_backend(A, B, scale=0.5, eps=1e-6, sqrt_mode=sqrt_mode, weights=weights, uniform_weight=0.37,
                                        shard=(0, 1), want_loss=True, want_grad=want_grad, want_dist=want_dist, want_eig=want_eig)


SELF_SHAPES = [(16, 5, False), (16, 17, False), (16, 37, False), (12, 21, False), (17, 21, False), (32, 21, False), (8, 70, False),
               (16, 21, True),
               # the other rows with the kernel, and sizes below their padded size
               (14, 21, False), (19, 21, False), (20, 21, False), (22, 21, False), (24, 21, False),
               (12, 21, True), (14, 21, True), (17, 21, True), (20, 21, True), (24, 21, True)]


def _inputs(m, C, f64, seed=0):
    rng = np.random.default_rng(100 * m + C + seed)
    return torch.tensor(spd(rng, C, m), dtype=torch.float64 if f64 else torch.float32, device=DEV)


@pytest.mark.parametrize("geometry", [0, -1])
@pytest.mark.parametrize("m,C,f64", SELF_SHAPES)
def test_self_mode_fused_and_separate_launches_agree_exactly(m, C, f64, geometry):
    """geometry 0: the small-launch row of the size where it has one; -1: the regular row (what C=1000 runs on)."""
    A = _inputs(m, C, f64)
    old, new = run(A, None, -1, geometry=geometry), run(A, None, 0, geometry=geometry)
    assert old["nonfinite"].tolist() == [0, 0]
    assert_same_bits(new, old)


@pytest.mark.parametrize("nA,nB", [(19, 37), (37, 3)])
@pytest.mark.parametrize("m,f64", [(16, False), (17, False), (32, False), (16, True), (14, False), (24, False), (22, True)])
def test_cross_mode_fused_and_separate_launches_agree_exactly(m, f64, nA, nB):
    rng = np.random.default_rng(m + nA)
    dtype = torch.float64 if f64 else torch.float32
    A = torch.tensor(spd(rng, nA, m), dtype=dtype, device=DEV)
    B = torch.tensor(spd(rng, nB, m), dtype=dtype, device=DEV)
    old, new = run(A, B, -1), run(A, B, 0)
    assert old["nonfinite"].tolist() == [0, 0] and old["gradB"] is not None
    assert_same_bits(new, old)


@pytest.mark.parametrize("m,C,f64", SELF_SHAPES)
def test_output_flags_and_weights(m, C, f64):
    """No gradient; distances and eigenvalues with their diagonals; squared distances; per-pair weights."""
    A = _inputs(m, C, f64, seed=1)
    W = torch.tensor(np.random.default_rng(C).standard_normal((C, C)), dtype=A.dtype, device=DEV)
    for kw in (dict(want_grad=False, want_dist=False, want_eig=False), dict(want_grad=False), dict(sqrt_mode=False),
               dict(weights=W), dict(weights=W, sqrt_mode=False, want_eig=False)):
        assert_same_bits(run(A, None, 0, **kw), run(A, None, -1, **kw), what=f"{kw}: ")


@pytest.mark.parametrize("m,f64", [(16, False), (17, False), (32, False), (16, True), (14, False), (24, False)])
def test_non_spd_class(m, f64):
    """A class whose factorisation breaks down half-way: the same NaNs in the same places, the same flags, no fault."""
    rng = np.random.default_rng(m)
    C, bad = 21, 7
    A = spd(rng, C, m)
    w, Q = np.linalg.eigh(A[bad])
    w[m // 2] = -0.3
    A[bad] = (Q * w) @ Q.T
    A = torch.tensor(A, dtype=torch.float64 if f64 else torch.float32, device=DEV)
    old, new = run(A, None, -1), run(A, None, 0)
    assert old["nonfinite"].tolist()[0] == C - 1
    assert_same_bits(new, old)


@pytest.mark.parametrize("m,f64", [(16, False), (17, False), (32, False), (16, True)])
def test_fused_prologue_alone(m, f64):
    """launch_policy = SQFA_LAUNCH_FUSED_PROLOGUE selects the prologue by its own bit; the reserved bit changes nothing."""
    A = _inputs(m, 37, f64, seed=2)
    old = run(A, None, -1, geometry=-1)
    assert_same_bits(run(A, None, 1, geometry=-1), old)
    assert_same_bits(run(A, None, 2, geometry=-1), old)
    assert_same_bits(run(A, None, 3, geometry=-1), old)


def test_captured_call_replayed_on_changed_inputs():
    """The call inside a captured graph, replayed three times on new matrices: every replay equals the separate launches."""
    m, C = 16, 37
    A = _inputs(m, C, False, seed=3)
    run(A, None, 0)   # the library is loaded and the workspace query answered before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    # torch no longer collects garbage before a capture, and a cyclic collection inside one that finalises device
    # tensors or an older graph aborts the process (_optim._no_gc): collect now, none while the stream captures
    gc.collect()
    with _no_gc(), torch.cuda.graph(g):
        out = run(A, None, 0)
    for seed in (4, 5, 6):
        fresh = _inputs(m, C, False, seed=seed)
        A.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(out, run(fresh, None, -1), what=f"replay {seed}: ")
