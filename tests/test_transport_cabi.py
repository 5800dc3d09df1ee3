"""CPU tests of the Bures-Wasserstein feature (sqfa_amd.transport, sqfa_bw_pairwise): exported symbols and bindings,
host-side argument validation and workspace bounds, the module's public names and fused spec, the refusal of CPU
tensors, and the float64 numpy oracle of tests/bw_oracle.py against central differences."""
import ctypes

import numpy as np
import pytest
import torch

import bw_oracle
import sqfa_amd
from sqfa_amd import _lib, distances, transport

NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in ("sqfa_bw_pairwise", "sqfa_bw_workspace_bytes", "sqfa_bw_workspace_bytes_sharded"):
        assert name in _lib.PROTOTYPES
        fn = getattr(lib, name)
        assert fn.restype is _lib.PROTOTYPES[name][0]
    assert len(_lib.PROTOTYPES["sqfa_bw_pairwise"][1]) == 21
    assert lib.sqfa_hip_max_dim() == 128


def _call(lib, A=1, nA=4, B=None, nB=0, m=8, dtype=_lib.SQFA_F32, shard=(0, 1), ws=1, ws_bytes=1 << 20):
    dummy = ctypes.c_void_p(0x1000)
    return lib.sqfa_bw_pairwise(dummy if A else NULL, nA, B if B is not None else NULL, nB, m, dtype, 1e-6, 1,
                                NULL, -1.0, shard[0], shard[1], NULL, NULL, NULL, NULL, None,
                                dummy if ws else NULL, ws_bytes, NULL, None)


def test_argument_validation(lib):
    assert _call(lib, m=0) == -1                      # m < 1 is a bad size argument, as for sqfa_airm_pairwise
    assert _call(lib, m=129) == -2                    # SQFA_ERR_UNSUPPORTED_M
    assert _call(lib, A=0) == -1
    assert _call(lib, ws=0) == -1
    assert _call(lib, dtype=7) == -1
    assert _call(lib, nA=1) == -1                     # self mode needs two classes
    assert _call(lib, shard=(2, 2)) == -1
    assert _call(lib, B=ctypes.c_void_p(0x2000), nB=0) == -1
    assert _call(lib, ws_bytes=16) == -3              # SQFA_ERR_WORKSPACE
    assert _call(lib, m=100, ws_bytes=16) == -3       # the LDS range is supported


@pytest.mark.parametrize("m", [1, 4, 16, 17, 33, 48, 64, 65, 96, 128])
@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_bounds(lib, m, dtype):
    C = 50
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for nB in (0, 30):
        full = lib.sqfa_bw_workspace_bytes(C, nB, m, dtype)
        airm = lib.sqfa_airm_workspace_bytes(C, nB, m, dtype)
        nBe = nB or C
        # at least the affine-invariant workspace plus S^-1, G, W (3 m^2 doubles per B class)
        assert full >= airm + 3 * nBe * m * m * 8
        assert full < airm + 3 * nBe * m * m * 8 + 64 * (C + 1) * (nBe + 64) * 8 + (1 << 20)
        for shards in (1, 2, 8):
            for pol in (-1, 0, 1):
                sh = lib.sqfa_bw_workspace_bytes_sharded(C, nB, m, dtype, shards, pol)
                assert 0 < sh <= full
        assert esz in (4, 8)
    assert lib.sqfa_bw_workspace_bytes(C, 0, 129, dtype) == 0
    assert lib.sqfa_bw_workspace_bytes(C, 0, 0, dtype) == 0


def test_module_names_and_fused_spec():
    assert "transport" in sqfa_amd.__all__
    assert set(transport.__all__) == {"bures_wasserstein_sq", "bures_wasserstein", "wasserstein_sq", "wasserstein"}
    assert distances.fused_spec(transport.bures_wasserstein) == ("spd", 1.0, True, "bw")
    assert distances.fused_spec(transport.bures_wasserstein_sq) == ("spd", 1.0, False, "bw")
    assert distances.fused_spec(transport.wasserstein) is None
    assert distances.fused_spec(distances.affine_invariant) == ("spd", 1.0, True, "airm")
    assert "bures_wasserstein" not in distances.__all__


def test_cpu_tensors_refused():
    A = torch.eye(3, dtype=torch.float64).expand(4, 3, 3).contiguous()
    for fn in (transport.bures_wasserstein, transport.bures_wasserstein_sq):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(A, A)
    stats = {"means": torch.zeros(4, 3, dtype=torch.float64), "covariances": A}
    for fn in (transport.wasserstein, transport.wasserstein_sq):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(stats, stats)


def _spd(rng, m, kappa=10.0):
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    return (Q * np.geomspace(1.0, kappa, m)) @ Q.T


def test_oracle_sanity():
    m = 4
    I = np.eye(m)
    assert abs(bw_oracle.bw2(I, I)) < 1e-12
    s = 2.5
    assert np.allclose(bw_oracle.transport_map(s * I, I), s ** -0.5 * I)
    ga, gb = bw_oracle.bw2_grads(I, I)
    assert np.abs(ga).max() < 1e-12 and np.abs(gb).max() < 1e-12


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_gradients_central_differences(seed):
    rng = np.random.default_rng(seed)
    m = 5
    A, B = _spd(rng, m), _spd(rng, m, 30.0)
    ga, gb = bw_oracle.bw2_grads(A, B)
    h = 1e-6
    for which, g in (("A", ga), ("B", gb)):
        num = np.zeros((m, m))
        for r in range(m):
            for c in range(r, m):
                E = np.zeros((m, m))
                E[r, c] = E[c, r] = h  # symmetric perturbation: d/dt f(X + tE) = <G, E>
                Xp = (A + E, B) if which == "A" else (A, B + E)
                Xm = (A - E, B) if which == "A" else (A, B - E)
                d = (bw_oracle.bw2(*Xp) - bw_oracle.bw2(*Xm)) / (2 * h)
                num[r, c] = num[c, r] = d if r == c else d / 2
        assert np.abs(num - g).max() < 3e-7 * max(1.0, np.abs(g).max())


def test_oracle_values_match_the_tutorial_expression():
    """bw2 via eigh agrees with the tutorial's torch expression (spd_sqrt + conjugation + eigvalsh), CPU float64."""
    rng = np.random.default_rng(3)
    A = np.stack([_spd(rng, 6) for _ in range(3)])
    B = np.stack([_spd(rng, 6, 100.0) for _ in range(2)])
    At, Bt = torch.tensor(A), torch.tensor(B)
    from sqfa_amd import linalg
    tr_A = torch.einsum("ijj->i", At)
    tr_B = torch.einsum("ijj->i", Bt)
    C = linalg.conjugate_matrix(Bt, linalg.spd_sqrt(At))
    tut = (tr_A[None, :] + tr_B[:, None] - 2 * torch.sqrt(torch.linalg.eigvalsh(C)).sum(-1)).numpy()  # (nB, nA)
    D, _, _ = bw_oracle.pairwise(A, B, sqrt_mode=False)
    assert np.abs(D - tut.T).max() < 1e-10
