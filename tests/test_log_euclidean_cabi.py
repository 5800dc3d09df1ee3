"""CPU tests of the fused log-Euclidean closure (sqfa_log_euclidean_pairwise_loss, _native.ClassPairLoss): exported
symbols and bindings, host-side argument validation (every code is returned before any HIP call, so no GPU is needed), the
workspace query, distances.class_fused_spec and the models' _has_fused_closure()."""
import ctypes
import os

import pytest
import torch

import sqfa_amd
from sqfa_amd import _lib, _native, distances

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in ("sqfa_log_euclidean_pairwise_loss", "sqfa_log_euclidean_workspace_bytes"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    assert len(_lib.PROTOTYPES["sqfa_log_euclidean_pairwise_loss"][1]) == 14
    assert _lib.PROTOTYPES["sqfa_log_euclidean_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "sqfa_log_euclidean_pairwise_loss(" in header and "sqfa_log_euclidean_workspace_bytes(" in header


def _call(lib, S=1, n=4, m=8, dtype=_lib.SQFA_F32, sqrt_mode=1, grad=1, ws=1, ws_bytes=1 << 24):
    return lib.sqfa_log_euclidean_pairwise_loss(FAKE if S else NULL, n, m, dtype, sqrt_mode, 1e-6, -1.0, FAKE,
                                                FAKE if grad else NULL, NULL, NULL, FAKE if ws else NULL, ws_bytes, NULL)


def test_argument_validation(lib):
    assert _call(lib, S=0) == -1
    assert _call(lib, n=1) == -1                       # at least one pair
    assert _call(lib, n=0) == -1
    assert _call(lib, m=0) == -1
    assert _call(lib, dtype=7) == -1
    assert _call(lib, dtype=-1) == -1
    assert _call(lib, sqrt_mode=2) == -1
    assert _call(lib, sqrt_mode=-1) == -1
    assert _call(lib, m=65) == -2                      # SQFA_ERR_UNSUPPORTED_M: the limit of sqfa_spd_function
    assert _call(lib, m=128) == -2
    assert _call(lib, ws_bytes=16) == -3               # SQFA_ERR_WORKSPACE
    assert _call(lib, ws=0) == -3
    assert _call(lib, m=64, ws_bytes=16) == -3         # 64 is supported: only the workspace is wrong
    assert _call(lib, sqrt_mode=0, grad=0, ws_bytes=16) == -3   # forward only passes the argument checks too
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):       # one byte short of the query
        need = lib.sqfa_log_euclidean_workspace_bytes(4, 8, dtype)
        assert _call(lib, dtype=dtype, ws_bytes=need - 1) == -3


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(lib, dtype):
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for m in (1, 3, 4, 16, 17, 33, 64):
        prev = 0
        for n in (2, 3, 10, 100, 1000, 1001):
            b = lib.sqfa_log_euclidean_workspace_bytes(n, m, dtype)
            assert b >= prev and b >= n * m * m * esz, (n, m)
            # the logarithms, their gradient, U and lambda in double, sqfa_spd_function's own: no (n,n) term
            assert b >= lib.sqfa_spd_function_workspace_bytes(n, m, dtype) + 2 * n * m * m * esz + n * m * (m + 1) * 8
            assert b < 6 * n * 64 * 64 * 8 + 64 * n + 8192
            prev = b
    assert lib.sqfa_log_euclidean_workspace_bytes(10, 64, dtype) > 0
    assert lib.sqfa_log_euclidean_workspace_bytes(10, 65, dtype) == 0
    assert lib.sqfa_log_euclidean_workspace_bytes(10, 0, dtype) == 0
    assert lib.sqfa_log_euclidean_workspace_bytes(1, 4, dtype) == 0
    assert lib.sqfa_log_euclidean_workspace_bytes(10, 4, 5) == 0


def test_spd_function_limit_unchanged(lib):
    assert lib.sqfa_spd_function_workspace_bytes(3, 65, _lib.SQFA_F32) == 0
    assert lib.sqfa_spd_function(FAKE, 3, 65, 0, 0, FAKE, FAKE, FAKE, FAKE, 1 << 24, NULL) == -2


def test_class_fused_specs_and_switch(monkeypatch):
    assert distances.LOG_EUCLIDEAN_FUSED_CLOSURE is True
    assert distances.class_fused_spec(distances.log_euclidean) == ("spd", True)
    assert distances.class_fused_spec(distances.log_euclidean_sq) == ("spd", False)
    for name in ("affine_invariant", "affine_invariant_sq", "fisher_rao_lower_bound", "bhattacharyya", "hellinger",
                 "mahalanobis", "fisher_rao_same_cov"):
        assert distances.class_fused_spec(getattr(distances, name)) is None, name
    assert distances.class_fused_spec(lambda A, B: None) is None
    # the registry of the pair-kernel operators does not know these two
    assert distances.fused_spec(distances.log_euclidean) is None
    assert distances.fused_spec(distances.log_euclidean_sq) is None
    assert distances.fused_spec(distances.affine_invariant) == ("spd", 1.0, True, "airm")
    monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", False)
    assert distances.class_fused_spec(distances.log_euclidean) is None
    assert distances.class_fused_spec(distances.log_euclidean_sq) is None
    assert distances.fused_spec(distances.affine_invariant) == ("spd", 1.0, True, "airm")


def test_models_follow_the_spec(monkeypatch):
    SM, SQ = sqfa_amd.model.SecondMomentsSQFA, sqfa_amd.model.SQFA
    for fn in (distances.log_euclidean, distances.log_euclidean_sq):
        assert SM(n_dim=6, n_filters=2, distance_fun=fn)._has_fused_closure()
        assert SM(n_dim=6, n_filters=2, distance_fun=fn).double()._has_fused_closure()
        assert SM(n_dim=6, n_filters=2, distance_fun=fn, constraint="orthogonal")._has_fused_closure()
        assert SM(n_dim=80, n_filters=64, distance_fun=fn)._has_fused_closure()
        # these operators take matrices, not statistics dictionaries: not a distance_fun of SQFA's closure
        assert not SQ(n_dim=6, n_filters=2, distance_fun=fn)._has_fused_closure()
        # beyond the per-class SPD functions' limits the generic closure is used (and never captured in a graph)
        assert not SM(n_dim=80, n_filters=65, distance_fun=fn)._has_fused_closure()
        assert not SM(n_dim=6, n_filters=2, distance_fun=fn).half()._has_fused_closure()
    # the other operators answer as before
    assert SM(n_dim=6, n_filters=2)._has_fused_closure()
    assert not SM(n_dim=6, n_filters=2, distance_fun=distances.hellinger)._has_fused_closure()
    assert SQ(n_dim=6, n_filters=2, distance_fun=distances.hellinger)._has_fused_closure()
    monkeypatch.setattr(distances, "LOG_EUCLIDEAN_FUSED_CLOSURE", False)
    for fn in (distances.log_euclidean, distances.log_euclidean_sq):
        assert not SM(n_dim=6, n_filters=2, distance_fun=fn)._has_fused_closure()
    assert SM(n_dim=6, n_filters=2)._has_fused_closure()


def test_sharded_models_keep_the_generic_closure():
    class FakeShard:
        shard, world_size = (0, 2), 2

    model = sqfa_amd.model.SecondMomentsSQFA(n_dim=6, n_filters=2, distance_fun=distances.log_euclidean)
    model.pair_shard = FakeShard()
    assert not model._has_fused_closure()
    assert model._fused_closure_loss(torch.eye(6).repeat(3, 1, 1)) is None


def test_cpu_statistics_keep_the_generic_closure():
    """CPU tensors: _fused_closure_loss declines (None) and the fit runs the torch expressions as before; the native call
    itself refuses CPU tensors instead of computing something else."""
    g = torch.Generator().manual_seed(0)
    X = torch.randn(5, 6, 24, generator=g, dtype=torch.float64)
    scatters = X @ X.transpose(1, 2) / 24
    for fn in (distances.log_euclidean, distances.log_euclidean_sq):
        model = sqfa_amd.model.SecondMomentsSQFA(n_dim=6, n_filters=2, feature_noise=1e-2, distance_fun=fn).double()
        assert model._has_fused_closure()
        assert model._fused_closure_loss(scatters) is None
        assert model._fused_closure_loss({"means": torch.zeros(5, 6, dtype=torch.float64), "covariances": scatters}) is None
        loss, _ = model.fit(data_statistics=scatters, max_epochs=3, show_progress=False, return_loss=True)
        assert torch.isfinite(loss).all() and loss[-1] < loss[0]
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.ClassPairLoss.apply(None, scatters[:, :2, :2], "log_euclidean", True, 1e-6, -0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.hip_log_euclidean_pairwise_loss(scatters[:, :2, :2], False, 1e-6, -0.1)
