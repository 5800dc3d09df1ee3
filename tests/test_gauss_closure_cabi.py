"""CPU tests of the fused Gaussian pair closure (sqfa_gauss_pairwise_loss, _native.ClassPairLoss): exported symbols and
bindings, host-side argument validation (every code is returned before any launch, so no GPU is needed), workspace
query, the fused specs of the four operators and the models' _has_fused_closure()."""
import ctypes
import os

import pytest
import torch

import sqfa_amd
from sqfa_amd import _lib, _native, distances

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
OPS = {"bhattacharyya": 0, "hellinger": 1, "mahalanobis_sq": 2, "mahalanobis": 3}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in ("sqfa_gauss_pairwise_loss", "sqfa_gauss_pairwise_workspace_bytes"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    assert len(_lib.PROTOTYPES["sqfa_gauss_pairwise_loss"][1]) == 16
    assert _lib.PROTOTYPES["sqfa_gauss_pairwise_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert (_lib.SQFA_GAUSS_BHATTACHARYYA, _lib.SQFA_GAUSS_HELLINGER, _lib.SQFA_GAUSS_MAHALANOBIS_SQ,
            _lib.SQFA_GAUSS_MAHALANOBIS) == (0, 1, 2, 3)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    for name, code in (("BHATTACHARYYA", 0), ("HELLINGER", 1), ("MAHALANOBIS_SQ", 2), ("MAHALANOBIS", 3)):
        assert any(line.split() == ["#define", f"SQFA_GAUSS_{name}", str(code)] for line in header.splitlines())
    assert "sqfa_gauss_pairwise_loss(" in header and "sqfa_gauss_pairwise_workspace_bytes(" in header


def _call(lib, mu=1, cov=1, n=4, m=8, dtype=_lib.SQFA_F32, kind=0, gmu=1, gcov=1, ws=1, ws_bytes=1 << 24):
    return lib.sqfa_gauss_pairwise_loss(FAKE if mu else NULL, FAKE if cov else NULL, n, m, dtype, kind, 1e-6, -1.0,
                                        FAKE, FAKE if gmu else NULL, FAKE if gcov else NULL, NULL, NULL,
                                        FAKE if ws else NULL, ws_bytes, NULL)


def test_argument_validation(lib):
    assert _call(lib, mu=0) == -1
    assert _call(lib, cov=0) == -1
    assert _call(lib, n=1) == -1                       # at least one pair
    assert _call(lib, n=0) == -1
    assert _call(lib, m=0) == -1
    assert _call(lib, dtype=7) == -1
    assert _call(lib, kind=4) == -1
    assert _call(lib, kind=-1) == -1
    assert _call(lib, gmu=0, gcov=1) == -1             # both gradients or neither
    assert _call(lib, gmu=1, gcov=0) == -1
    assert _call(lib, m=65) == -2                      # SQFA_ERR_UNSUPPORTED_M
    assert _call(lib, ws_bytes=16) == -3               # SQFA_ERR_WORKSPACE
    assert _call(lib, ws=0) == -3
    assert _call(lib, m=64, ws_bytes=16) == -3         # 64 is supported: only the workspace is wrong
    assert _call(lib, gmu=0, gcov=0, ws_bytes=16) == -3   # forward only passes the argument checks too


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(lib, dtype):
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for m in (1, 3, 4, 16, 17, 33, 64):
        prev = 0
        for n in (2, 3, 10, 100, 1000, 1001):
            b = lib.sqfa_gauss_pairwise_workspace_bytes(n, m, dtype)
            assert b >= prev and b >= n * m * m * esz + n * 8, (n, m)   # one inverse and one log-determinant per class
            assert b < 2 * n * (m + 3) * (m + 3) * 8 + 64 * n + 4096
            prev = b
    assert lib.sqfa_gauss_pairwise_workspace_bytes(10, 64, dtype) > 0
    assert lib.sqfa_gauss_pairwise_workspace_bytes(10, 65, dtype) == 0
    assert lib.sqfa_gauss_pairwise_workspace_bytes(10, 0, dtype) == 0
    assert lib.sqfa_gauss_pairwise_workspace_bytes(1, 4, dtype) == 0
    assert lib.sqfa_gauss_pairwise_workspace_bytes(10, 4, 5) == 0


def test_plain_pair_terms_limits_unchanged(lib):
    assert lib.sqfa_gauss_pair_terms(FAKE, FAKE, 3, FAKE, FAKE, 3, 65, 0, NULL, NULL, FAKE, FAKE, NULL, NULL, NULL) == -2


def test_fused_specs_and_switch(monkeypatch):
    for name, code in OPS.items():
        spec = distances.fused_spec(getattr(distances, name))
        assert spec is not None and spec[0] == "gaussian" and spec[1] == code and spec[3] == "gauss", name
    assert distances.fused_spec(distances.fisher_rao_same_cov) is None     # NaN closure gradient in the reference: not fused
    assert distances.fused_spec(distances.log_euclidean) is None
    assert distances.fused_spec(distances.fisher_rao_lower_bound) == ("gaussian", 0.5, True, "airm")
    assert distances.GAUSS_FUSED_CLOSURE is True
    monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", False)
    for name in OPS:
        assert distances.fused_spec(getattr(distances, name)) is None
    assert distances.fused_spec(distances.fisher_rao_lower_bound) == ("gaussian", 0.5, True, "airm")


def test_models_follow_the_spec(monkeypatch):
    for name in OPS:
        fn = getattr(distances, name)
        assert sqfa_amd.model.SQFA(n_dim=6, n_filters=2, distance_fun=fn)._has_fused_closure()
        # these operators take statistics dictionaries: not a distance_fun of the second-moment model
        assert not sqfa_amd.model.SecondMomentsSQFA(n_dim=6, n_filters=2, distance_fun=fn)._has_fused_closure()
    assert not sqfa_amd.model.SQFA(n_dim=6, n_filters=2, distance_fun=distances.fisher_rao_same_cov)._has_fused_closure()
    # beyond the kernels' limits the generic closure is used (and never captured in a graph)
    assert not sqfa_amd.model.SQFA(n_dim=80, n_filters=65, distance_fun=distances.hellinger)._has_fused_closure()
    assert not sqfa_amd.model.SQFA(n_dim=6, n_filters=2, distance_fun=distances.hellinger).half()._has_fused_closure()
    monkeypatch.setattr(distances, "GAUSS_FUSED_CLOSURE", False)
    assert not sqfa_amd.model.SQFA(n_dim=6, n_filters=2, distance_fun=distances.hellinger)._has_fused_closure()


def test_cpu_statistics_keep_the_generic_closure():
    """CPU tensors: _fused_closure_loss declines (None) and the fit runs the torch expressions as before; the native call
    itself refuses CPU tensors instead of computing something else."""
    g = torch.Generator().manual_seed(0)
    X = torch.randn(5, 6, 24, generator=g, dtype=torch.float64)
    stats = {"means": 0.3 * torch.randn(5, 6, generator=g, dtype=torch.float64),
             "covariances": X @ X.transpose(1, 2) / 24}
    model = sqfa_amd.model.SQFA(n_dim=6, n_filters=2, feature_noise=1e-2, distance_fun=distances.bhattacharyya).double()
    assert model._fused_closure_loss(stats) is None
    loss, _ = model.fit(data_statistics=stats, max_epochs=3, show_progress=False, return_loss=True)
    assert torch.isfinite(loss).all() and loss[-1] < loss[0]
    with pytest.raises(RuntimeError, match="GPU only"):
        _native.ClassPairLoss.apply(stats["means"][:, :2], stats["covariances"][:, :2, :2], "gauss", 0, 1e-6, -0.1)
