"""CPU tests of the C ABI of the fused Jeffreys closure (sqfa_jeffreys_pairwise_loss, sqfa_jeffreys_workspace_bytes):
exported symbols and bindings, the workspace query, and host-side argument validation with fake pointers (every code is
returned before the first HIP call, so no GPU is needed and nothing is launched)."""
import ctypes
import os

import pytest

import sqfa_amd
from sqfa_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in ("sqfa_jeffreys_pairwise_loss", "sqfa_jeffreys_workspace_bytes"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    # mu, cov, n, m, dtype, sqrt_mode, eps, pair_weights, uniform_weight, loss_out, gmu_out, gcov_out, dist_out,
    # nonfinite_out, workspace, workspace_bytes, stream
    assert len(_lib.PROTOTYPES["sqfa_jeffreys_pairwise_loss"][1]) == 17
    assert _lib.PROTOTYPES["sqfa_jeffreys_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "sqfa_jeffreys_pairwise_loss(" in header and "sqfa_jeffreys_workspace_bytes(" in header


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(lib, dtype):
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    assert lib.sqfa_jeffreys_workspace_bytes(10, 64, dtype) > 0
    assert lib.sqfa_jeffreys_workspace_bytes(10, 65, dtype) == 0
    assert lib.sqfa_jeffreys_workspace_bytes(1, 4, dtype) == 0
    assert lib.sqfa_jeffreys_workspace_bytes(10, 0, dtype) == 0
    assert lib.sqfa_jeffreys_workspace_bytes(10, 4, 5) == 0
    for m in (1, 3, 16, 17, 33, 64):
        prev = 0
        for n in (2, 3, 10, 1000, 1001):
            b = lib.sqfa_jeffreys_workspace_bytes(n, m, dtype)
            # the precisions, the two accumulated gradients, one double matrix per class: no (n,n) term
            assert b >= prev and b >= n * m * m * (3 * esz + 8), (n, m)
            assert b < n * m * m * (3 * esz + 8) + 16 * n + 8192, (n, m)
            prev = b


def _call(lib, mu=1, cov=1, n=4, m=8, dtype=_lib.SQFA_F32, sqrt_mode=1, gmu=1, gcov=1, ws=1, ws_bytes=1 << 26):
    return lib.sqfa_jeffreys_pairwise_loss(FAKE if mu else NULL, FAKE if cov else NULL, n, m, dtype, sqrt_mode, 1e-6, NULL, -1.0,
                                           FAKE, FAKE if gmu else NULL, FAKE if gcov else NULL, NULL, NULL,
                                           FAKE if ws else NULL, ws_bytes, NULL)


def test_argument_validation(lib):
    assert _call(lib, cov=0) == -1
    assert _call(lib, n=1) == -1                       # at least one pair
    assert _call(lib, n=0) == -1
    assert _call(lib, m=0) == -1
    assert _call(lib, dtype=7) == -1
    assert _call(lib, sqrt_mode=2) == -1
    assert _call(lib, sqrt_mode=-1) == -1
    assert _call(lib, gmu=1, gcov=0) == -1             # exactly one of the two gradients
    assert _call(lib, gmu=0, gcov=1) == -1
    assert _call(lib, mu=0, gmu=1, gcov=1) == -1       # no means, no gradient of the means
    assert _call(lib, mu=0, gmu=1, gcov=0) == -1
    assert _call(lib, m=65) == -2                      # SQFA_ERR_UNSUPPORTED_M
    assert _call(lib, m=128) == -2
    assert _call(lib, m=65, sqrt_mode=2) == -1         # the argument checks come before the size check ...
    assert _call(lib, m=65, ws_bytes=16) == -2         # ... and the size check before the workspace check
    assert _call(lib, ws_bytes=16) == -3               # SQFA_ERR_WORKSPACE
    assert b"workspace" in lib.sqfa_hip_last_error()
    assert _call(lib, ws=0) == -3
    assert _call(lib, m=64, ws_bytes=16) == -3         # 64 is supported: only the workspace is wrong
    assert _call(lib, gmu=0, gcov=0, ws_bytes=16) == -3            # forward only passes the argument checks
    assert _call(lib, mu=0, gmu=0, gcov=1, ws_bytes=16) == -3      # and so do the means-free calls, with
    assert _call(lib, mu=0, gmu=0, gcov=0, ws_bytes=16) == -3      # and without the gradient
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):       # one byte short of the query
        need = lib.sqfa_jeffreys_workspace_bytes(4, 8, dtype)
        assert _call(lib, dtype=dtype, ws_bytes=need - 1) == -3
        assert b"workspace" in lib.sqfa_hip_last_error()
