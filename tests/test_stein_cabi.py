"""CPU tests of the C ABI of the fused Stein closure (sqfa_stein_pairwise_loss, sqfa_stein_workspace_bytes): exported
symbols and bindings, the workspace query, and host-side argument validation with fake pointers (every code is returned
before the first HIP call, so no GPU is needed and nothing is launched)."""
import ctypes
import os
import re

import pytest

import sqfa_amd
from sqfa_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in ("sqfa_stein_pairwise_loss", "sqfa_stein_workspace_bytes"):
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    # S, n, m, dtype, sqrt_mode, eps, pair_weights, uniform_weight, loss_out, gradS_out, dist_out, nonfinite_out,
    # workspace, workspace_bytes, stream: sqfa_jeffreys_pairwise_loss without mu and gmu_out
    assert len(_lib.PROTOTYPES["sqfa_stein_pairwise_loss"][1]) == 15
    jeff = list(_lib.PROTOTYPES["sqfa_jeffreys_pairwise_loss"][1])
    del jeff[10], jeff[0]
    assert _lib.PROTOTYPES["sqfa_stein_pairwise_loss"] == (ctypes.c_int, jeff)
    assert _lib.PROTOTYPES["sqfa_stein_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "size_t sqfa_stein_workspace_bytes(int n, int m, int dtype);" in header
    decl = re.search(r"int sqfa_stein_pairwise_loss\(([^;]*)\);", header)
    assert decl is not None and decl.group(1).count(",") == 14


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(lib, dtype):
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    assert lib.sqfa_stein_workspace_bytes(10, 64, dtype) > 0
    assert lib.sqfa_stein_workspace_bytes(10, 65, dtype) == 0
    assert lib.sqfa_stein_workspace_bytes(10, 128, dtype) == 0
    assert lib.sqfa_stein_workspace_bytes(0, 4, dtype) == 0
    assert lib.sqfa_stein_workspace_bytes(-3, 4, dtype) == 0
    assert lib.sqfa_stein_workspace_bytes(1, 4, dtype) == 0            # no pair
    assert lib.sqfa_stein_workspace_bytes(10, 0, dtype) == 0
    assert lib.sqfa_stein_workspace_bytes(10, 4, 5) == 0
    assert lib.sqfa_stein_workspace_bytes(10, 4, -1) == 0
    # the inverses and the partial sums of the gradient (one slice up to m = 16, one per lane group of the pass above:
    # 8 up to 32, 4 up to 64): no (n,n) term
    for m, slices in ((1, 1), (3, 1), (16, 1), (17, 8), (32, 8), (33, 4), (64, 4)):
        prev = 0
        for n in (2, 3, 10, 1000, 1001):
            b = lib.sqfa_stein_workspace_bytes(n, m, dtype)
            assert b >= prev and b >= n * m * m * (1 + slices) * esz, (n, m)
            assert b < n * m * m * (1 + slices) * esz + 40 * n + 8192, (n, m)
            prev = b


def _call(lib, S=1, n=4, m=8, dtype=_lib.SQFA_F32, sqrt_mode=1, grad=1, ws=1, ws_bytes=1 << 26):
    return lib.sqfa_stein_pairwise_loss(FAKE if S else NULL, n, m, dtype, sqrt_mode, 1e-6, NULL, -1.0, FAKE,
                                        FAKE if grad else NULL, NULL, NULL, FAKE if ws else NULL, ws_bytes, NULL)


def test_argument_validation(lib):
    assert _call(lib, S=0) == -1
    assert _call(lib, n=1) == -1                       # at least one pair
    assert _call(lib, n=0) == -1
    assert _call(lib, m=0) == -1
    assert _call(lib, dtype=7) == -1
    assert _call(lib, sqrt_mode=2) == -1
    assert _call(lib, sqrt_mode=-1) == -1
    assert b"sqrt_mode" in lib.sqfa_hip_last_error()
    assert _call(lib, m=65) == -2                      # SQFA_ERR_UNSUPPORTED_M
    assert _call(lib, m=128) == -2
    assert b"m > 64" in lib.sqfa_hip_last_error()
    assert _call(lib, m=65, sqrt_mode=2) == -1         # the argument checks come before the size check ...
    assert _call(lib, m=65, S=0) == -1
    assert _call(lib, m=65, ws_bytes=16) == -2         # ... and the size check before the workspace check
    assert _call(lib, m=65, ws=0) == -2
    assert _call(lib, ws_bytes=16) == -3               # SQFA_ERR_WORKSPACE
    assert b"workspace" in lib.sqfa_hip_last_error()
    assert _call(lib, ws=0) == -3
    assert _call(lib, m=64, ws_bytes=16) == -3         # 64 is supported: only the workspace is wrong
    assert _call(lib, grad=0, ws_bytes=16) == -3       # forward only passes the argument checks
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):       # one byte short of the query
        for m in (8, 24, 64):
            need = lib.sqfa_stein_workspace_bytes(4, m, dtype)
            assert _call(lib, m=m, dtype=dtype, ws_bytes=need - 1) == -3
            assert b"workspace" in lib.sqfa_hip_last_error()
