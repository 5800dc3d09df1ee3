"""CPU tests of the C ABI of the nested Gaussian class scores (sqfa_gauss_class_factors_nested, sqfa_gauss_scores_nested,
sqfa_gauss_scores_nested_workspace_bytes, sqfa_gauss_label_scores_nested): exported symbols and bindings, the header, the
workspace query, and host-side argument validation with fake pointers (every code is returned before the first HIP call, so
no GPU is needed and nothing is launched)."""
import ctypes
import os
import re

import pytest

import sqfa_amd
from sqfa_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
NAMES = ("sqfa_gauss_class_factors_nested", "sqfa_gauss_scores_nested", "sqfa_gauss_scores_nested_workspace_bytes",
         "sqfa_gauss_label_scores_nested")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    assert _lib.PROTOTYPES["sqfa_gauss_scores_nested_workspace_bytes"] == _lib.PROTOTYPES["sqfa_gauss_scores_workspace_bytes"]
    assert _lib.PROTOTYPES["sqfa_gauss_class_factors_nested"] == _lib.PROTOTYPES["sqfa_gauss_class_factors"]
    assert len(_lib.PROTOTYPES["sqfa_gauss_scores_nested"][1]) == 14
    assert len(_lib.PROTOTYPES["sqfa_gauss_label_scores_nested"][1]) == 13
    assert _lib.PROTOTYPES["sqfa_gauss_scores_nested"][1][1] is ctypes.c_longlong          # N
    assert _lib.PROTOTYPES["sqfa_gauss_label_scores_nested"][1][2] is ctypes.c_longlong    # N
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "size_t sqfa_gauss_scores_nested_workspace_bytes(long long N, int C, int K, int dtype);" in header
    for name, commas in (("sqfa_gauss_class_factors_nested", 9), ("sqfa_gauss_scores_nested", 13),
                         ("sqfa_gauss_label_scores_nested", 12)):
        decl = re.search(rf"int {name}\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") == commas, name


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(lib, dtype):
    q = lib.sqfa_gauss_scores_nested_workspace_bytes
    assert q(1, 1, 1, dtype) > 0
    assert q(1000, 10, 64, dtype) > 0
    assert q(1000, 10, 65, dtype) == 0
    assert q(1000, 10, 128, dtype) == 0
    assert q(1000, 10, 0, dtype) == 0
    assert q(0, 10, 4, dtype) == 0
    assert q(-5, 10, 4, dtype) == 0
    assert q(1000, 0, 4, dtype) == 0
    assert q(1000, 10, 4, 5) == 0
    assert q(1000, 10, 4, -1) == 0
    # (splits, N, K) partials of three values and an index, at most 16 splits, each array rounded up to 256 bytes; nothing
    # where the samples alone fill the GPU; no N C term
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for N in (1, 63, 64, 65, 1000, 10 ** 5, 10 ** 6):
        for K in (1, 16, 64):
            sizes = [q(N, C, K, dtype) for C in (1, 4, 5, 100, 1000, 10 ** 5)]
            assert all(16 <= b <= 16 * N * K * (3 * esz + 4) + 4 * 256 for b in sizes), (N, K, sizes)
            assert sizes[0] == 16 and sizes[-1] == sizes[-2]
    assert q(10 ** 6, 1000, 16, dtype) == 16


def _factors(lib, cov=1, W=1, off=1, bad=1, C=4, K=8, dtype=_lib.SQFA_F32, means=1, priors=0):
    return lib.sqfa_gauss_class_factors_nested(FAKE if means else NULL, FAKE if cov else NULL, FAKE if priors else NULL, C, K,
                                               dtype, FAKE if W else NULL, FAKE if off else NULL, FAKE if bad else NULL, NULL)


def _scores(lib, Z=1, N=100, W=1, off=1, C=4, K=8, dtype=_lib.SQFA_F32, argmax=1, lse=0, bad=1, ws=1, ws_bytes=1 << 28):
    return lib.sqfa_gauss_scores_nested(FAKE if Z else NULL, N, NULL, FAKE if W else NULL, FAKE if off else NULL, C, K, dtype,
                                        FAKE if argmax else NULL, FAKE if lse else NULL, FAKE if bad else NULL,
                                        FAKE if ws else NULL, ws_bytes, NULL)


def _labels(lib, Z=1, labels=1, N=100, W=1, off=1, C=4, K=8, dtype=_lib.SQFA_F32, lse=1, ll=1, flags=1):
    return lib.sqfa_gauss_label_scores_nested(FAKE if Z else NULL, FAKE if labels else NULL, N, NULL, FAKE if W else NULL,
                                              FAKE if off else NULL, C, K, dtype, FAKE if lse else NULL, FAKE if ll else NULL,
                                              FAKE if flags else NULL, NULL)


def test_class_factors_argument_validation(lib):
    assert _factors(lib, cov=0) == -1
    assert _factors(lib, W=0) == -1
    assert _factors(lib, off=0) == -1
    assert _factors(lib, bad=0) == -1
    assert _factors(lib, C=0) == -1
    assert _factors(lib, K=0) == -1
    assert _factors(lib, dtype=7) == -1
    assert b"dtype" in lib.sqfa_hip_last_error()
    assert _factors(lib, K=65) == -2                   # SQFA_ERR_UNSUPPORTED_M
    assert _factors(lib, K=65, means=0) == -2
    assert b"sqfa_gauss_class_factors_nested: K > 64" in lib.sqfa_hip_last_error()
    assert _factors(lib, K=65, cov=0) == -1            # the argument checks come before the size check
    assert _factors(lib, K=65, dtype=7) == -1


def test_scores_argument_validation(lib):
    assert _scores(lib, Z=0) == -1
    assert _scores(lib, W=0) == -1
    assert _scores(lib, off=0) == -1
    assert _scores(lib, bad=0) == -1                   # the counter is not optional
    assert _scores(lib, N=0) == -1
    assert _scores(lib, N=-1) == -1
    assert _scores(lib, C=0) == -1
    assert _scores(lib, K=0) == -1
    assert _scores(lib, dtype=7) == -1
    assert _scores(lib, argmax=0, lse=0) == -1         # one of the two outputs at least
    assert b"no output" in lib.sqfa_hip_last_error()
    assert _scores(lib, K=65) == -2                    # SQFA_ERR_UNSUPPORTED_M
    assert _scores(lib, K=128) == -2
    assert b"K > 64" in lib.sqfa_hip_last_error()
    assert lib.sqfa_gauss_scores_nested_workspace_bytes(100, 4, 65, _lib.SQFA_F32) == 0
    assert _scores(lib, K=65, Z=0) == -1               # the argument checks come before the size check ...
    assert _scores(lib, K=65, dtype=7) == -1
    assert _scores(lib, K=65, ws_bytes=0) == -2        # ... and the size check before the workspace check
    assert _scores(lib, K=65, ws=0) == -2
    assert _scores(lib, N=2 ** 31 * 64 + 1) == -2      # more sample tiles than a grid holds
    assert _scores(lib, ws=0) == -3                    # SQFA_ERR_WORKSPACE
    assert _scores(lib, ws_bytes=8) == -3
    assert b"workspace" in lib.sqfa_hip_last_error()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):       # one byte short of the query, with and without class splits
        for N, C, K in ((100, 40, 8), (100, 1, 64), (10 ** 6, 1000, 16)):
            need = lib.sqfa_gauss_scores_nested_workspace_bytes(N, C, K, dtype)
            assert _scores(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1) == -3
            assert _scores(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1, argmax=0, lse=1) == -3


def test_label_scores_argument_validation(lib):
    for missing in ("Z", "labels", "W", "off", "lse", "ll", "flags"):
        assert _labels(lib, **{missing: 0}) == -1, missing
    assert _labels(lib, N=0) == -1
    assert _labels(lib, C=0) == -1
    assert _labels(lib, K=0) == -1
    assert _labels(lib, dtype=7) == -1
    assert _labels(lib, K=65) == -2                    # SQFA_ERR_UNSUPPORTED_M
    assert b"sqfa_gauss_label_scores_nested: K > 64" in lib.sqfa_hip_last_error()
    assert _labels(lib, K=65, labels=0) == -1          # the argument checks come before the size check
    assert _labels(lib, N=2 ** 31 * 64 + 1) == -2      # more sample tiles than a grid holds
