"""CPU tests of the C ABI of the top-k and label-rank entries (sqfa_gauss_scores_topk, sqfa_gauss_label_rank and their
workspace queries): exported symbols and bindings, the header, the workspace queries, and host-side argument validation with
fake pointers (every code is returned before the first HIP call, so no GPU is needed and nothing is launched)."""
import ctypes
import os
import re

import pytest

import sqfa_amd
from sqfa_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
NAMES = ("sqfa_gauss_scores_topk_workspace_bytes", "sqfa_gauss_scores_topk", "sqfa_gauss_label_rank_workspace_bytes",
         "sqfa_gauss_label_rank")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES[NAMES[0]] == (ctypes.c_size_t, [ctypes.c_longlong] + [ctypes.c_int] * 4)
    assert _lib.PROTOTYPES[NAMES[2]] == (ctypes.c_size_t, [ctypes.c_longlong] + [ctypes.c_int] * 3)
    assert len(_lib.PROTOTYPES[NAMES[1]][1]) == 15 and len(_lib.PROTOTYPES[NAMES[3]][1]) == 15
    assert _lib.PROTOTYPES[NAMES[1]][1][1] is ctypes.c_longlong       # N
    assert _lib.PROTOTYPES[NAMES[3]][1][2] is ctypes.c_longlong
    assert _lib.PROTOTYPES[NAMES[1]][1][13] is ctypes.c_size_t and _lib.PROTOTYPES[NAMES[3]][1][13] is ctypes.c_size_t
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "size_t sqfa_gauss_scores_topk_workspace_bytes(long long N, int C, int K, int dtype, int k);" in header
    assert "size_t sqfa_gauss_label_rank_workspace_bytes(long long N, int C, int K, int dtype);" in header
    decl = re.search(r"int sqfa_gauss_scores_topk\(([^;]*)\);", header)
    assert decl is not None and decl.group(1).count(",") == 14 and "long long N" in decl.group(1) and "int k" in decl.group(1)
    decl = re.search(r"int sqfa_gauss_label_rank\(([^;]*)\);", header)
    assert decl is not None and decl.group(1).count(",") == 14 and "const long long *labels" in decl.group(1)


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_queries(lib, dtype):
    topk, rank = lib.sqfa_gauss_scores_topk_workspace_bytes, lib.sqfa_gauss_label_rank_workspace_bytes
    assert topk(1, 1, 1, dtype, 1) > 0 and rank(1, 1, 1, dtype) > 0
    assert topk(1000, 10, 64, dtype, 8) > 0 and rank(1000, 10, 64, dtype) > 0
    for k in (1, 2, 3, 4, 5, 7, 8):
        assert topk(1000, 10, 16, dtype, k) > 0
    for k in (0, -1, 9, 11, 1000):
        assert topk(1000, 10, 16, dtype, k) == 0
    assert topk(1000, 3, 16, dtype, 3) > 0 and topk(1000, 3, 16, dtype, 4) == 0     # k <= C
    for bad in ((1000, 10, 65), (1000, 10, 128), (1000, 10, 0), (0, 10, 4), (-5, 10, 4), (1000, 0, 4),
                (2 ** 31 * 64 + 1, 10, 4)):
        assert topk(*bad, dtype, 1) == 0 and rank(*bad, dtype) == 0
    for code in (5, -1):
        assert topk(1000, 10, 4, code, 1) == 0 and rank(1000, 10, 4, code) == 0
    # no N C term: the class count enters only through the number of splits, which is at most 16; the partial lists are
    # 16 splits x 8 entries x (a value and an index) per sample at most, the rank's 8 bytes and 16 int32 counts per sample
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for N in (1, 63, 64, 65, 1000, 10 ** 5, 10 ** 6, 3 * 10 ** 9):
        for K in (1, 16, 64):
            for k in (1, 2, 5, 8):
                sizes = [topk(N, C, K, dtype, k) for C in (8, 9, 100, 1000, 10 ** 5)]
                assert all(16 <= b <= 16 * N * 8 * (esz + 4) + 16 for b in sizes), (N, K, k, sizes)
                assert sizes[-1] == sizes[-2]
            sizes = [rank(N, C, K, dtype) for C in (1, 4, 5, 100, 1000, 10 ** 5)]
            assert all(16 <= b <= N * (8 + 16 * 4) + 16 for b in sizes), (N, K, sizes)
            assert sizes[-1] == sizes[-2]
    assert topk(10 ** 6, 1000, 16, dtype, 5) == 16          # 15625 sample tiles: the classes are not split
    assert rank(10 ** 6, 1000, 16, dtype) == 8 * 10 ** 6


def _topk(lib, Z=1, N=100, W=1, off=1, C=40, K=8, dtype=_lib.SQFA_F32, k=5, index=1, score=0, bad=1, ws=1, ws_bytes=1 << 26):
    return lib.sqfa_gauss_scores_topk(FAKE if Z else NULL, N, NULL, FAKE if W else NULL, FAKE if off else NULL, C, K, dtype, k,
                                      FAKE if index else NULL, FAKE if score else NULL, FAKE if bad else NULL,
                                      FAKE if ws else NULL, ws_bytes, NULL)


def _rank(lib, Z=1, labels=1, N=100, W=1, off=1, C=40, K=8, dtype=_lib.SQFA_F32, rank=1, score=0, flags=1, ws=1,
          ws_bytes=1 << 26):
    return lib.sqfa_gauss_label_rank(FAKE if Z else NULL, FAKE if labels else NULL, N, NULL, FAKE if W else NULL,
                                     FAKE if off else NULL, C, K, dtype, FAKE if rank else NULL, FAKE if score else NULL,
                                     FAKE if flags else NULL, FAKE if ws else NULL, ws_bytes, NULL)


def test_topk_argument_validation(lib):
    for null in ("Z", "W", "off", "index", "bad"):
        assert _topk(lib, **{null: 0}) == -1
    for size in (dict(N=0), dict(N=-1), dict(C=0), dict(K=0)):
        assert _topk(lib, **size) == -1
    assert _topk(lib, dtype=7) == -1
    assert b"dtype" in lib.sqfa_hip_last_error()
    for k, C in ((0, 40), (9, 40), (-1, 40), (41, 40), (5, 4), (2, 1)):   # k = 0, 9 and C + 1
        assert _topk(lib, k=k, C=C) == -1
        assert b"k outside" in lib.sqfa_hip_last_error()
    assert _topk(lib, k=9, dtype=7) == -1
    assert b"dtype" in lib.sqfa_hip_last_error()                 # dtype before k
    assert _topk(lib, K=65) == -2                                # SQFA_ERR_UNSUPPORTED_M
    assert b"K > 64" in lib.sqfa_hip_last_error()
    assert _topk(lib, K=65, Z=0) == -1                           # the argument checks come before the size check ...
    assert _topk(lib, K=65, k=0) == -1
    assert _topk(lib, K=65, k=9) == -1
    assert _topk(lib, K=65, ws_bytes=0) == -2                    # ... and the size check before the workspace check
    assert _topk(lib, K=65, ws=0) == -2
    assert _topk(lib, N=2 ** 31 * 64 + 1) == -2                  # more sample tiles than a grid holds
    assert _topk(lib, ws=0) == -3                                # SQFA_ERR_WORKSPACE
    assert _topk(lib, ws_bytes=8) == -3
    assert b"workspace" in lib.sqfa_hip_last_error()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):                 # one byte short of the query, with and without class splits
        for N, C, K, k in ((100, 40, 8, 5), (100, 40, 8, 1), (100, 1, 64, 1), (10 ** 6, 1000, 16, 8)):
            need = lib.sqfa_gauss_scores_topk_workspace_bytes(N, C, K, dtype, k)
            assert _topk(lib, N=N, C=C, K=K, dtype=dtype, k=k, ws_bytes=need - 1) == -3
            assert _topk(lib, N=N, C=C, K=K, dtype=dtype, k=k, ws_bytes=need - 1, score=1) == -3


def test_label_rank_argument_validation(lib):
    for null in ("Z", "labels", "W", "off", "rank", "flags"):
        assert _rank(lib, **{null: 0}) == -1
    for size in (dict(N=0), dict(N=-1), dict(C=0), dict(K=0)):
        assert _rank(lib, **size) == -1
    assert _rank(lib, dtype=7) == -1
    assert b"dtype" in lib.sqfa_hip_last_error()
    assert _rank(lib, K=65) == -2
    assert b"K > 64" in lib.sqfa_hip_last_error()
    assert _rank(lib, K=65, labels=0) == -1
    assert _rank(lib, K=65, dtype=7) == -1
    assert _rank(lib, K=65, ws_bytes=0) == -2
    assert _rank(lib, K=65, ws=0) == -2
    assert _rank(lib, N=2 ** 31 * 64 + 1) == -2
    assert _rank(lib, N=2 ** 31 * 16 + 1) == -2                  # the label pass takes 16 samples per workgroup
    assert _rank(lib, ws=0) == -3
    assert _rank(lib, ws_bytes=8) == -3
    assert b"workspace" in lib.sqfa_hip_last_error()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):
        for N, C, K in ((100, 40, 8), (100, 1, 64), (10 ** 6, 1000, 16)):
            need = lib.sqfa_gauss_label_rank_workspace_bytes(N, C, K, dtype)
            assert _rank(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1) == -3
            assert _rank(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1, score=1) == -3
