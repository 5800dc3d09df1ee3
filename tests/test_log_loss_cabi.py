"""CPU tests of the C ABI of the Gaussian log-loss (sqfa_gauss_log_loss, sqfa_gauss_log_loss_backward, their workspace
queries and sqfa_gauss_log_loss_layout): exported symbols and bindings, the header, the queries, and host-side argument
validation with fake pointers (every code is returned before the first HIP call, so no GPU is needed and nothing is
launched)."""
import ctypes
import os
import re

import pytest

import sqfa_amd
from sqfa_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)
NAMES = ("sqfa_gauss_log_loss", "sqfa_gauss_log_loss_backward", "sqfa_gauss_log_loss_workspace_bytes",
         "sqfa_gauss_log_loss_backward_workspace_bytes", "sqfa_gauss_log_loss_layout")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    for name in NAMES:
        assert name in _lib.PROTOTYPES
        assert getattr(lib, name).restype is _lib.PROTOTYPES[name][0]
    query = (ctypes.c_size_t, [ctypes.c_longlong] + [ctypes.c_int] * 3)
    assert _lib.PROTOTYPES["sqfa_gauss_log_loss_workspace_bytes"] == query
    assert _lib.PROTOTYPES["sqfa_gauss_log_loss_backward_workspace_bytes"] == query
    assert len(_lib.PROTOTYPES["sqfa_gauss_log_loss"][1]) == 16
    assert len(_lib.PROTOTYPES["sqfa_gauss_log_loss_backward"][1]) == 17
    assert _lib.PROTOTYPES["sqfa_gauss_log_loss"][1][2] is ctypes.c_longlong            # N
    assert _lib.PROTOTYPES["sqfa_gauss_log_loss_backward"][1][2] is ctypes.c_longlong
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(sqfa_amd.__file__))), "include", "sqfa_hip.h")) as fh:
        header = fh.read()
    assert "size_t sqfa_gauss_log_loss_workspace_bytes(long long N, int C, int K, int dtype);" in header
    assert "size_t sqfa_gauss_log_loss_backward_workspace_bytes(long long N, int C, int K, int dtype);" in header
    for name, commas in (("sqfa_gauss_log_loss", 15), ("sqfa_gauss_log_loss_backward", 16), ("sqfa_gauss_log_loss_layout", 7)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None and decl.group(1).count(",") == commas and "long long N" in decl.group(1)


def _layout(lib, N, C, K, dtype):
    cs, gps, ss = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tps = ctypes.c_longlong()
    status = lib.sqfa_gauss_log_loss_layout(N, C, K, dtype, ctypes.byref(cs), ctypes.byref(gps), ctypes.byref(ss),
                                            ctypes.byref(tps))
    return status, (cs.value, gps.value, ss.value, tps.value)


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_queries(lib, dtype):
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for q in (lib.sqfa_gauss_log_loss_workspace_bytes, lib.sqfa_gauss_log_loss_backward_workspace_bytes):
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
        # nothing of size N C or C N K: (N, C) float32 at N = 10^6, C = 1000 is 4 GB
        assert q(10 ** 6, 1000, 16, dtype) < 10 ** 6 * 1000 * 4
    # forward: the scores pass's workspace and one double per 64 samples
    for N, C, K in ((1, 1, 1), (100, 40, 8), (10 ** 6, 1000, 16)):
        fw = lib.sqfa_gauss_log_loss_workspace_bytes(N, C, K, dtype)
        sc = lib.sqfa_gauss_scores_workspace_bytes(N, C, K, dtype)
        assert sc + 8 * ((N + 63) // 64) <= fw <= sc + 8 * ((N + 63) // 64) + 512
    # backward: at most 16 class splits of (N, K + 1), more than one only while the samples alone do not fill the GPU, and a slab of the
    # sample splits that stays below 32 MB unless one split alone (the size of grad_cov and grad_means) is larger
    for N, C, K in ((1, 1, 1), (100, 40, 8), (2000, 300, 16), (60000, 1000, 16), (10 ** 6, 10, 64), (1000, 10 ** 5, 64)):
        status, (cs, gps, ss, tps) = _layout(lib, N, C, K, dtype)
        assert status == 0
        bw = lib.sqfa_gauss_log_loss_backward_workspace_bytes(N, C, K, dtype)
        per_class = (K * K + K + 1) * esz
        upart = cs * N * K * esz + cs * N * esz + N * esz   # u and P of every class split, P
        assert upart + ss * C * per_class <= bw <= upart + ss * C * per_class + 1024
        assert ss == 1 or ss * C * per_class <= 32 << 20
        assert cs == 1 or (cs - 1) * ((N + 63) // 64) < 1024   # the classes are split only below 1024 workgroups


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_layout_query(lib, dtype):
    for N, C, K in ((1, 1, 1), (17, 3, 3), (257, 17, 4), (2000, 300, 16), (65537, 5, 3), (10 ** 6, 1000, 64)):
        status, lay = _layout(lib, N, C, K, dtype)
        assert status == 0
        assert _layout(lib, N, C, K, dtype) == (0, lay)                       # deterministic
        cs, gps, ss, tps = lay
        groups, tiles = (C + 3) // 4, (N + 15) // 16
        assert 1 <= cs <= 16 and (cs - 1) * gps < groups <= cs * gps          # every split holds a group
        assert 1 <= ss <= 1024 and (ss - 1) * tps < tiles <= ss * tps         # every split holds a tile
    # both sides of each decision: few sample tiles split the classes, many do not; few tiles leave the samples unsplit
    assert _layout(lib, 2000, 300, 16, dtype)[1][0] > 1 and _layout(lib, 65537, 300, 16, dtype)[1][0] == 1
    assert _layout(lib, 256, 5, 3, dtype)[1][2] == 1 and _layout(lib, 2000, 5, 3, dtype)[1][2] > 1
    assert _layout(lib, 1000, 10, 65, dtype)[0] == -2
    assert _layout(lib, 0, 10, 4, dtype)[0] == -1
    assert _layout(lib, 1000, 10, 4, 7)[0] == -1
    assert lib.sqfa_gauss_log_loss_layout(1000, 10, 4, dtype, None, None, None, None) == -1


# (N, C, K): the shapes of tests/test_gpu_log_loss.py, the timing tools' large cases, and both sides of the class split
# (fewer and more than 1024 / 16 sample tiles, fewer groups of 4 classes than splits)
SPLIT_GRID = [(1, 1, 1), (65, 2, 1), (17, 3, 3), (257, 17, 4), (1000, 37, 16), (1000, 37, 17), (513, 130, 5), (300, 9, 33),
              (200, 5, 64), (100, 4, 48), (2000, 300, 16), (65537, 5, 3), (60000, 1000, 16), (60000, 1000, 32),
              (60000, 1000, 64), (65536, 300, 16), (65537, 300, 16), (64 * 1023, 5, 3), (64 * 1024, 5, 3), (64 * 63, 1000, 16),
              (64 * 64, 1000, 16), (64 * 64 + 1, 1000, 16), (64 * 70, 57, 16), (64 * 70, 61, 16), (10 ** 6, 1, 1)]


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_class_splits_are_those_of_the_scores_pass(lib, dtype):
    """The sample-owned backward pass splits the classes as the scores pass does: class_splits of the layout query against
    the splits the scores workspace implies -- splits * N * (3 * element size + 4) bytes where the classes are split (at
    least 32 bytes), the 16-byte minimum where they are not."""
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    seen = set()
    for N, C, K in SPLIT_GRID:
        status, (cs, _, _, _) = _layout(lib, N, C, K, dtype)
        assert status == 0
        ws = lib.sqfa_gauss_scores_workspace_bytes(N, C, K, dtype)
        if ws == 16:
            implied = 1
        else:
            assert ws % (N * (3 * esz + 4)) == 0
            implied = ws // (N * (3 * esz + 4))
            assert implied >= 2
        assert cs == implied, (N, C, K)
        seen.add(cs > 1)
    assert seen == {False, True}


def _forward(lib, Z=1, labels=1, N=100, means=0, W=1, off=1, C=4, K=8, dtype=_lib.SQFA_F32, loss=1, ll=0, lse=1, flags=1,
             ws=1, ws_bytes=1 << 26):
    p = lambda on: FAKE if on else NULL
    return lib.sqfa_gauss_log_loss(p(Z), p(labels), N, p(means), p(W), p(off), C, K, dtype, p(loss), p(ll), p(lse), p(flags),
                                   p(ws), ws_bytes, NULL)


def _backward(lib, Z=1, labels=1, N=100, means=1, W=1, off=1, C=4, K=8, dtype=_lib.SQFA_F32, lse=1, up=0, gZ=1, gmu=1, gcov=1,
              ws=1, ws_bytes=1 << 26):
    p = lambda on: FAKE if on else NULL
    return lib.sqfa_gauss_log_loss_backward(p(Z), p(labels), N, p(means), p(W), p(off), C, K, dtype, p(lse), p(up), p(gZ),
                                            p(gmu), p(gcov), p(ws), ws_bytes, NULL)


def test_forward_argument_validation(lib):
    for null in ("Z", "labels", "W", "off", "loss", "lse", "flags"):   # logsumexp_out and the flags are not optional
        assert _forward(lib, **{null: 0}) == -1, null
    assert b"sqfa_gauss_log_loss" in lib.sqfa_hip_last_error()
    for name in ("N", "C", "K"):
        assert _forward(lib, **{name: 0}) == -1
        assert _forward(lib, **{name: -1}) == -1
    assert _forward(lib, dtype=7) == -1
    assert b"dtype" in lib.sqfa_hip_last_error()
    assert _forward(lib, K=65) == -2                    # SQFA_ERR_UNSUPPORTED_M
    assert _forward(lib, K=128, means=1) == -2
    assert b"K > 64" in lib.sqfa_hip_last_error()
    assert _forward(lib, K=65, labels=0) == -1          # the argument checks come before the size check ...
    assert _forward(lib, K=65, dtype=7) == -1
    assert _forward(lib, K=65, ws_bytes=0) == -2        # ... and the size check before the workspace check
    assert _forward(lib, K=65, ws=0) == -2
    assert _forward(lib, N=2 ** 31 * 64 + 1) == -2      # more sample tiles than a grid holds
    assert _forward(lib, ws=0) == -3                    # SQFA_ERR_WORKSPACE
    assert _forward(lib, ws_bytes=8) == -3
    assert b"workspace" in lib.sqfa_hip_last_error()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):        # one byte short of the query, with and without class splits
        for N, C, K in ((100, 40, 8), (100, 1, 64), (10 ** 6, 1000, 16)):
            need = lib.sqfa_gauss_log_loss_workspace_bytes(N, C, K, dtype)
            assert _forward(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1) == -3
            assert _forward(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1, ll=1, means=1) == -3


def test_backward_argument_validation(lib):
    for null in ("Z", "labels", "W", "off", "lse"):
        assert _backward(lib, **{null: 0}) == -1, null
    for name in ("N", "C", "K"):
        assert _backward(lib, **{name: 0}) == -1
    assert _backward(lib, dtype=7) == -1
    assert _backward(lib, gZ=0, gmu=0, gcov=0) == -1    # nothing asked for
    assert b"no gradient" in lib.sqfa_hip_last_error()
    assert _backward(lib, means=0) == -1                # grad_means_out without means
    assert b"grad_means_out" in lib.sqfa_hip_last_error()
    assert _backward(lib, K=65) == -2
    assert b"K > 64" in lib.sqfa_hip_last_error()
    assert _backward(lib, K=65, lse=0) == -1            # BAD_ARGUMENT, UNSUPPORTED_M, WORKSPACE in that order
    assert _backward(lib, K=65, means=0) == -1
    assert _backward(lib, K=65, ws=0) == -2
    assert _backward(lib, N=2 ** 31 * 64 + 1) == -2
    assert _backward(lib, ws=0) == -3
    assert _backward(lib, ws_bytes=8) == -3
    assert b"workspace" in lib.sqfa_hip_last_error()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):        # one byte short, whatever subset is asked for
        for N, C, K in ((100, 40, 8), (100, 1, 64), (10 ** 6, 1000, 16)):
            need = lib.sqfa_gauss_log_loss_backward_workspace_bytes(N, C, K, dtype)
            for subset in (dict(), dict(gmu=0, gcov=0), dict(gZ=0), dict(gZ=0, gmu=0, means=0), dict(up=1)):
                assert _backward(lib, N=N, C=C, K=K, dtype=dtype, ws_bytes=need - 1, **subset) == -3
