"""CPU checks of the class-statistics entry points of the C ABI: every argument check returns its code before any
HIP call (fake non-null pointers, nothing is launched), and the workspace query."""
import ctypes

import pytest

from sqfa_amd import _lib

Z, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(4096)


def moments(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_moments(g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z), g("class_start", FAKE),
                                          g("C", 3), g("dtype", 0), g("estimator", 0), g("means", FAKE), g("cov", FAKE),
                                          g("second", Z), g("ws", FAKE), g("nbytes", 1 << 30), Z)


def update(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_moments_update(g("points", FAKE), g("N", 10), g("D", 5), g("row_index", Z),
                                                 g("class_start", FAKE), g("C", 3), g("dtype", 0), g("counts", FAKE),
                                                 g("means", FAKE), g("m2", FAKE), g("ws", FAKE), g("nbytes", 1 << 30), Z)


def finalize(**kw):
    g = lambda k, d: kw.get(k, d)
    return _lib.load().sqfa_class_moments_finalize(g("counts", FAKE), g("means", FAKE), g("m2", FAKE), g("C", 3), g("D", 5),
                                                   g("dtype", 0), g("estimator", 0), g("cov", FAKE), g("second", Z),
                                                   g("ws", FAKE), g("nbytes", 1 << 30), Z)


def test_estimator_codes():
    from sqfa_amd import _native
    assert (_native.COV_EMPIRICAL, _native.COV_OAS, _native.COV_SCATTER) == (0, 1, 2)


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
def test_workspace_query(dtype):
    lib = _lib.load()
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for C, D in ((1, 1), (5, 63), (1000, 784), (1000, 2048), (100, 3072)):
        nbytes = lib.sqfa_class_moments_workspace_bytes(C, D, dtype)
        tiles = -(-D // 64)
        assert nbytes >= C * D * esz + C * (tiles * (tiles + 1) // 2) * 16   # batch means + {tr, sum sq} per tile
        assert nbytes < 64 << 20
    assert lib.sqfa_class_moments_workspace_bytes(10, 8, 7) == 0            # bad dtype
    assert lib.sqfa_class_moments_workspace_bytes(0, 8, dtype) == 0
    assert lib.sqfa_class_moments_workspace_bytes(10, 0, dtype) == 0
    assert lib.sqfa_class_moments_workspace_bytes(1 << 20, 8, dtype) == 0   # beyond the grid limits


def test_class_moments_argument_checks():
    for bad in (dict(points=Z), dict(class_start=Z), dict(means=Z), dict(cov=Z), dict(N=-1), dict(C=0), dict(D=0),
                dict(dtype=2), dict(dtype=-1), dict(estimator=3), dict(estimator=-1)):
        assert moments(**bad) == -1, bad
    assert moments(C=1 << 20) == -2
    assert moments(ws=Z) == -3
    assert moments(nbytes=8) == -3
    # the checks come in this order: a bad argument wins over a short workspace
    assert moments(dtype=9, nbytes=8) == -1 and moments(estimator=9, ws=Z) == -1


def test_class_moments_update_argument_checks():
    for bad in (dict(points=Z), dict(class_start=Z), dict(counts=Z), dict(means=Z), dict(m2=Z), dict(N=-1), dict(C=0),
                dict(D=0), dict(dtype=2)):
        assert update(**bad) == -1, bad
    assert update(C=1 << 20) == -2
    assert update(ws=Z) == -3 and update(nbytes=8) == -3


def test_class_moments_finalize_argument_checks():
    for bad in (dict(counts=Z), dict(means=Z), dict(m2=Z), dict(cov=Z), dict(C=0), dict(D=0), dict(dtype=2),
                dict(estimator=2), dict(estimator=-1)):
        assert finalize(**bad) == -1, bad
    assert finalize(C=1 << 20) == -2
    assert finalize(ws=Z) == -3 and finalize(nbytes=8) == -3
