"""CPU checks of the C ABI for matrix sizes 65..128 (the LDS pair kernel): sizes, tilings and workspace bounds are
answered on the host, without a device."""
import ctypes

import pytest

from sqfa_amd import _lib, _native

LARGE = [65, 72, 96, 127, 128]
UNSUPPORTED_M, ERR_WORKSPACE = -2, -3  # include/sqfa_hip.h


def _tiling(nA, nB, m, dtype):
    lib = _lib.load()
    out = [ctypes.c_int() for _ in range(5)]
    status = lib.sqfa_airm_tiling(nA, nB, m, dtype, *[ctypes.byref(v) for v in out])
    return status, [v.value for v in out]


def test_max_dim_is_128():
    assert _lib.load().sqfa_hip_max_dim() == 128


@pytest.mark.parametrize("dtype", [_lib.SQFA_F32, _lib.SQFA_F64])
@pytest.mark.parametrize("m", LARGE)
def test_tiling_and_workspace_large(m, dtype):
    lib = _lib.load()
    esz = 4 if dtype == _lib.SQFA_F32 else 8
    for nA, nB in ((300, 0), (40, 0), (2, 0), (7, 5), (30, 90)):
        status, (ti, tj, nbi, nbj, mr) = _tiling(nA, nB, m, dtype)
        assert status == 0
        nBe = nB or nA
        assert m <= mr <= 128 and mr % 8 == 0
        assert ti >= 1 and tj >= 1 and ti * nbi >= nA and tj * nbj >= nBe
        nbytes = lib.sqfa_airm_workspace_bytes(nA, nB, m, dtype)
        assert nbytes >= (nA + nBe // 2) * mr * mr * esz
        for shards in (1, 2, 3, 8):
            sh = lib.sqfa_airm_workspace_bytes_sharded(nA, nB, m, dtype, shards, 0)
            assert 0 < sh <= nbytes


def test_size_limits():
    lib = _lib.load()
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):
        assert _tiling(10, 0, 129, dtype)[0] == UNSUPPORTED_M
        assert lib.sqfa_airm_workspace_bytes(10, 0, 129, dtype) == 0
        assert lib.sqfa_airm_workspace_bytes(10, 0, 1000, dtype) == 0
        assert lib.sqfa_airm_workspace_bytes_sharded(10, 0, 129, dtype, 1, 0) == 0
    # the per-class SPD functions keep their own limit of 64
    assert lib.sqfa_spd_function_workspace_bytes(10, 65, 0) == 0
    assert lib.sqfa_spd_function_workspace_bytes(10, 64, 0) > 0


def test_pairwise_rejects_129_on_the_host():
    lib = _lib.load()
    z, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    status = lib.sqfa_airm_pairwise(fake, 4, z, 0, 129, 0, 1.0, 1e-6, 1, z, 0.0, 0, 1, z, z, z, z, z, z,
                                    fake, 1 << 30, z)
    assert status == UNSUPPORTED_M
    status = lib.sqfa_airm_pairwise(fake, 4, z, 0, 100, 0, 1.0, 1e-6, 1, z, 0.0, 0, 1, z, z, z, z, z, z,
                                    fake, 8, z)
    assert status == ERR_WORKSPACE


def test_workspace_bounds():
    lib = _lib.load()
    assert 0 < lib.sqfa_airm_workspace_bytes(1000, 0, 128, _lib.SQFA_F32) <= 3e9
    assert 0 < lib.sqfa_airm_workspace_bytes(100, 0, 128, _lib.SQFA_F64) <= 0.5e9


def test_small_launches_fill_the_chip():
    """C=100 gives at least 256 workgroups (one per tile) at every large size."""
    for m in LARGE:
        for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):
            _, (ti, tj, nbi, nbj, _) = _tiling(100, 0, m, dtype)
            tiles = sum(min(nbj, (bi * ti + ti - 2) // tj + 1) for bi in range(nbi))
            assert tiles >= 256


def test_boundary_64_keeps_the_register_geometry():
    for dtype in (_lib.SQFA_F32, _lib.SQFA_F64):
        status, (ti, tj, nbi, nbj, mr) = _tiling(1000, 0, 64, dtype)
        assert status == 0 and mr == 64 and 64 % ti == 0
        status, (_, _, _, _, mr65) = _tiling(1000, 0, 65, dtype)
        assert status == 0 and mr65 == 72


def test_spd_function_limit_is_its_own():
    assert _native.SPD_FUNCTION_MAX_DIM == 64

    class FakeCuda:  # the shape / dtype test of spd_function_supported, without a device
        is_cuda = True
        dtype = __import__("torch").float32
        shape = (3, 65, 65)

        def dim(self):
            return 3

        def numel(self):
            return 3 * 65 * 65

    assert not _native.spd_function_supported(FakeCuda())
    FakeCuda.shape = (3, 64, 64)
    assert _native.spd_function_supported(FakeCuda())
