"""CPU checks of the native orthogonal constraint's boundary: argument validation of sqfa_orthogonal_* on the host (fake
pointers, no launch), the shape test of _native.orthogonal_supported, and that constraint="orthogonal" still registers
torch's own parametrization class with torch's state_dict keys."""
import ctypes

import torch
from torch.nn.utils.parametrizations import _Orthogonal, orthogonal

from sqfa_amd import _lib, _native, constraints


def test_workspace_bytes():
    lib = _lib.load()
    for dt in (_lib.SQFA_F32, _lib.SQFA_F64):
        assert lib.sqfa_orthogonal_workspace_bytes(65, 784, dt) == 0
        assert lib.sqfa_orthogonal_workspace_bytes(16, 784, dt) > 16 * 784 * (4 if dt == _lib.SQFA_F32 else 8)
        assert lib.sqfa_orthogonal_workspace_bytes(64, 3072, dt) > 0
        assert lib.sqfa_orthogonal_workspace_bytes(8, 8, dt) == 0 and lib.sqfa_orthogonal_workspace_bytes(0, 8, dt) == 0
    assert lib.sqfa_orthogonal_workspace_bytes(16, 784, 7) == 0


def test_argument_validation_on_the_host():
    lib = _lib.load()
    z, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    big = 1 << 30
    fwd = lambda X=fake, base=fake, K=4, D=16, dt=0, F=fake, ws=fake, n=big: lib.sqfa_orthogonal_forward(X, base, K, D, dt, F, ws, n, z)
    bwd = lambda X=fake, base=fake, g=fake, K=4, D=16, dt=0, out=fake, ws=fake, n=big: lib.sqfa_orthogonal_backward(
        X, base, g, K, D, dt, out, ws, n, z)
    for call in (fwd, bwd):
        assert call(K=65, D=128) == -2
        assert call(K=16, D=16) == -1 and call(K=17, D=16) == -1 and call(K=0) == -1
        assert call(dt=5) == -1
        assert call(X=z) == -1 and call(base=z) == -1
        assert call(ws=z) == -3 and call(n=8) == -3
        need = lib.sqfa_orthogonal_workspace_bytes(4, 16, 0)
        assert call(n=need - 1) == -3
    assert fwd(F=z) == -1
    assert bwd(g=z) == -1 and bwd(out=z) == -1


class FakeCuda:
    """The shape / dtype / device test of orthogonal_supported, without a device."""
    is_cuda = True
    dtype = torch.float32
    device = "cuda:0"

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def test_orthogonal_supported_limits():
    assert _native.orthogonal_supported(FakeCuda(16, 784), FakeCuda(784, 784))
    assert _native.orthogonal_supported(FakeCuda(64, 65), FakeCuda(65, 65))
    assert not _native.orthogonal_supported(FakeCuda(65, 784), FakeCuda(784, 784))     # K > 64
    assert not _native.orthogonal_supported(FakeCuda(16, 16), FakeCuda(16, 16))        # K = D: torch's matrix_exp
    assert not _native.orthogonal_supported(FakeCuda(16, 784), FakeCuda(783, 783))
    assert not _native.orthogonal_supported(FakeCuda(16, 784), None)
    assert not _native.orthogonal_supported(torch.zeros(4, 16), torch.eye(16))        # CPU tensors
    wrong = FakeCuda(784, 784)
    wrong.dtype = torch.float64
    assert not _native.orthogonal_supported(FakeCuda(16, 784), wrong)


def test_model_keeps_torchs_parametrization():
    import sqfa_amd
    assert constraints.NATIVE_ORTHOGONAL is True
    for n_filters in (3, 8):   # Householder map, and square filters (matrix_exp)
        torch.manual_seed(5)
        model = sqfa_amd.model.SQFA(n_dim=8, n_filters=n_filters, feature_noise=0.01, constraint="orthogonal")
        par = model.parametrizations.filters[0]
        assert isinstance(par, _Orthogonal) and type(par) is constraints.Orthogonal
        # the same registration through torch itself: same keys, same random numbers, same values
        torch.manual_seed(5)
        twin = torch.nn.Module()
        twin.filters = torch.nn.Parameter(torch.randn(n_filters, 8))
        twin.register_buffer("noise_mat", 0.01 * torch.eye(n_filters))
        orthogonal(twin, "filters")
        assert sorted(model.state_dict()) == sorted(twin.state_dict())
        assert par.orthogonal_map == twin.parametrizations.filters[0].orthogonal_map
        assert torch.equal(par.base, twin.parametrizations.filters[0].base)
        assert torch.equal(model.parametrizations.filters.original, twin.parametrizations.filters.original)
        assert torch.equal(model.filters, twin.filters)       # CPU tensors: torch's own forward
        F = model.filters.detach()
        assert torch.allclose(F @ F.T, torch.eye(n_filters), atol=1e-5)
        # not a single-node closure on the CPU
        assert model._single_node_inputs({"means": torch.zeros(5, 8), "covariances": torch.eye(8).repeat(5, 1, 1)}) is None
