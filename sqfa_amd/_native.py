"""torch <-> C-ABI glue for the pairwise SPD-distance kernels.

torch is used for device memory, streams and autograd bookkeeping only; all arithmetic of
the hot path happens inside libsqfa_hip.so.  The single call site of the library is
``hip_pair_backend`` (bound to the module attribute ``_pair_backend`` that the autograd
functions call through); it refuses CPU tensors and there is no other implementation in
this package.
"""
import collections
import ctypes
import math

import torch

from . import _lib
from ._memo import TensorMemo

EPSILON = 1e-6  # value added inside square roots (reference: src/sqfa/distances.py:29)


def _dtype_code(t):
    if t.dtype == torch.float32:
        return _lib.SQFA_F32
    if t.dtype == torch.float64:
        return _lib.SQFA_F64
    raise TypeError(f"sqfa_amd kernels support float32 and float64, got {t.dtype}")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def max_dim():
    return _lib.load().sqfa_hip_max_dim()


class _on_stream(torch.cuda.device):
    """with _on_stream(dev) as stream: `dev` is current (torch allocates there), `stream` its current stream as the C ABI's handle."""

    def __enter__(self):
        super().__enter__()
        return ctypes.c_void_p(torch.cuda.current_stream(self.idx).cuda_stream)


def _workspace(query, *args):
    """(uint8 workspace on the current device, its size) as the library's `query(*args)` asks for."""
    nbytes = query(*args)
    if nbytes == 0:
        raise _lib.NativeLibraryError(f"{query.__name__} rejected the problem shape")
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


# Per-call policies of the pair kernels (sqfa_airm_options, include/sqfa_hip.h), read at every launch -- from whichever
# thread launches (the autograd engine runs backward passes on its own).  The library itself holds no policy state.
#   geometry      0 small-launch lane geometries by pair count (default), 1 wherever one exists, -1 never
#   class_factor  0 class factor pass K0b by pair count (default), 1 always, -1 never
#   sweep_counter None, or an int64 CUDA tensor of two elements {sum of Jacobi sweeps, wave rounds} the kernel adds to
#   mean_metric   1 the factor pass works in the metric of the mean class where it can (opt-in: pays for classes that share a
#                 dominant covariance, loses 1-3 % on BASELINE's synthetic generator); 0 (default) plain inner product
#   launch        0 every fused launch that applies (default), -1 the separate launches throughout, 1 the fused class prologue
#                 only (a mask of the SQFA_LAUNCH_* bits); bit-identical results whatever the value
POLICY = {"geometry": 0, "class_factor": 0, "sweep_counter": None, "mean_metric": 0, "launch": 0}


class policies:
    """with policies(geometry=-1, class_factor=1): ...   (tests, A/B timing; restores the previous values)"""

    def __init__(self, **kw):
        unknown = set(kw) - set(POLICY)
        if unknown:
            raise TypeError(f"unknown policy {sorted(unknown)}")
        self.kw = kw

    def __enter__(self):
        self.saved = dict(POLICY)
        POLICY.update(self.kw)
        return self

    def __exit__(self, *exc):
        POLICY.clear()
        POLICY.update(self.saved)
        return False


def _options():
    cnt = POLICY["sweep_counter"]
    return _lib.AirmOptions(int(POLICY["geometry"]), int(POLICY["class_factor"]),
                            ctypes.c_void_p(cnt.data_ptr()) if cnt is not None else None, int(POLICY["mean_metric"]),
                            int(POLICY["launch"]))


def hip_pair_backend(A, B, *, scale, eps, sqrt_mode, weights, uniform_weight, shard,
                     want_loss, want_grad, want_dist, want_eig, out_loss=None, out_gradA=None, metric="airm"):
    """Run sqfa_airm_pairwise (metric "airm") or sqfa_bw_pairwise (metric "bw": Bures-Wasserstein, `scale` unused, no
    eigenvalues) on the current stream.  A (nA,m,m); B (nB,m,m) or None (self).
    Returns dict(loss, gradA, gradB, dist, eig, nonfinite) of freshly allocated tensors
    (None where not requested)."""
    if metric not in ("airm", "bw"):
        raise ValueError(f"unknown pair metric {metric!r}")
    if metric == "bw" and want_eig:
        raise ValueError("the Bures-Wasserstein pair path has no eigenvalue output")
    lib = _lib.load()
    if not A.is_cuda:
        raise RuntimeError(
            "sqfa_amd computes pairwise SPD distances on the GPU only (no CPU fallback): "
            "move the statistics/model to a HIP device, or pass your own distance_fun."
        )
    if B is not None and (B.device != A.device or B.dtype != A.dtype):
        raise ValueError("A and B must share device and dtype")
    A = A.detach().contiguous()
    nA, m = A.shape[0], A.shape[-1]
    if B is not None:
        B = B.detach().contiguous()
        nB = B.shape[0]
    else:
        nB = 0
    code = _dtype_code(A)
    if m > lib.sqfa_hip_max_dim():
        raise NotImplementedError(
            f"matrix size {m} exceeds the largest size the native pair kernels handle ({lib.sqfa_hip_max_dim()}: "
            "register kernels up to 64, the LDS kernel from 65 to 128)"
        )
    opts = _options()
    ws_query = lib.sqfa_bw_workspace_bytes_sharded if metric == "bw" else lib.sqfa_airm_workspace_bytes_sharded
    dev = A.device
    nBe = nA if B is None else nB
    with _on_stream(dev) as stream:
        ws, nbytes = _workspace(ws_query, nA, nB, m, code, int(shard[1]), opts.geometry_policy)
        # out_loss / out_gradA: caller-provided views (e.g. into a fused all-reduce buffer)
        # (loss and the two validity counters are always written by the finalize kernel: no memset)
        loss = (out_loss if out_loss is not None else torch.empty((), dtype=A.dtype, device=dev)) if want_loss else None
        nonfinite = torch.empty(2, dtype=torch.int32, device=dev)
        gradA = (out_gradA if out_gradA is not None else torch.empty_like(A)) if want_grad else None
        gradB = torch.empty_like(B) if (want_grad and B is not None) else None
        if want_dist:
            dist = (torch.zeros if shard[1] > 1 else torch.empty)((nA, nBe), dtype=A.dtype, device=dev)
        else:
            dist = None
        eig = torch.empty((nA, nBe, m), dtype=A.dtype, device=dev) if want_eig else None
        if weights is not None:
            weights = weights.detach().to(dtype=A.dtype, device=dev).contiguous()
            if tuple(weights.shape) != (nA, nBe):
                raise ValueError("pair weights must have shape (nA, nB)")
        if metric == "bw":
            status = lib.sqfa_bw_pairwise(
                _ptr(A), nA, _ptr(B), nB, m, code, float(eps), int(bool(sqrt_mode)),
                _ptr(weights), float(uniform_weight), int(shard[0]), int(shard[1]),
                _ptr(loss), _ptr(gradA), _ptr(gradB), _ptr(dist), _ptr(nonfinite),
                _ptr(ws), nbytes, stream, ctypes.byref(opts),
            )
            _lib.check(status, "sqfa_bw_pairwise")
            return {"loss": loss, "gradA": gradA, "gradB": gradB, "dist": dist, "eig": None, "nonfinite": nonfinite}
        status = lib.sqfa_airm_pairwise_opt(
            _ptr(A), nA, _ptr(B), nB, m, code,
            float(scale), float(eps), int(bool(sqrt_mode)),
            _ptr(weights), float(uniform_weight),
            int(shard[0]), int(shard[1]),
            _ptr(loss), _ptr(gradA), _ptr(gradB), _ptr(dist), _ptr(eig), _ptr(nonfinite),
            _ptr(ws), nbytes, stream, ctypes.byref(opts),
        )
    _lib.check(status, "sqfa_airm_pairwise_opt")
    return {"loss": loss, "gradA": gradA, "gradB": gradB, "dist": dist, "eig": eig, "nonfinite": nonfinite}


_pair_backend = hip_pair_backend


def normalized_pair_weights(pair_weights, n_classes, dtype, device):
    """The closures' static weight tensor of one fit: validates a (C,C) tensor-like of per-pair class weights on the host
    (ValueError naming the condition) and returns  Wn = -W / sum_{i>j} W_ij  with a zero diagonal, in `dtype` on `device`,
    so that  sum_{i>j} Wn_ij D_ij  is the loss  -sum_{i>j} W_ij D_ij / sum_{i>j} W_ij.  None stays None."""
    if pair_weights is None:
        return None
    W = torch.as_tensor(pair_weights).detach().to(device="cpu", dtype=torch.float64)
    C = int(n_classes)
    if tuple(W.shape) != (C, C):
        raise ValueError(f"pair_weights must have shape (n_classes, n_classes) = ({C}, {C}), got {tuple(W.shape)}")
    if not bool(torch.isfinite(W).all()):
        raise ValueError("pair_weights must be finite (found NaN or inf)")
    if bool((W < 0).any()):
        raise ValueError("pair_weights must be non-negative")
    if not bool(torch.equal(W, W.t())):
        raise ValueError("pair_weights must be symmetric")
    total = torch.tril(W, -1).sum()
    if not float(total) > 0.0:
        raise ValueError("pair_weights must have a positive sum over the pairs i > j")
    Wn = -W / total
    Wn.fill_diagonal_(0.0)
    return Wn.to(device=device, dtype=dtype).contiguous()


def _self_pair_weights(pair_weights):
    """What the affine-invariant / Bures-Wasserstein kernels take for the closure's symmetric weights: in self mode they
    weigh the unordered pair with w_ij + w_ji, so they get the strict lower triangle."""
    return None if pair_weights is None else torch.tril(pair_weights, -1)


# ------------------------------------------------------------------------------------------
# autograd wrappers


class PairDistanceMatrix(torch.autograd.Function):
    """D[i,j] = dist(A_i, B_j) as a differentiable (nA,nB) matrix.  The backward pass
    re-evaluates the pairs with the incoming gradient as per-pair weights (nothing of
    size nA*nB*m*m is ever stored)."""

    @staticmethod
    def forward(ctx, A, B, scale, eps, sqrt_mode, metric="airm"):
        kw = {"metric": metric} if metric != "airm" else {}
        out = _pair_backend(A, B, scale=scale, eps=eps, sqrt_mode=sqrt_mode, weights=None,
                            uniform_weight=0.0, shard=(0, 1), want_loss=False, want_grad=False,
                            want_dist=True, want_eig=False, **kw)
        ctx.save_for_backward(A, B if B is not None else A.new_empty(0))
        ctx.self_mode = B is None
        ctx.cfg = (scale, eps, sqrt_mode)
        ctx.kw = kw
        ctx.mark_non_differentiable(out["nonfinite"])
        return out["dist"], out["nonfinite"]

    @staticmethod
    def backward(ctx, gD, _gflag):
        A, B = ctx.saved_tensors
        B = None if ctx.self_mode else B
        scale, eps, sqrt_mode = ctx.cfg
        out = _pair_backend(A, B, scale=scale, eps=eps, sqrt_mode=sqrt_mode, weights=gD,
                            uniform_weight=0.0, shard=(0, 1), want_loss=False, want_grad=True,
                            want_dist=False, want_eig=False, **ctx.kw)
        return out["gradA"], out["gradB"], None, None, None, None


def fused_reduce_owner(reducer, shard):
    """The reducer's owner when a sharded evaluation goes through the fused all-reduce buffer [loss, nan, inf, grad...] (the
    pair kernel writes loss and gradient straight into it: no packing copies, ONE all-reduce), else None."""
    owner = getattr(reducer, "__self__", None)
    if reducer is not None and shard[1] > 1 and _pair_backend is hip_pair_backend and hasattr(owner, "reduce_fused"):
        return owner
    return None


def fused_buffer(shape, dtype, device):
    return torch.empty(math.prod(shape) + 3, dtype=dtype, device=device)


def fused_outputs(fused, shape):
    """The views of the buffer that the pair backend writes through (its out_loss / out_gradA arguments)."""
    return {"out_loss": fused[0], "out_gradA": fused[3:].view(shape)}


class _SavedGradientLoss(torch.autograd.Function):
    """Base of the fused closure losses: forward gets loss, flags and the gradients of the first inputs from ONE native
    pass and keeps the gradients (`_saved`); backward only scales them by the upstream gradient of the loss."""

    @staticmethod
    def _saved(ctx, n_inputs, loss, nonfinite, *grads):
        """`grads`: one per leading input, None for an absent one (the means of a means-free loss)."""
        ctx.save_for_backward(*(g for g in grads if g is not None))
        ctx.present = tuple(g is not None for g in grads)
        ctx.n_inputs = n_inputs
        ctx.mark_non_differentiable(nonfinite)
        return loss, nonfinite

    @staticmethod
    def backward(ctx, gloss, _gflag):
        saved = iter(ctx.saved_tensors)
        grads = tuple(next(saved) * gloss if present else None for present in ctx.present)
        return grads + (None,) * (ctx.n_inputs - len(grads))


class PairwiseLoss(_SavedGradientLoss):
    """Fused closure loss: sum over the unordered pairs i>j of  weight * dist(S_i, S_j)
    (weight = -1/P gives the reference's -mean, src/sqfa/_optim.py:94) together with its
    gradient, in one pass.  `reducer(loss, nonfinite, grad)` combines shards (all-reduce).  `pair_weights`: the symmetric
    (C,C) per-pair weights of normalized_pair_weights in place of `weight`."""

    @staticmethod
    def forward(ctx, S, scale, eps, sqrt_mode, weight, shard, reducer, metric="airm", pair_weights=None):
        extra = {"metric": metric} if metric != "airm" else {}
        owner = fused_reduce_owner(reducer, shard)
        fused = fused_buffer(S.shape, S.dtype, S.device) if owner is not None else None
        if fused is not None:
            extra.update(fused_outputs(fused, S.shape))
        out = _pair_backend(S, None, scale=scale, eps=eps, sqrt_mode=sqrt_mode, weights=_self_pair_weights(pair_weights),
                            uniform_weight=weight, shard=shard, want_loss=True, want_grad=True,
                            want_dist=False, want_eig=False, **extra)
        loss, nonfinite, grad = out["loss"], out["nonfinite"], out["gradA"]
        if fused is not None:
            loss, nonfinite, grad = owner.reduce_fused(fused, nonfinite, S.shape)
        elif reducer is not None:
            loss, nonfinite, grad = reducer(loss, nonfinite, grad)
        return _SavedGradientLoss._saved(ctx, 9, loss, nonfinite, grad)


def hip_eigenvalues_backward(A, B, eig_weights):
    """sqfa_airm_eigenvalues_backward on the current stream: gradients of sum(eig_weights * eig)
    wrt A (nA,m,m) and B (nB,m,m), `eig_weights` (nA,nB,m) in the kernel's unsorted column order."""
    lib = _lib.load()
    if not A.is_cuda:
        raise RuntimeError("sqfa_amd computes generalized eigenvalues on the GPU only (no CPU fallback)")
    A = A.detach().contiguous()
    B = B.detach().contiguous()
    W = eig_weights.detach().to(A.dtype).contiguous()
    nA, nB, m = A.shape[0], B.shape[0], A.shape[-1]
    code = _dtype_code(A)
    with _on_stream(A.device) as stream:
        ws, nbytes = _workspace(lib.sqfa_airm_workspace_bytes, nA, nB, m, code)
        gA, gB = torch.empty_like(A), torch.empty_like(B)
        opts = _options()   # the policies of the forward call: the kernel's eigenvalue order depends on the lane geometry
        status = lib.sqfa_airm_eigenvalues_backward(_ptr(A), nA, _ptr(B), nB, m, code, _ptr(W), _ptr(gA), _ptr(gB),
                                                    _ptr(ws), nbytes, stream, ctypes.byref(opts))
    _lib.check(status, "sqfa_airm_eigenvalues_backward")
    return gA, gB


_eig_backward_backend = hip_eigenvalues_backward


class GeneralizedEigenvalues(torch.autograd.Function):
    """(nA,nB,m) generalized eigenvalues of every pair (A_i, B_j), descending, differentiable
    (the reference's generalized_eigenvalues is autograd-transparent, src/sqfa/linalg.py:48-70).
    The kernel returns the eigenvalues in its own (deterministic) column order; the sort
    permutation is kept and the upstream gradient is scattered back through it, then one
    more launch evaluates sum_k w_k dlambda_k/d(A,B) in closed form (u u^T, -lambda u u^T)."""

    @staticmethod
    def forward(ctx, A, B):
        out = _pair_backend(A, B, scale=1.0, eps=EPSILON, sqrt_mode=False, weights=None,
                            uniform_weight=0.0, shard=(0, 1), want_loss=False, want_grad=False,
                            want_dist=False, want_eig=True)
        lam, order = torch.sort(out["eig"], dim=-1, descending=True)
        ctx.save_for_backward(A, B, order)
        return lam

    @staticmethod
    def backward(ctx, g_lam):
        A, B, order = ctx.saved_tensors
        w = torch.zeros_like(g_lam).scatter_(-1, order, g_lam)
        gA, gB = _eig_backward_backend(A, B, w)
        return gA, gB


def generalized_eigenvalues_raw(A, B):
    """(nA,nB,m) generalized eigenvalues of (A_i, B_j), descending; differentiable wrt A and B."""
    return GeneralizedEigenvalues.apply(A, B)


# ------------------------------------------------------------------------------------------
# Gaussian pair terms (bhattacharyya / mahalanobis / hellinger / fisher_rao_same_cov)


def _gauss_padded_size(m, n_pairs):
    """The one-pair-per-lane kernel reads whole 16-byte rows when the matrices ARE its padded size (4 / 8 / 12 / 16): from
    20000 pairs on the callers pad with an identity block themselves (_pad_gauss) instead of letting the kernel pad with
    scalar loads and selects (K=15 at C=1000: 1.11 -> 0.55 ms forward + backward)."""
    return (m + 3) // 4 * 4 if (m < 16 and m % 4 != 0 and n_pairs >= 20000) else m


def _pad_gauss(mu, cov, M):
    """Identity padding of (n,m) means / (n,m,m) covariances to size M: exact for Q, logdet and the distances built on
    them (log 1 = 0; the padded coordinates have delta = 0)."""
    m = cov.shape[-1]
    cov_p = torch.eye(M, dtype=cov.dtype, device=cov.device).repeat(cov.shape[0], 1, 1)
    cov_p[:, :m, :m] = cov
    return torch.nn.functional.pad(mu, (0, M - m)), cov_p


def hip_gauss_terms(muA, covA, muB, covB, gQ=None, gLD=None, want_outputs=True, want_grad=False):
    """sqfa_gauss_pair_terms on the current stream.  Returns (Q, LD, gmuA, gcovA) (None where not requested)."""
    lib = _lib.load()
    if not covA.is_cuda:
        raise RuntimeError("sqfa_amd's native Gaussian pair terms run on the GPU only")
    muA, covA, muB, covB = (t.detach().contiguous() for t in (muA, covA, muB, covB))
    nA, nB, m = covA.shape[0], covB.shape[0], covA.shape[-1]
    m_true, m = m, _gauss_padded_size(m, nA * nB)
    if m != m_true:
        same = muB.data_ptr() == muA.data_ptr() and covB.data_ptr() == covA.data_ptr() and nA == nB   # B is A: pad once
        muA, covA = _pad_gauss(muA, covA, m)
        muB, covB = (muA, covA) if same else _pad_gauss(muB, covB, m)
    code = _dtype_code(covA)
    dev, dt = covA.device, covA.dtype
    with _on_stream(dev) as stream:
        Q = torch.empty((nA, nB), dtype=dt, device=dev) if want_outputs else None
        LD = torch.empty((nA, nB), dtype=dt, device=dev) if want_outputs else None
        gmu = torch.empty((nA, m), dtype=dt, device=dev) if want_grad else None
        gcov = torch.empty((nA, m, m), dtype=dt, device=dev) if want_grad else None
        gQ = gQ.detach().to(dt).contiguous() if gQ is not None else None
        gLD = gLD.detach().to(dt).contiguous() if gLD is not None else None
        status = lib.sqfa_gauss_pair_terms(_ptr(muA), _ptr(covA), nA, _ptr(muB), _ptr(covB), nB, m, code,
                                           _ptr(gQ), _ptr(gLD), _ptr(Q), _ptr(LD), _ptr(gmu), _ptr(gcov), stream)
    _lib.check(status, "sqfa_gauss_pair_terms")
    if m != m_true and want_grad:
        gmu, gcov = gmu[:, :m_true].contiguous(), gcov[:, :m_true, :m_true].contiguous()
    return Q, LD, gmu, gcov


GAUSS_MAX_DIM = 64


class GaussPairTerms(torch.autograd.Function):
    """Q_ij = (mu_i-mu_j)^T Sbar_ij^-1 (mu_i-mu_j) and LD_ij = logdet Sbar_ij with
    Sbar_ij = (Sigma_i + Sigma_j)/2, as differentiable (nA,nB) matrices -- the pair-dependent part of
    the reference's bhattacharyya / mahalanobis / hellinger / fisher_rao_same_cov
    (src/sqfa/distances.py:240-432), without the (nA,nB,K,K) tensor those build.  `same` marks the
    self case (B is A): one backward launch with symmetrised upstream gradients."""

    @staticmethod
    def forward(ctx, muA, covA, muB, covB, same):
        Q, LD, _, _ = hip_gauss_terms(muA, covA, muB, covB)
        ctx.save_for_backward(muA, covA, muB, covB)
        ctx.same = same
        return Q, LD

    @staticmethod
    def backward(ctx, gQ, gLD):
        muA, covA, muB, covB = ctx.saved_tensors
        if ctx.same:
            _, _, gmu, gcov = hip_gauss_terms(muA, covA, muA, covA, gQ + gQ.t(), gLD + gLD.t(),
                                              want_outputs=False, want_grad=True)
            return gmu, gcov, None, None, None
        _, _, gmuA, gcovA = hip_gauss_terms(muA, covA, muB, covB, gQ, gLD, want_outputs=False, want_grad=True)
        _, _, gmuB, gcovB = hip_gauss_terms(muB, covB, muA, covA, gQ.t(), gLD.t(), want_outputs=False, want_grad=True)
        return gmuA, gcovA, gmuB, gcovB, None


def _pair_weight_matrix(pair_weights, n, dtype, device):
    """(n,n) per-pair weights as the fused entries read them: contiguous, the statistics' dtype and device."""
    if pair_weights is None:
        return None
    W = pair_weights.detach().to(dtype=dtype, device=device).contiguous()
    if tuple(W.shape) != (n, n):
        raise ValueError(f"pair weights must have shape ({n}, {n}), got {tuple(W.shape)}")
    return W


# ------------------------------------------------------------------------------------------
# fused class-pair losses: per-class pre-stages, ONE pass over the ordered class pairs, a one-workgroup reduction

SPD_FUNCTION_MAX_DIM = 64   # the per-class SPD functions (log_euclidean's pre-stage; see spd_function_supported)
JEFFREYS_MAX_DIM = 64

# One row per family.  entry: the C entry that takes pair weights (NULL: uniform); name: what _lib.check reports; query: the
# workspace query; limit: the largest matrix size; means: whether the entry takes means and returns their gradient; what,
# size_error: the wording of the family's error messages.
PairFamily = collections.namedtuple("PairFamily", "entry name query limit means what size_error")
PAIR_FAMILIES = {
    "gauss": PairFamily("sqfa_gauss_pairwise_loss_weighted", "sqfa_gauss_pairwise_loss", "sqfa_gauss_pairwise_workspace_bytes",
                        GAUSS_MAX_DIM, True, "Gaussian",
                        "feature dimension {m} exceeds the native Gaussian pair kernels' limit ({limit})"),
    "log_euclidean": PairFamily("sqfa_log_euclidean_pairwise_loss_weighted", "sqfa_log_euclidean_pairwise_loss",
                                "sqfa_log_euclidean_workspace_bytes", SPD_FUNCTION_MAX_DIM, False, "log-Euclidean",
                                "matrix size {m} exceeds the native per-class SPD functions' limit ({limit})"),
    "jeffreys": PairFamily("sqfa_jeffreys_pairwise_loss", "sqfa_jeffreys_pairwise_loss", "sqfa_jeffreys_workspace_bytes",
                           JEFFREYS_MAX_DIM, True, "Jeffreys",
                           "feature dimension {m} exceeds the native Jeffreys kernels' limit ({limit})"),
}


# The Stein family (sqfa_amd.logdet) has its own table: the keys of PAIR_FAMILIES are the three families the registry was
# unified over, and tests pin them.  pair_family() is the lookup over both.
STEIN_MAX_DIM = 64
LOGDET_PAIR_FAMILIES = {
    "stein": PairFamily("sqfa_stein_pairwise_loss", "sqfa_stein_pairwise_loss", "sqfa_stein_workspace_bytes", STEIN_MAX_DIM,
                        False, "Stein", "matrix size {m} exceeds the native Stein kernels' limit ({limit})"),
}


def pair_family(family):
    """The PairFamily row of a class-pair family, whichever table holds it."""
    row = PAIR_FAMILIES.get(family)
    return row if row is not None else LOGDET_PAIR_FAMILIES[family]


def _class_pair_call(family, mu, cov, mode, eps, weight, want_grad, want_dist, pair_weights):
    """One fused class-pair loss on the current stream (no host read-back, workspace from the torch allocator: safe inside
    a graph capture): cov (n,m,m) SPD, mu (n,m) or None, `mode` the family's kind code / sqrt_mode, `pair_weights` symmetric
    (n,n) per-pair weights in place of `weight`.  Returns dict(loss, gmu, gcov, dist, nonfinite) (None where not requested;
    gmu None without means)."""
    fam = pair_family(family)
    lib = _lib.load()
    if not cov.is_cuda:
        raise RuntimeError(f"sqfa_amd's fused {fam.what} pair loss runs on the GPU only (no CPU fallback)")
    if mu is not None and (mu.device != cov.device or mu.dtype != cov.dtype):
        raise ValueError("means and covariances must share device and dtype")
    cov = cov.detach().contiguous()
    mu = mu.detach().contiguous() if mu is not None else None
    n, m = cov.shape[0], cov.shape[-1]
    if m > fam.limit:
        raise NotImplementedError(fam.size_error.format(m=m, limit=fam.limit))
    code = _dtype_code(cov)
    dev, dt = cov.device, cov.dtype
    with _on_stream(dev) as stream:
        ws, nbytes = _workspace(getattr(lib, fam.query), n, m, code)
        loss = torch.empty((), dtype=dt, device=dev)
        nonfinite = torch.empty(2, dtype=torch.int32, device=dev)
        gmu = torch.empty((n, m), dtype=dt, device=dev) if want_grad and mu is not None else None
        gcov = torch.empty((n, m, m), dtype=dt, device=dev) if want_grad else None
        dist = torch.empty((n, n), dtype=dt, device=dev) if want_dist else None
        W = _pair_weight_matrix(pair_weights, n, dt, dev)
        means_in, means_out = ((_ptr(mu),), (_ptr(gmu),)) if fam.means else ((), ())
        status = getattr(lib, fam.entry)(*means_in, _ptr(cov), n, m, code, int(mode), float(eps), _ptr(W),
                                         0.0 if W is not None else float(weight), _ptr(loss), *means_out, _ptr(gcov),
                                         _ptr(dist), _ptr(nonfinite), _ptr(ws), nbytes, stream)
    _lib.check(status, fam.name)
    return {"loss": loss, "gmu": gmu, "gcov": gcov, "dist": dist, "nonfinite": nonfinite}


def class_pair_loss(family, mu, cov, mode, eps, weight, want_grad=True, want_dist=False, pair_weights=None):
    """_class_pair_call, with the Gaussian family's identity padding around it (`pair_weights` are never padded: the
    padding changes K, not the classes)."""
    m = cov.shape[-1]
    M = _gauss_padded_size(m, cov.shape[0] * cov.shape[0]) if family == "gauss" else m
    if M != m:
        mu, cov = _pad_gauss(mu.detach(), cov.detach(), M)
    out = _class_pair_call(family, mu, cov, mode, eps, weight, want_grad, want_dist, pair_weights)
    if M != m and want_grad:
        out["gmu"], out["gcov"] = out["gmu"][:, :m].contiguous(), out["gcov"][:, :m, :m].contiguous()
    return out


def hip_gauss_pairwise_loss(mu, cov, kind, eps, weight, want_grad=True, want_dist=False, pair_weights=None):
    """sqfa_gauss_pairwise_loss_weighted on the current stream (class_pair_loss, family "gauss"; kind: _lib.SQFA_GAUSS_*).
    Returns dict(loss, gmu, gcov, dist, nonfinite) (None where not requested)."""
    return class_pair_loss("gauss", mu, cov, kind, eps, weight, want_grad, want_dist, pair_weights)


def hip_log_euclidean_pairwise_loss(S, sqrt_mode, eps, weight, want_grad=True, want_dist=False, pair_weights=None):
    """sqfa_log_euclidean_pairwise_loss_weighted on the current stream (class_pair_loss, family "log_euclidean"): S (n,m,m)
    SPD.  Returns dict(loss, gS, dist, nonfinite) (None where not requested)."""
    out = class_pair_loss("log_euclidean", None, S, bool(sqrt_mode), eps, weight, want_grad, want_dist, pair_weights)
    return {"loss": out["loss"], "gS": out["gcov"], "dist": out["dist"], "nonfinite": out["nonfinite"]}


def hip_jeffreys_pairwise_loss(mu, cov, sqrt_mode, eps, weight, want_grad=True, want_dist=False, pair_weights=None):
    """sqfa_jeffreys_pairwise_loss on the current stream (class_pair_loss, family "jeffreys"): cov (n,m,m) SPD, mu (n,m) or
    None (zero means).  Returns dict(loss, gmu, gcov, dist, nonfinite) (None where not requested; gmu None without means)."""
    return class_pair_loss("jeffreys", mu, cov, bool(sqrt_mode), eps, weight, want_grad, want_dist, pair_weights)


def hip_stein_pairwise_loss(S, sqrt_mode, eps, weight, want_grad=True, want_dist=False, pair_weights=None):
    """sqfa_stein_pairwise_loss on the current stream (class_pair_loss, family "stein"): S (n,m,m) SPD.  Returns dict(loss,
    gS, dist, nonfinite) (None where not requested)."""
    out = class_pair_loss("stein", None, S, bool(sqrt_mode), eps, weight, want_grad, want_dist, pair_weights)
    return {"loss": out["loss"], "gS": out["gcov"], "dist": out["dist"], "nonfinite": out["nonfinite"]}


class ClassPairLoss(_SavedGradientLoss):
    """Fused closure loss of a class-pair family (PAIR_FAMILIES): weight * sum over the unordered class pairs of the
    distance, with its gradient wrt means (C,K) (None for a means-free loss: log_euclidean, jeffreys_spd) and covariances
    (C,K,K), from ONE native call -- in place of the operator's torch / per-pair-term expression, the tril gather, the mean
    and their autograd backward.  family "gauss": bhattacharyya / hellinger / mahalanobis[_sq] (mode: _lib.SQFA_GAUSS_*);
    "log_euclidean": log_euclidean (mode True) / log_euclidean_sq (False), the pass over the pairs between the per-class
    logarithm and its Daleckii-Krein backward; "jeffreys": jeffreys[_spd] (mode False) / their _root forms (True); "stein":
    logdet.stein (False) / stein_root (True).
    Returns (loss, flags {#NaN, #inf})."""

    @staticmethod
    def forward(ctx, means, covariances, family, mode, eps, weight, pair_weights=None):
        out = class_pair_loss(family, means, covariances, mode, eps, weight, pair_weights=pair_weights)
        return _SavedGradientLoss._saved(ctx, 7, out["loss"], out["nonfinite"], out["gmu"], out["gcov"])


# ------------------------------------------------------------------------------------------
# per-class matrix functions (spd_log / spd_sqrt: log_euclidean's building block)

SPD_LOG, SPD_SQRT, SPD_INV_SQRT = 0, 1, 2
# the per-class SPD functions have their own size limit, SPD_FUNCTION_MAX_DIM (the pair kernels go to sqfa_hip_max_dim() =
# 128); larger matrices keep the eigh path of linalg.py


def spd_function_supported(M):
    return (M.is_cuda and M.dtype in (torch.float32, torch.float64) and M.dim() >= 2 and M.shape[-1] == M.shape[-2]
            and 1 <= M.shape[-1] <= SPD_FUNCTION_MAX_DIM and M.numel() > 0)


class SpdFunction(torch.autograd.Function):
    """f(S) = Q f(Lambda) Q^T for a batch (n,m,m) of SPD matrices through sqfa_spd_function (Cholesky + one-sided Jacobi
    per class, double inside), differentiable through sqfa_spd_function_backward (Daleckii-Krein).  Replaces the
    reference's torch.linalg.eigh + einsum (src/sqfa/linalg.py:121-141, 165-183) and eigh's autograd backward."""

    @staticmethod
    def forward(ctx, S, kind):
        lib = _lib.load()
        S3 = S.detach().contiguous()
        n, m = S3.shape[0], S3.shape[-1]
        code = _dtype_code(S3)
        dev = S3.device
        with _on_stream(dev) as stream:
            ws, nbytes = _workspace(lib.sqfa_spd_function_workspace_bytes, n, m, code)
            F = torch.empty_like(S3)
            U = torch.empty((n, m, m), dtype=torch.float64, device=dev)
            lam = torch.empty((n, m), dtype=torch.float64, device=dev)
            _lib.check(lib.sqfa_spd_function(_ptr(S3), n, m, code, int(kind), _ptr(F), _ptr(U), _ptr(lam), _ptr(ws), nbytes, stream),
                       "sqfa_spd_function")
        ctx.save_for_backward(U, lam)
        ctx.kind = int(kind)
        return F

    @staticmethod
    def backward(ctx, gF):
        U, lam = ctx.saved_tensors
        lib = _lib.load()
        G = gF.detach().contiguous()
        n, m = G.shape[0], G.shape[-1]
        with _on_stream(G.device) as stream:
            gS = torch.empty_like(G)
            _lib.check(lib.sqfa_spd_function_backward(_ptr(U), _ptr(lam), _ptr(G), n, m, _dtype_code(G), ctx.kind, _ptr(gS), stream),
                       "sqfa_spd_function_backward")
        return gS, None


def spd_function(M, kind):
    """(..., m, m) -> (..., m, m) on the native kernels (the caller has checked spd_function_supported)."""
    lead = M.shape[:-2]
    out = SpdFunction.apply(M.reshape(-1, M.shape[-2], M.shape[-1]), kind)
    return out.reshape(*lead, M.shape[-2], M.shape[-1])


# ------------------------------------------------------------------------------------------
# class statistics from labelled points (class_moments_kernel.hip)

COV_EMPIRICAL, COV_OAS, COV_SCATTER = 0, 1, 2


def class_moments_supported(points):
    return points.is_cuda and points.dim() == 2 and points.dtype in (torch.float32, torch.float64) and points.shape[1] >= 1


def grouped_rows(labels, n_classes):
    """(order, class_start) of integer labels on their device: the indices of a stable sort and the exclusive cumulative
    class sizes (C+1, int64) -- what sqfa_class_moments gathers rows by.  No host read."""
    order = torch.sort(labels, stable=True).indices
    class_start = torch.zeros(n_classes + 1, dtype=torch.int64, device=labels.device)
    class_start[1:] = torch.cumsum(torch.bincount(labels, minlength=n_classes), 0)
    return order, class_start


def class_moments(points, order, class_start, C, estimator, want_second=True):
    """sqfa_class_moments on the current stream: (means (C,D), covariances (C,D,D), second moments or None) of the rows
    `points[order]` grouped by `class_start` (order None: already grouped).  estimator: COV_EMPIRICAL / COV_OAS / COV_SCATTER."""
    lib = _lib.load()
    if not class_moments_supported(points):
        raise RuntimeError("sqfa_amd's class statistics kernels take (N, D) float32 / float64 points on the GPU")
    points = points.detach().contiguous()
    N, D = points.shape
    code = _dtype_code(points)
    dev, dt = points.device, points.dtype
    with _on_stream(dev) as stream:
        ws, nbytes = _workspace(lib.sqfa_class_moments_workspace_bytes, C, D, code)
        means = torch.empty((C, D), dtype=dt, device=dev)
        cov = torch.empty((C, D, D), dtype=dt, device=dev)
        second = torch.empty((C, D, D), dtype=dt, device=dev) if want_second and estimator != COV_SCATTER else None
        _lib.check(lib.sqfa_class_moments(_ptr(points), N, D, _ptr(order), _ptr(class_start), C, code, int(estimator),
                                          _ptr(means), _ptr(cov), _ptr(second), _ptr(ws), nbytes, stream),
                   "sqfa_class_moments")
    return means, cov, second


def class_moments_update(points, order, class_start, C, counts, means, m2):
    """sqfa_class_moments_update on the current stream: merges the batch `points[order]` grouped by `class_start` into the
    running counts (C, float64), means (C,D) and m2 (C,D,D), in place."""
    lib = _lib.load()
    if not class_moments_supported(points) or points.dtype != means.dtype:
        raise RuntimeError("sqfa_amd's class statistics kernels take (N, D) float32 / float64 points on the GPU")
    points = points.detach().contiguous()
    N, D = points.shape
    code = _dtype_code(points)
    with _on_stream(points.device) as stream:
        ws, nbytes = _workspace(lib.sqfa_class_moments_workspace_bytes, C, D, code)
        _lib.check(lib.sqfa_class_moments_update(_ptr(points), N, D, _ptr(order), _ptr(class_start), C, code,
                                                 _ptr(counts), _ptr(means), _ptr(m2), _ptr(ws), nbytes, stream),
                   "sqfa_class_moments_update")


def class_moments_finalize(counts, means, m2, estimator, want_second=True):
    """sqfa_class_moments_finalize: (covariances, second moments or None) from an accumulator's state."""
    lib = _lib.load()
    C, D = means.shape
    code = _dtype_code(means)
    with _on_stream(means.device) as stream:
        ws, nbytes = _workspace(lib.sqfa_class_moments_workspace_bytes, C, D, code)
        cov = torch.empty_like(m2)
        second = torch.empty_like(m2) if want_second else None
        _lib.check(lib.sqfa_class_moments_finalize(_ptr(counts), _ptr(means), _ptr(m2), C, D, code, int(estimator),
                                                   _ptr(cov), _ptr(second), _ptr(ws), nbytes, stream),
                   "sqfa_class_moments_finalize")
    return cov, second


# ------------------------------------------------------------------------------------------
# feature moments straight from the labelled points (class_points_kernel.hip): nothing of size (C,D,D)

POINT_MAX_FILTERS = 64


def class_means(points, order, class_start, C):
    """sqfa_class_means on the current stream: the (C,D) class means of `points[order]` grouped by `class_start`, the same
    bits as class_moments' means."""
    lib = _lib.load()
    if not class_moments_supported(points) or not points.is_contiguous():
        raise RuntimeError("sqfa_amd's class statistics kernels take contiguous (N, D) float32 / float64 points on the GPU")
    N, D = points.shape
    with _on_stream(points.device) as stream:
        means = torch.empty((C, D), dtype=points.dtype, device=points.device)
        _lib.check(lib.sqfa_class_means(_ptr(points), N, D, _ptr(order), _ptr(class_start), C, _dtype_code(points),
                                        _ptr(means), stream), "sqfa_class_means")
    return means


def class_shrinkage(points, order, class_start, means, C):
    """sqfa_class_shrinkage on the current stream: (keep (C), shift (C) in the dtype, rho (C) float64) of the OAS shrinkage
    OAS(S_c) = keep_c S_c + shift_c I of the classes of `points[order]` grouped by `class_start`, from the points and their
    `means` (class_means) alone: the bits class_moments(COV_OAS) applies, with nothing of size (D,D) written."""
    lib = _lib.load()
    if not class_moments_supported(points) or not points.is_contiguous():
        raise RuntimeError("sqfa_amd's class statistics kernels take contiguous (N, D) float32 / float64 points on the GPU")
    N, D = points.shape
    code = _dtype_code(points)
    dev, dt = points.device, points.dtype
    with _on_stream(dev) as stream:
        ws, nbytes = _workspace(lib.sqfa_class_moments_workspace_bytes, C, D, code)
        keep = torch.empty(C, dtype=dt, device=dev)
        shift = torch.empty(C, dtype=dt, device=dev)
        rho = torch.empty(C, dtype=torch.float64, device=dev)
        _lib.check(lib.sqfa_class_shrinkage(_ptr(points), N, D, _ptr(order), _ptr(class_start), C, code, _ptr(means),
                                            _ptr(keep), _ptr(shift), _ptr(rho), _ptr(ws), nbytes, stream),
                   "sqfa_class_shrinkage")
    return keep, shift, rho


def class_feature_moments_supported(points, filters):
    """Contiguous float32 / float64 (N,D) points on the GPU and (K,D) filters of the same dtype and device, K <= 64."""
    return bool(class_moments_supported(points) and points.is_contiguous() and filters.dim() == 2
                and filters.device == points.device and filters.dtype == points.dtype
                and filters.shape[1] == points.shape[1] and 1 <= filters.shape[0] <= POINT_MAX_FILTERS)


def point_backward_groups(N, D):
    """Row groups of sqfa_class_feature_moments_backward: groups x 64-column stripes of ~1024 workgroups (four per CU), at
    most 64 groups (the (groups, K, D) partial sums are read again by the sum over the groups) and no group below one
    chunk of 32 rows."""
    stripes = (D + 63) // 64
    return max(1, min(64, -(-1024 // stripes), -(-max(N, 1) // 32)))


def _feature_moments_entry(cp, suffix=""):
    """(shrinkage coefficients or (), entry name, workspace query) for a ClassPoints: one with shrinkage coefficients
    (estimator="oas") goes through the _shrunk entries, which take `keep` and `shift` (and the filters, backward) as well."""
    keep, shift = getattr(cp, "shrink_keep", None), getattr(cp, "shrink_shift", None)
    shrink = () if keep is None else (keep, shift)
    name = "sqfa_class_feature_moments" + ("_shrunk" if shrink else "")
    return shrink, name + suffix, getattr(_lib.load(), name + "_workspace_bytes")


def class_feature_moments(cp, F, second_moments, noise):
    """sqfa_class_feature_moments on the current stream for a statistics.ClassPoints `cp` and contiguous filters F (K,D):
    (zc (N,K) in grouped order, means_f (C,K), cov_f (C,K,K), second_f (C,K,K) or None).  A `cp` with shrinkage
    coefficients (estimator="oas") goes through sqfa_class_feature_moments_shrunk."""
    X = cp.points
    N, D = X.shape
    K, C = F.shape[0], cp.n_classes
    code = _dtype_code(X)
    dev, dt = X.device, X.dtype
    shrink, name, query = _feature_moments_entry(cp)
    with _on_stream(dev) as stream:
        ws, nbytes = _workspace(query, N, C, D, K, code)
        zc = torch.empty((N, K), dtype=dt, device=dev)
        means_f = torch.empty((C, K), dtype=dt, device=dev)
        cov_f = torch.empty((C, K, K), dtype=dt, device=dev)
        second_f = torch.empty((C, K, K), dtype=dt, device=dev) if second_moments else None
        status = getattr(_lib.load(), name)(_ptr(X), N, D, _ptr(cp.order), _ptr(cp.row_class), _ptr(cp.class_start), C,
                                            _ptr(cp.means), _ptr(F), K, code, float(noise), *map(_ptr, shrink), _ptr(zc),
                                            _ptr(means_f), _ptr(cov_f), _ptr(second_f), _ptr(ws), nbytes, stream)
    _lib.check(status, name)
    return zc, means_f, cov_f, second_f


def class_feature_moments_backward(cp, zc, G, g_means, F=None):
    """sqfa_class_feature_moments_backward on the current stream: the (n_groups, K, D) partial sums of dL/dF for
    G = dL/dcov_f (C,K,K) and g_means = dL/dmeans_f (C,K) or None.  A `cp` with shrinkage coefficients needs the contiguous
    filters F (K,D) of the forward call as well (sqfa_class_feature_moments_shrunk_backward)."""
    X = cp.points
    N, D = X.shape
    K, C = zc.shape[1], cp.n_classes
    code = _dtype_code(X)
    G = G.detach().contiguous()
    g_means = g_means.detach().contiguous() if g_means is not None else None
    groups = point_backward_groups(N, D)
    shrink, name, query = _feature_moments_entry(cp, "_backward")
    if shrink and F is None:
        raise ValueError("the backward of shrunk feature moments needs the filters")
    with _on_stream(X.device) as stream:
        ws, nbytes = _workspace(query, N, C, D, K, code)
        partial = torch.empty((groups, K, D), dtype=X.dtype, device=X.device)
        status = getattr(_lib.load(), name)(_ptr(X), N, D, _ptr(cp.order), _ptr(cp.row_class), _ptr(cp.class_start), C,
                                            _ptr(cp.means), *((_ptr(F),) if shrink else ()), _ptr(zc), _ptr(G), K,
                                            _ptr(g_means), *map(_ptr, shrink), K, code, groups, _ptr(partial), _ptr(ws),
                                            nbytes, stream)
    _lib.check(status, name)
    return partial


class ClassFeatureMoments(torch.autograd.Function):
    """(means_f (C,K), cov_f (C,K,K)[, second_f (C,K,K)]) of the projected points F x, per class, from a
    statistics.ClassPoints: F mu_c, cov(F x | c) (+ noise on the diagonal) and their second moment, equal to F mu_c,
    F cov_c F^T and F (cov_c + mu_c mu_c^T) F^T of the dense statistics without forming them (replaces class_statistics
    + transform_scatters of the reference, src/sqfa/statistics.py:8-124, src/sqfa/model.py:172-188).  The backward
    returns dL/dF only; it needs the centred features (N,K) and the points, read once more.  A ClassPoints with
    estimator="oas" gives the same moments of the shrunk covariances keep_c cov_c + shift_c I (the shrunk entries)."""

    @staticmethod
    def forward(ctx, filters, class_points, second_moments, noise):
        F = filters.detach().contiguous()
        zc, means_f, cov_f, second_f = class_feature_moments(class_points, F, second_moments, noise)
        shrunk = getattr(class_points, "shrink_keep", None) is not None
        ctx.save_for_backward(zc, means_f, *((F,) if shrunk else ()))   # shrunk: the backward adds H F
        ctx.class_points = class_points
        ctx.second = bool(second_moments)
        return (means_f, cov_f, second_f) if second_moments else (means_f, cov_f)

    @staticmethod
    def backward(ctx, g_means, g_cov, g_second=None):
        zc, means_f, *filters = ctx.saved_tensors
        G = g_cov
        if ctx.second:
            # second = cov + m m^T: its gradient goes to the covariance as it is and to the means through the product
            # (elementwise, not a batched GEMM: a first BLAS call inside a graph capture allocates its own workspace of
            # tens of MB in the graph's pool)
            G = G + g_second
            sym = g_second + g_second.transpose(1, 2)
            g_means = g_means + (sym * means_f.unsqueeze(1)).sum(dim=-1)
        partial = class_feature_moments_backward(ctx.class_points, zc, G, g_means, *filters)
        return partial.sum(dim=0), None, None, None


# ------------------------------------------------------------------------------------------
# projection of the class scatter matrices (the HBM-bound stage around the pair kernel)


_symmetry_check_warned = False
_symmetry_checked = TensorMemo()   # scatters -> verdict


def _is_symmetric_batch(scatters):
    """The streaming kernel forms T = Psi^T F^T, which equals the reference's Psi F^T only for
    symmetric Psi (covariance / second-moment matrices are; conjugate_matrix itself is general,
    src/sqfa/linalg.py:19-45).  Checked ONCE per tensor object and version (one pass over Psi in class chunks of
    at most ~256 MB -- the c4 statistics are 16.8 GB, whole-tensor temporaries would triple that -- and one host
    read), outside any graph capture; asymmetry at rounding level (a GEMM-built X^T X) passes.  The verdict is
    keyed on the tensor OBJECT (weak reference), not on its address: the caching allocator hands a freed address
    to the next tensor.  Any failure of the check itself (e.g. out of memory) selects the general torch expression."""
    hit = _symmetry_checked.get(scatters)
    if hit is not None:
        return hit
    if torch.cuda.is_current_stream_capturing():
        return False  # never seen outside a capture: take the general torch expression
    tol = 1e-5 if scatters.dtype == torch.float32 else 1e-12
    try:
        with torch.no_grad():
            per_class = scatters[0].numel() * scatters.element_size()
            step = max(1, (256 << 20) // max(per_class, 1))
            asym = scatters.new_zeros(())
            peak = scatters.new_zeros(())
            for c0 in range(0, scatters.shape[0], step):
                blk = scatters[c0:c0 + step]
                asym = torch.maximum(asym, (blk - blk.transpose(-2, -1)).abs().amax())
                peak = torch.maximum(peak, blk.abs().amax())
            ok = bool(asym <= tol * peak)
    except Exception as err:   # the check must never take the fit down: the torch expression handles every input
        ok = False
        global _symmetry_check_warned
        if not _symmetry_check_warned:
            _symmetry_check_warned = True
            import warnings
            warnings.warn(f"sqfa_amd: the symmetry check of the scatter matrices itself failed ({err!r}); this tensor keeps the "
                          "general torch projection (slower, same results)")
    return _symmetry_checked.put(ok, scatters)


def native_projection_supported(scatters, filters):
    """The streaming kernel handles SYMMETRIC float32/float64 (C,D,D) scatters on the GPU with
    D % 4 == 0, 16-byte aligned storage and up to 64 filters; anything else keeps the plain torch
    expression (conjugate_matrix)."""
    return (
        scatters.is_cuda and filters.is_cuda and scatters.dtype in (torch.float32, torch.float64)
        and filters.dtype == scatters.dtype
        and scatters.dim() == 3 and filters.dim() == 2 and scatters.shape[-1] % 4 == 0
        and filters.shape[0] <= 64 and filters.shape[0] <= filters.shape[1]
        and scatters.shape[-1] == scatters.shape[-2] == filters.shape[1] and not scatters.requires_grad
        and scatters.is_contiguous() and scatters.data_ptr() % 16 == 0
        and _is_symmetric_batch(scatters)
    )


# ---- block-triangular packed statistics (sqfa_pack_scatters / sqfa_project_scatters_packed) ------------------------------
# The symmetric (C,D,D) statistics are packed ONCE per prepared tensor (model._prepare_statistics) into their lower block
# triangle; every closure then streams 51-54 % of the bytes.  The packed copy lives beside the caller's tensor (which the
# caller owns and may free: statistics.pack_scatters hands the packed form out for that case).
# Measured (tools/time_projection_packed.py, profiles/r4_projection_packed.txt; full tensor -> packed, two boxes): c3 (C=1000,
# D=784, K=16) 0.43-0.45 -> 0.35-0.37 ms, K=8 0.43 -> 0.33-0.35, D=1024 0.63-0.67 -> 0.55-0.58, D=2048 / K=16 2.70 -> 2.29-2.40;
# it LOSES where the walk is short or the chip is not full: D=512 0.169 -> 0.186, C=256 0.121 -> 0.143, C=500 / D=3072 a tie;
# K=32 (c4) 3.02 -> 4.4-4.6 ms (two filter blocks: twice the exact-f32 MFMA work per byte, MFMA-bound); C=100 (c5) 0.58 -> 1.1-1.2 ms
# (one workgroup per class leaves 60 % of the CUs idle; splitting a class over several workgroups with a second pass over
# their partial results was built and measured at 1.08 ms: the per-row-block barrier of the walk dominates there; removed).
PACKED_PROJECTION = True
PACKED_MIN_CLASSES = 512      # one workgroup per class, two resident per CU
PACKED_MIN_DIM = 768
PACKED_MAX_FILTERS = 16       # one 16-filter block: beyond it the packed kernel is MFMA-bound and loses to the full-tensor stream
_packed = TensorMemo()        # scatters -> packed copy


def packed_supported(scatters):
    return (PACKED_PROJECTION and scatters.is_cuda and scatters.dtype == torch.float32 and scatters.dim() == 3
            and scatters.shape[-1] == scatters.shape[-2] and scatters.shape[-1] % 16 == 0 and PACKED_MIN_DIM <= scatters.shape[-1] <= 4096
            and scatters.shape[0] >= PACKED_MIN_CLASSES and scatters.is_contiguous() and scatters.data_ptr() % 16 == 0
            and not scatters.requires_grad)


def pack_scatters(scatters):
    """(C,D,D) symmetric float32 scatters -> (C, packed_elems) block-triangular packed form (sqfa_pack_scatters)."""
    lib = _lib.load()
    C, D = scatters.shape[0], scatters.shape[-1]
    n = lib.sqfa_packed_scatter_elems(D)
    if n == 0:
        raise ValueError(f"n_dim = {D} has no packed form (needs D % 16 == 0)")
    with _on_stream(scatters.device) as stream:
        out = torch.empty((C, n), dtype=scatters.dtype, device=scatters.device)
        _lib.check(lib.sqfa_pack_scatters(_ptr(scatters), C, D, _dtype_code(scatters), _ptr(out), stream), "sqfa_pack_scatters")
    return out


def prepare_packed(scatters, n_filters):
    """Pack `scatters` once (outside any graph capture) if the packed projection applies to it and to this filter count;
    later projections of the same tensor object / version find the packed copy through packed_for."""
    if (not torch.is_tensor(scatters) or n_filters > PACKED_MAX_FILTERS or not packed_supported(scatters)
            or torch.cuda.is_current_stream_capturing()):
        return None
    hit = packed_for(scatters)
    if hit is not None:
        return hit
    if not _is_symmetric_batch(scatters):
        return None
    return _packed.put(pack_scatters(scatters), scatters)


def packed_for(scatters, n_filters=1):
    return _packed.get(scatters) if (PACKED_PROJECTION and n_filters <= PACKED_MAX_FILTERS) else None


def _launch_projection(lib, F, Psi, T, K, D, C, code, stream):
    """T = Psi F^T: from the packed copy when one was prepared for this tensor, else from the full tensor."""
    packed = packed_for(Psi, K)
    if packed is not None:
        _lib.check(lib.sqfa_project_scatters_packed(_ptr(F), K, D, _ptr(packed), C, code, _ptr(T), stream),
                   "sqfa_project_scatters_packed")
    else:
        _lib.check(lib.sqfa_project_scatters(_ptr(F), K, D, _ptr(Psi), C, code, _ptr(T), stream), "sqfa_project_scatters")


def backward_groups(C, D, cap=64):
    """Class groups of sqfa_feature_scatters_backward: the kernel wants ~3000 waves in flight (one per 16-column
    block and group; it is latency-bound), while the (groups, K, D) partial sums are re-read by the reduction that
    follows, whose time grows with the group count.  Measured (tools/time_feature_backward.py, backward + reduction):
    c3 (D=784) 64 groups 34 us (16: 43), c4 (D=2048) 32: 128 us (64: 139, 16: 151), c5 (D=3072, C=100) 16: 28 us
    (64: 56)."""
    blocks = (D + 15) // 16
    want = max(1, -(-3072 // blocks))
    groups = 8
    while groups < want:
        groups *= 2
    return max(1, min(groups, cap, C))


class ProjectScatters(torch.autograd.Function):
    """S_c = F Psi_c F^T for symmetric Psi_c, reading Psi (C,D,D) from HBM once.

    forward : T = Psi F^T through sqfa_project_scatters (streaming MFMA kernel), S = F T through
              sqfa_feature_scatters
    backward: dL/dF = sum_c (G_c + G_c^T) T_c^T through sqfa_feature_scatters_backward -- needs
              T (C,D,K) only, not Psi.
    Replaces conjugate_matrix (reference src/sqfa/linalg.py:19-45) in transform_scatters
    (src/sqfa/model.py:172-188), whose autograd reads Psi a second time in the backward."""

    # class groups of the backward kernel (one wave per 16-column block and group): see backward_groups
    BACKWARD_GROUPS = 64
    # S = F T and dL/dF go through the HIP kernels from this many classes on (measured, closure at
    # C=1000, D=784, K=16: 1.61 -> 1.56 ms); below, torch's batched GEMMs are as fast (both are
    # launch/latency-bound there).  A huge value selects the torch expressions everywhere.
    NATIVE_PRODUCTS_MIN_CLASSES = 256

    @staticmethod
    def forward(ctx, filters, scatters):
        lib = _lib.load()
        F = filters.detach().contiguous()
        Psi = scatters.detach().contiguous()
        K, D = F.shape
        C = Psi.shape[0]
        code = _dtype_code(Psi)
        with _on_stream(Psi.device) as stream:
            T = torch.empty((C, D, K), dtype=Psi.dtype, device=Psi.device)
            S = torch.empty((C, K, K), dtype=Psi.dtype, device=Psi.device)
            _launch_projection(lib, F, scatters if scatters.is_contiguous() else Psi, T, K, D, C, code, stream)
            if C >= ProjectScatters.NATIVE_PRODUCTS_MIN_CLASSES:
                _lib.check(lib.sqfa_feature_scatters(_ptr(F), K, D, _ptr(T), C, code, _ptr(S), stream),
                           "sqfa_feature_scatters")
            else:
                S = torch.matmul(F.unsqueeze(0), T)
        ctx.save_for_backward(T)
        return S

    @staticmethod
    def backward(ctx, gS):
        (T,) = ctx.saved_tensors
        C, D, K = T.shape
        if C >= ProjectScatters.NATIVE_PRODUCTS_MIN_CLASSES:
            lib = _lib.load()
            G = gS.contiguous()
            groups = backward_groups(C, D, ProjectScatters.BACKWARD_GROUPS)
            with _on_stream(T.device) as stream:
                partial = torch.empty((groups, K, D), dtype=T.dtype, device=T.device)
                _lib.check(lib.sqfa_feature_scatters_backward(_ptr(G), _ptr(T), C, D, K, _dtype_code(T), groups,
                                                              _ptr(partial), stream), "sqfa_feature_scatters_backward")
            return partial.sum(dim=0), None
        # few classes (launch-bound either way) or a filter count that is not a multiple of 4:
        # per-class (K,K)@(K,D) products, then the sum over classes.  (One flat GEMM (K, C*K)@(C*K, D) is the same arithmetic but hipBLASLt is
        # erratic for that skinny shape: 8 ms at C=1000, K=16 in isolation.)
        sym = gS + gS.transpose(1, 2)
        return torch.bmm(sym, T.transpose(1, 2)).sum(dim=0), None


def project_scatters(scatters, filters):
    """(C,D,D) x (K,D) -> (C,K,K); native streaming kernel when supported, torch otherwise."""
    if native_projection_supported(scatters, filters):
        return ProjectScatters.apply(filters, scatters)
    return None


# ------------------------------------------------------------------------------------------
# the orthogonal filter constraint (torch's _Orthogonal, Householder map with a `base` matrix)

ORTHOGONAL_MAX_FILTERS = 64


def orthogonal_supported(X, base):
    """The native map handles a contiguous float32/float64 (K,D) raw parameter on the GPU with K <= 64 and K < D (the
    shapes for which torch picks the Householder map) and a contiguous (D,D) base of the same dtype and device; anything
    else keeps torch's own forward."""
    if X is None or base is None:
        return False
    return bool(X.is_cuda and base.is_cuda and X.dtype in (torch.float32, torch.float64) and base.dtype == X.dtype
                and X.dim() == 2 and base.dim() == 2 and 1 <= X.shape[0] <= ORTHOGONAL_MAX_FILTERS
                and X.shape[0] < X.shape[1] and tuple(base.shape) == (X.shape[1], X.shape[1])
                and X.device == base.device and X.is_contiguous() and base.is_contiguous())


def _orthogonal_call(forward, X, base, gF=None):
    """sqfa_orthogonal_forward / sqfa_orthogonal_backward on the current stream (workspace from the torch allocator, no
    host read-back: safe inside a graph capture).  Returns F or dL/dX, (K,D)."""
    lib = _lib.load()
    K, D = X.shape
    code = _dtype_code(X)
    with _on_stream(X.device) as stream:
        ws, nbytes = _workspace(lib.sqfa_orthogonal_workspace_bytes, K, D, code)
        out = torch.empty_like(X)
        if forward:
            _lib.check(lib.sqfa_orthogonal_forward(_ptr(X), _ptr(base), K, D, code, _ptr(out), _ptr(ws), nbytes, stream),
                       "sqfa_orthogonal_forward")
        else:
            _lib.check(lib.sqfa_orthogonal_backward(_ptr(X), _ptr(base), _ptr(gF), K, D, code, _ptr(out), _ptr(ws), nbytes,
                                                    stream), "sqfa_orthogonal_backward")
    return out


class OrthogonalFilters(torch.autograd.Function):
    """F = (base @ householder_product(tril(X^T, -1), tau) * sign)^T, torch's _Orthogonal.forward for a wide (K,D) raw
    parameter (reference: src/sqfa/model.py:416-431), through sqfa_orthogonal_forward / sqfa_orthogonal_backward
    (compact WY form, 4 launches each way).  The backward recomputes from X: nothing but X and base is saved."""

    @staticmethod
    def forward(ctx, X, base):
        Xc, Bc = X.detach().contiguous(), base.detach().contiguous()
        ctx.save_for_backward(Xc, Bc)
        return _orthogonal_call(True, Xc, Bc)

    @staticmethod
    def backward(ctx, gF):
        Xc, Bc = ctx.saved_tensors
        return _orthogonal_call(False, Xc, Bc, gF.detach().contiguous()), None


# ------------------------------------------------------------------------------------------
# the whole closure as one autograd node


def closure_stage_project(raw, scatters, means, noise, sphere, out_S=None):
    """First half of a closure evaluation, no autograd: parametrization -> T = Psi F^T -> [m = mu F^T] -> S | E
    (feature scatters + noise, or their Calvo-Oller embedding), written into `out_S` when given (a slice of
    the all-gather buffer of a class-sharded evaluation).  Returns what the backward stage needs.
    `sphere`: True (Sphere), False (Identity), or the (D,D) `base` tensor of an orthogonal parametrization."""
    lib = _lib.load()
    X = raw.detach().contiguous()
    Psi = scatters.detach()
    K, D = X.shape
    C = Psi.shape[0]
    code = _dtype_code(Psi)
    dev, dt = Psi.device, Psi.dtype
    with _on_stream(dev) as stream:
        base = sphere.detach() if torch.is_tensor(sphere) else None
        sphere = base is None and bool(sphere)
        if base is not None:
            F, norms = _orthogonal_call(True, X, base), None
        elif sphere:
            F = torch.empty_like(X)
            norms = torch.empty(K, dtype=dt, device=dev)
            _lib.check(lib.sqfa_sphere_forward(_ptr(X), K, D, code, _ptr(F), _ptr(norms), stream), "sqfa_sphere_forward")
        else:
            F, norms = X, None
        T = torch.empty((C, D, K), dtype=dt, device=dev)
        _launch_projection(lib, F, scatters, T, K, D, C, code, stream)   # keyed on the caller's tensor object (packed copy)
        msize = K + 1 if means is not None else K
        m = torch.matmul(means.detach(), F.t()).contiguous() if means is not None else None   # (C,K) projected means
        S = out_S if out_S is not None else torch.empty((C, msize, msize), dtype=dt, device=dev)
        if tuple(S.shape) != (C, msize, msize) or not S.is_contiguous():
            raise ValueError("out_S must be a contiguous (C, m, m) tensor")
        _lib.check(lib.sqfa_feature_scatters_ex(_ptr(F), K, D, _ptr(T), C, code, float(noise), _ptr(m), _ptr(S), stream),
                   "sqfa_feature_scatters_ex")
    return {"X": X, "norms": norms, "T": T, "m": m, "means": means.detach() if means is not None else None,
            "S": S, "S_shape": tuple(S.shape), "sphere": sphere, "base": base}


def closure_stage_pairs(S, scale, sqrt_mode, weight, shard, fused=None, metric="airm", pair_weights=None):
    """Second half: K0 / K1 / K2 on the (C,m,m) batch.  `fused` (S.numel() + 3 elements), when given, receives
    [loss, nan, inf, dL/dS...] in place (the all-reduce buffer of a sharded evaluation).  `pair_weights`: the symmetric
    (C,C) per-pair weights of normalized_pair_weights in place of `weight`."""
    extra = {"metric": metric} if metric != "airm" else {}
    if fused is not None:
        extra.update(fused_outputs(fused, S.shape))
    out = _pair_backend(S, None, scale=scale, eps=EPSILON, sqrt_mode=sqrt_mode, weights=_self_pair_weights(pair_weights),
                        uniform_weight=weight, shard=shard, want_loss=True, want_grad=True,
                        want_dist=False, want_eig=False, **extra)
    if fused is not None:
        fused[1:3].copy_(out["nonfinite"])   # int32 -> real in the copy itself
    return out["loss"], out["nonfinite"], out["gradA"]


def closure_stage_backward(st, gS, gloss):
    """Kernels from dL/dS (or dL/dE) back to the raw filter parameter: backward product, [means path],
    class reduction + sphere backward (+ multiplication by `gloss`, a device scalar or None); for an orthogonal
    parametrization the class reduction (sphere backward without norms) and then sqfa_orthogonal_backward."""
    lib = _lib.load()
    X, norms, T, m, means = st["X"], st["norms"], st["T"], st["m"], st["means"]
    C, D, K = T.shape
    code = _dtype_code(T)
    dev, dt = T.device, T.dtype
    groups = backward_groups(C, D, FusedClosure.BACKWARD_GROUPS)
    gS = gS.contiguous()
    ldg = gS.shape[-1]
    with _on_stream(dev) as stream:
        partial = torch.empty((groups, K, D), dtype=dt, device=dev)
        # gS is the pair kernels' dL/dS (or dL/dE): written symmetric by sqfa_airm_pairwise, sums of shards included
        _lib.check(lib.sqfa_feature_scatters_backward_ex(_ptr(gS), ldg, _ptr(T), C, D, K, code, groups, 1, _ptr(partial), stream),
                   "sqfa_feature_scatters_backward_ex")
        extra = None
        if m is not None:
            gm = torch.empty((C, K), dtype=dt, device=dev)
            _lib.check(lib.sqfa_embed_backward_means(_ptr(gS), _ptr(m), C, K, code, _ptr(gm), stream), "sqfa_embed_backward_means")
            extra = torch.matmul(gm.t(), means).contiguous()          # (K,D): m = mu F^T  =>  dL/dF += g_m^T mu
        grad = torch.empty_like(X)
        gl = gloss.detach().to(dt).contiguous() if gloss is not None else None
        _lib.check(lib.sqfa_sphere_backward(_ptr(X), _ptr(norms if st["sphere"] else None), K, D, code, _ptr(partial), groups,
                                            _ptr(extra), _ptr(gl), _ptr(grad), stream), "sqfa_sphere_backward")
        if st.get("base") is not None:
            grad = _orthogonal_call(False, X, st["base"], grad)
    return grad


class FusedClosure(torch.autograd.Function):
    """loss(raw filters) of one closure evaluation as ONE autograd node, 8 launches for
    SecondMomentsSQFA and 11 for SQFA instead of ~40:

        forward   sphere (or nothing, or the orthogonal map: 4 launches)  ->  T = Psi F^T (streaming)  ->  [m = mu F^T]  ->
                  S = F T + noise I  |  E = [[S + m m^T, m], [m^T, 1]]  ->  K0 / K1 / K2 (loss, dL/dS, flags)
        backward  (G + G^T) T^T partial sums  ->  [g_m, g_m^T mu]  ->  class reduction + sphere backward + gloss
                  [-> orthogonal backward: 4 launches]

    Same arithmetic as the chain Sphere -> ProjectScatters -> (+noise) -> embed_gaussian -> PairwiseLoss
    it replaces (reference: src/sqfa/constraints.py:37, src/sqfa/model.py:172-188, 508-546,
    src/sqfa/distances.py:141-174, src/sqfa/_optim.py:90-96); the summation order of the row norms
    and of the class reduction differs (fixed, reproducible)."""

    BACKWARD_GROUPS = 64

    @staticmethod
    def forward(ctx, raw, scatters, means, noise, scale, sqrt_mode, weight, shard, reducer, sphere, metric="airm",
                pair_weights=None):
        owner = fused_reduce_owner(reducer, shard)
        fused = None
        if owner is not None:
            m = raw.shape[0] + (1 if means is not None else 0)
            fused = fused_buffer((scatters.shape[0], m, m), scatters.dtype, scatters.device)
        st = closure_stage_project(raw, scatters, means, noise, sphere)
        loss, nonfinite, gS = closure_stage_pairs(st.pop("S"), scale, sqrt_mode, weight, shard, fused, metric, pair_weights)
        if fused is not None:
            loss, nonfinite, gS = owner.reduce_fused(fused, nonfinite, st["S_shape"])
        elif reducer is not None:
            loss, nonfinite, gS = reducer(loss, nonfinite, gS)
        ctx.st = st
        ctx.gS = gS
        ctx.mark_non_differentiable(nonfinite)
        return loss, nonfinite

    @staticmethod
    def backward(ctx, gloss, _gflag):
        grad = closure_stage_backward(ctx.st, ctx.gS, gloss)
        return grad, None, None, None, None, None, None, None, None, None, None, None
