"""Gaussian class scores: quadratic discriminant analysis (QDA) in feature space, the step the reference's tutorial judges
every fit by (QDA accuracy on held-out samples), without leaving the GPU.

For features z (K), class means mu_c, class covariances Sigma_c = L_c L_c^T and priors pi_c

    score[n, c] = -1/2 |L_c^-1 (z_n - mu_c)|^2 - sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c  =  log p(z_n, c)

evaluated in this whitened-difference form (the expanded quadratic z^T P z - 2 b^T z + const cancels in float32).

    gaussian_class_scores(Z, means, covariances, priors=None)      (N, C) scores
    GaussianClassifier(means, covariances, priors=None)            scores / predict / log_evidence / predict_log_proba /
                                                                   predict_proba / accuracy of features Z (N, K)
    FeatureClassifier.from_model(model, X, y | data_statistics)    the same of raw points X (N, D), through the model's filters
    gaussian_log_loss(Z, y, means, covariances, priors=None)       -1/N sum_n log p(y_n | z_n), differentiable in Z, means
                                                                   and covariances
    feature_log_loss(model, X, y, ...) / fit_log_loss(model, X, y, ...)   that loss of a model's current filters, and L-BFGS on it

float32 / float64 GPU tensors with K <= 64 run on the native kernels (gauss_scores_kernel.hip): a factor pass once per
classifier (sqfa_gauss_class_factors) and one pass per batch of samples (sqfa_gauss_scores) that carries the argmax and the
log-sum-exp of every sample across the classes in registers, so that ``predict``, ``log_evidence`` and ``accuracy`` never
form anything of size (N, C).  Native results carry no graph.  CPU tensors, other dtypes, K > 64,
``NATIVE_CLASS_SCORES = False`` and any input that requires grad while grad is enabled evaluate the same formula as a torch
expression, chunked over the classes so that its (classes, N, K) temporary stays under ``FALLBACK_BYTES``; that expression is
differentiable.

The log-loss (``label_log_proba``, ``log_loss``, ``gaussian_log_loss``) runs natively under the same conditions
(gauss_log_loss_kernel.hip; switch ``NATIVE_LOG_LOSS``), also where an input asks for a gradient: sqfa_gauss_log_loss and
sqfa_gauss_log_loss_backward form nothing of size (N, C) or (C, N, K), and the forward costs one read from the device (the
bad-class count and the three flags together), the backward none.  Elsewhere the torch expression applies, chunked over the
classes for the forward; with a gradient wanted it holds what autograd holds: the (classes, N, K) whitened differences of
every chunk.

Nested classifiers (``nested_predict``, ``nested_log_evidence``, ``nested_accuracy``, ``nested_label_log_proba``,
``nested_log_loss``): column k - 1 of every result belongs to the classifier that sees only the first k features, so one
call gives accuracy and log-loss against the number of filters kept.  The leading k x k block of L_c is the Cholesky factor
of the leading block of Sigma_c, and the first k entries of L_c^-1 (z - mu_c) depend on the first k features only: score_k
is a prefix sum over the squares the full classifier sums anyway, plus a (C, K) table of offsets.  Native under the
conditions of the class scores (gauss_nested_kernel.hip; switch ``NATIVE_NESTED``) at N C K^2 work, with nothing of size
(N, C) or (N, C, K) formed; elsewhere a chunked torch expression under ``no_grad``.  Results carry no graph.

Top-k and the label's rank (``predict_topk``, ``label_rank``, ``topk_accuracy``): the k best classes of every sample and
the number of classes placed before the labelled one, under one total order: higher score first, equal scores: lower class
index first (a class of prior 0 scores -inf and comes after every finite one).  Native under the conditions of the class
scores, and k <= 8 for ``predict_topk`` (gauss_topk_kernel.hip; switch ``NATIVE_TOPK``): the scorer's pass with a short
sorted list, or a counter, per lane in place of (max, index), on scores with the bits of ``scores(Z)``, with nothing of
size (N, C) formed.  One shape condition, from the measurement in the README: with K > 48 and fewer than 512 classes
``label_rank`` counts on the native scores, a chunk of samples at a time (the same ranks).  Elsewhere ``_torch_scores`` and a
stable descending sort, or the count, under ``no_grad``, chunked over the samples.  Results carry no graph.
"""
import math
import time

import torch
from torch.autograd.function import once_differentiable

from . import _lib, _native
from .statistics import ClassPoints, class_statistics

__all__ = ["gaussian_class_scores", "GaussianClassifier", "FeatureClassifier"]   # the star-import surface stays as it was
# also public, by their module path: gaussian_log_loss, feature_log_loss, fit_log_loss

NATIVE_CLASS_SCORES = True
NATIVE_LOG_LOSS = True
NATIVE_NESTED = True
NATIVE_TOPK = True
NATIVE_TOPK_MAX = 8      # entries of the native top-k list at most
# label_rank by the rank kernels unless K > RANK_WIDE_FEATURES and C < RANK_WIDE_MIN_CLASSES: there the native scores and the
# count on them are faster (the label pre-pass stages a 16 KB class image per sample at K = 64; README, the top-k table)
RANK_WIDE_FEATURES = 48
RANK_WIDE_MIN_CLASSES = 512
NATIVE_MAX_FEATURES = 64
# the torch expression's (classes, N, K) temporaries (the differences and the solve's result) stay below this many bytes
FALLBACK_BYTES = 1 << 28
_NATIVE_DTYPES = (torch.float32, torch.float64)


def _log_priors(priors, n_classes, device):
    """(C,) float64 log priors: None / "uniform" -> -log C; a (C,) tensor-like of non-negative weights with a positive sum,
    normalised (a zero weight gives -inf: a class that never wins)."""
    if priors is None or (isinstance(priors, str) and priors == "uniform"):
        return torch.full((n_classes,), -math.log(n_classes), dtype=torch.float64, device=device)
    if isinstance(priors, str):
        raise ValueError(f"priors must be None, 'uniform' or (n_classes,) non-negative weights, got {priors!r}")
    try:
        # a list of Python floats in float64, not in torch's default dtype (float32 rounds the weights, and 1e-300 to zero)
        w = priors.detach() if torch.is_tensor(priors) else torch.as_tensor(priors, dtype=torch.float64)
        w = w.to(device=device, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as err:
        raise ValueError("priors must be None, 'uniform' or (n_classes,) non-negative weights") from err
    if w.shape != (n_classes,):
        raise ValueError(f"priors must have shape ({n_classes},), got {tuple(w.shape)}")
    lo, total = torch.stack((w.min(), w.sum())).tolist()
    if not (lo >= 0.0 and 0.0 < total < math.inf):   # also refuses NaN
        raise ValueError("priors must be non-negative and finite with a positive sum")
    return torch.log(w / total)


def _grad_wanted(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _native_applies(*tensors):
    """float32 / float64 tensors on one GPU, none of which asks for a gradient, with the switch on."""
    first = tensors[0]
    return bool(NATIVE_CLASS_SCORES and first.is_cuda and first.dtype in _NATIVE_DTYPES
                and all(t is None or (t.device == first.device and t.dtype == first.dtype) for t in tensors)
                and not _grad_wanted(*tensors))


def _native_class_factors(mu, cov, log_priors):
    """sqfa_gauss_class_factors on contiguous tensors without a graph: (W (C,K,K), offset (C,) float64, the number of bad
    classes as a (1,) int32 device tensor)."""
    lib = _lib.load()
    C, K = cov.shape[0], cov.shape[-1]
    with _native._on_stream(cov.device) as stream:
        W = torch.empty_like(cov)
        offset = torch.empty(C, dtype=torch.float64, device=cov.device)
        bad = torch.empty(1, dtype=torch.int32, device=cov.device)
        lp = log_priors.contiguous()
        _lib.check(lib.sqfa_gauss_class_factors(_native._ptr(mu), _native._ptr(cov), _native._ptr(lp), C, K,
                                                _native._dtype_code(cov), _native._ptr(W), _native._ptr(offset),
                                                _native._ptr(bad), stream), "sqfa_gauss_class_factors")
    return W, offset, bad


def _native_log_loss(Z, y, mu, W, offset, want_ll=False):
    """One sqfa_gauss_log_loss call: (loss (1,), ll (N,) | None, logsumexp (N,), flags (3,) int32 on the device: samples
    with a NaN in their score row, labels outside [0, C), labels on a class of prior 0)."""
    lib = _lib.load()
    N, K, C = Z.shape[0], Z.shape[1], W.shape[0]
    code = _native._dtype_code(Z)
    with _native._on_stream(Z.device) as stream:
        ws, nbytes = _native._workspace(lib.sqfa_gauss_log_loss_workspace_bytes, N, C, K, code)
        loss = torch.empty(1, dtype=Z.dtype, device=Z.device)
        ll = torch.empty(N, dtype=Z.dtype, device=Z.device) if want_ll else None
        lse = torch.empty(N, dtype=Z.dtype, device=Z.device)
        flags = torch.empty(3, dtype=torch.int32, device=Z.device)
        _lib.check(lib.sqfa_gauss_log_loss(_native._ptr(Z), _native._ptr(y), N, _native._ptr(mu), _native._ptr(W),
                                           _native._ptr(offset), C, K, code, _native._ptr(loss), _native._ptr(ll),
                                           _native._ptr(lse), _native._ptr(flags), _native._ptr(ws), nbytes, stream),
                   "sqfa_gauss_log_loss")
    return loss, ll, lse, flags


def _labels(y, n_samples, device):
    """(N,) int64 labels on `device`; ValueError for another shape or a dtype that is not an integer."""
    y = torch.as_tensor(y)
    if y.is_floating_point() or y.is_complex() or y.dtype == torch.bool or y.shape != (n_samples,):
        raise ValueError(f"labels must be integers of shape ({n_samples},), got {y.dtype} of shape {tuple(y.shape)}")
    return y.detach().to(device=device, dtype=torch.int64).contiguous()


def _class_inputs(means, covariances):
    """(means (C, K) in the covariances' dtype and device | None, covariances (C, K, K)), or ValueError."""
    cov = torch.as_tensor(covariances)
    if cov.dim() != 3 or cov.shape[-1] != cov.shape[-2] or not cov.is_floating_point() or 0 in cov.shape:
        raise ValueError("covariances must be a floating-point tensor of shape (n_classes, n_features, n_features)")
    C, K = cov.shape[0], cov.shape[-1]
    mu = None
    if means is not None:
        mu = torch.as_tensor(means).to(device=cov.device, dtype=cov.dtype)
        if mu.shape != (C, K):
            raise ValueError(f"means must have shape ({C}, {K}), got {tuple(mu.shape)}")
    return mu, cov


def _samples(Z, like):
    """(N >= 1, K) samples in the dtype and on the device of the covariances `like` (C, K, K), or ValueError."""
    Z = torch.as_tensor(Z)
    if Z.dim() != 2 or Z.shape[1] != like.shape[-1] or Z.shape[0] < 1:
        raise ValueError(f"samples must have shape (n_samples >= 1, {like.shape[-1]}), got {tuple(Z.shape)}")
    return Z.to(device=like.device, dtype=like.dtype)


def _refuse_bad_classes(bad, n_classes):
    if bad:
        raise ValueError(f"{bad} of {n_classes} classes are not symmetric positive definite or not finite")


def _refuse_labelled(n_nan, n_outside, n_prior0, n_classes):
    """The refusals of the log-loss, from the three counts of sqfa_gauss_log_loss's flags."""
    if n_outside:
        raise ValueError(f"{n_outside} labels are outside [0, {n_classes})")
    if n_prior0:
        raise ValueError(f"{n_prior0} labels belong to a class with prior 0")
    GaussianClassifier._refuse(n_nan)


class GaussianClassifier:
    """Quadratic classifier of features from the class Gaussians N(mu_c, Sigma_c) and priors pi_c.

    means (C, K) or None (zero means), covariances (C, K, K), priors None / "uniform" / (C,) non-negative weights
    (normalised).  Construction factors every class once and raises ValueError, naming the number of bad classes, when a
    class is not symmetric positive definite or not finite.  Attributes: ``n_classes``, ``n_features``, ``log_priors``
    ((C,) float64).  Samples with a non-finite score row raise ValueError with their count.
    """

    def __init__(self, means, covariances, priors=None):
        mu, cov = _class_inputs(means, covariances)
        C, K = cov.shape[0], cov.shape[-1]
        self.n_classes, self.n_features = C, K
        self.means, self.covariances = mu, cov
        self.log_priors = _log_priors(priors, C, cov.device)
        self._factors = None   # native: (W (C,K,K), offset (C,) float64)
        self._torch = None     # the torch expression's (W = L^-1 (C,K,K), offset (C,) in the dtype)
        if K <= NATIVE_MAX_FEATURES and _native_applies(cov, mu):
            bad = self._native_factors()
        else:
            bad = self._torch_factors()
        _refuse_bad_classes(bad, C)

    @property
    def dtype(self):
        return self.covariances.dtype

    @property
    def device(self):
        return self.covariances.device

    # ------------------------------------------------------------------ factors
    def _native_factors(self):
        cov = self.covariances.detach().contiguous()
        mu = self.means.detach().contiguous() if self.means is not None else None
        W, offset, bad = _native_class_factors(mu, cov, self.log_priors)
        self._means_native = mu
        self._factors = (W, offset)
        return int(bad.item())

    def _torch_factors(self):
        """Inverse Cholesky factors and offsets as torch tensors (differentiable); the number of bad classes."""
        cov, mu = self.covariances, self.means
        L, info = torch.linalg.cholesky_ex(cov)
        finite = torch.isfinite(cov).flatten(1).all(1)
        if mu is not None:
            finite = finite & torch.isfinite(mu).all(1)
        bad = int(((info != 0) | ~finite).sum().item())
        logdiag = torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)
        offset = -logdiag - 0.5 * self.n_features * math.log(2.0 * math.pi) + self.log_priors.to(cov.dtype)
        # W_c = L_c^-1 once, as the native factor pass: the triangular solve then has K right-hand sides per class, not N
        # (hipBLAS's batched trsm cannot allocate its workspace for tens of thousands of them)
        eye = torch.eye(self.n_features, dtype=cov.dtype, device=cov.device).expand_as(L)
        self._torch = (torch.linalg.solve_triangular(L, eye, upper=False), offset)
        return bad

    # ------------------------------------------------------------------ evaluation
    def _use_native(self, Z):
        return self._factors is not None and _native_applies(Z)

    def _native_call(self, Z, scores=False, argmax=False, logsumexp=False):
        """One sqfa_gauss_scores call: (scores (N,C) | None, argmax (N,) int64 | None, logsumexp (N,) | None, the count of
        samples with a NaN in their row as a (1,) int32 device tensor)."""
        lib = _lib.load()
        Z = Z.detach().contiguous()
        W, offset = self._factors
        N, K, C = Z.shape[0], self.n_features, self.n_classes
        code = _native._dtype_code(Z)
        with _native._on_stream(Z.device) as stream:
            ws, nbytes = _native._workspace(lib.sqfa_gauss_scores_workspace_bytes, N, C, K, code)
            out_s = torch.empty((N, C), dtype=Z.dtype, device=Z.device) if scores else None
            out_a = torch.empty(N, dtype=torch.int64, device=Z.device) if argmax else None
            out_l = torch.empty(N, dtype=Z.dtype, device=Z.device) if logsumexp else None
            bad = torch.empty(1, dtype=torch.int32, device=Z.device)
            _lib.check(lib.sqfa_gauss_scores(_native._ptr(Z), N, _native._ptr(self._means_native), _native._ptr(W),
                                             _native._ptr(offset), C, K, code, _native._ptr(out_s), _native._ptr(out_a),
                                             None, _native._ptr(out_l), _native._ptr(bad), _native._ptr(ws), nbytes, stream),
                       "sqfa_gauss_scores")
        return out_s, out_a, out_l, bad

    def _torch_scores(self, Z):
        """The definition as a torch expression, a chunk of classes at a time."""
        if self._torch is None:
            self._torch_factors()
        W, offset = self._torch
        N, K, C = Z.shape[0], self.n_features, self.n_classes
        per_class = 3 * N * K * Z.element_size()
        step = max(1, min(C, FALLBACK_BYTES // max(1, per_class)))
        out = []
        for c0 in range(0, C, step):
            Wc = W[c0:c0 + step]
            if self.means is None:
                y = Wc @ Z.T                                                             # (c, K, N)
            else:
                y = Wc @ (Z[None] - self.means[c0:c0 + step, None]).transpose(-1, -2)    # the whitened differences
            out.append(-0.5 * (y * y).sum(1) + offset[c0:c0 + step, None])
        return (out[0] if len(out) == 1 else torch.cat(out)).T

    @staticmethod
    def _refuse(count):
        if count:
            raise ValueError(f"{count} samples have non-finite scores (NaN features, or features at infinity)")

    def _evaluate(self, Z, scores=False, argmax=False, logsumexp=False):
        """(scores, argmax, logsumexp, count of NaN rows as a device tensor) on whichever path applies."""
        Z = _samples(Z, self.covariances)
        if self._use_native(Z):
            return self._native_call(Z, scores, argmax, logsumexp)
        S = self._torch_scores(Z)
        nan = torch.isnan(S).any(1)
        return (S if scores else None, torch.where(nan, -1, S.argmax(1)) if argmax else None,
                torch.logsumexp(S, 1) if logsumexp else None, nan.sum().reshape(1))

    def scores(self, Z):
        """(N, C) joint log densities log p(z_n, c)."""
        S, _, _, bad = self._evaluate(Z, scores=True)
        self._refuse(int(bad.item()))
        return S

    def predict(self, Z):
        """(N,) int64: the class of the largest score, ties to the lowest index."""
        _, A, _, bad = self._evaluate(Z, argmax=True)
        self._refuse(int(bad.item()))
        return A

    def log_evidence(self, Z):
        """(N,) log p(z_n) = logsumexp_c score[n, c]."""
        _, _, E, bad = self._evaluate(Z, logsumexp=True)
        self._refuse(int(bad.item()))
        return E

    def predict_log_proba(self, Z):
        """(N, C) log posteriors: scores - log evidence."""
        S, _, E, bad = self._evaluate(Z, scores=True, logsumexp=True)
        self._refuse(int(bad.item()))
        return S - E[:, None]

    def predict_proba(self, Z):
        return torch.exp(self.predict_log_proba(Z))

    def accuracy(self, Z, y):
        """The share of samples whose predicted class is y, a Python float (one read from the device)."""
        _, A, _, bad = self._evaluate(Z, argmax=True)
        y = torch.as_tensor(y).to(A.device).long()
        if y.shape != A.shape:
            raise ValueError(f"labels must have shape ({A.shape[0]},), got {tuple(y.shape)}")
        correct, n_bad = torch.stack(((A == y).sum(), bad.reshape(()).to(torch.int64))).tolist()
        self._refuse(n_bad)
        return correct / A.shape[0]

    # ------------------------------------------------------------------ log-loss
    def _torch_label_log_proba(self, Z, y):
        """ll_n = score[n, y_n] - logsumexp_c score[n, c] as a torch expression (differentiable), with the refusals of the
        native pass from one read."""
        S = self._torch_scores(Z)
        C = self.n_classes
        inside = (y >= 0) & (y < C)
        yc = y.clamp(0, C - 1)
        prior0 = inside & (self.log_priors[yc] == -math.inf)
        n_nan, n_outside, n_prior0 = torch.stack((torch.isnan(S).any(1).sum(), (~inside).sum(), prior0.sum())).tolist()
        _refuse_labelled(n_nan, n_outside, n_prior0, C)
        return S.gather(1, yc[:, None])[:, 0] - torch.logsumexp(S, 1)

    def _labelled(self, Z, y):
        """(ll (N,) without a graph, the log-loss as a 0-dim float64 tensor) on whichever path applies."""
        Z = _samples(Z, self.covariances).detach()
        y = _labels(y, Z.shape[0], self.device)
        if NATIVE_LOG_LOSS and self._factors is not None and Z.is_cuda and Z.dtype in _NATIVE_DTYPES:
            W, offset = self._factors
            loss, ll, _, flags = _native_log_loss(Z.contiguous(), y, self._means_native, W, offset, want_ll=True)
            value, n_nan, n_outside, n_prior0 = torch.cat((loss.double(), flags.double())).tolist()   # one read
            _refuse_labelled(int(n_nan), int(n_outside), int(n_prior0), self.n_classes)
            return ll, value
        with torch.no_grad():
            ll = self._torch_label_log_proba(Z, y)
            return ll, -ll.double().mean().item()

    def label_log_proba(self, Z, y):
        """(N,) log posteriors of the labelled classes, log p(y_n | z_n) <= 0, without a graph: the labelled entries of
        ``predict_log_proba`` with nothing of size (N, C) formed on the native path.  ValueError, naming the count, for
        labels that are not (N,) integers, lie outside [0, C) or belong to a class of prior 0, and for samples with a
        non-finite score row."""
        return self._labelled(Z, y)[0]

    def log_loss(self, Z, y):
        """The log-loss -1/N sum_n log p(y_n | z_n), a Python float (one read from the device)."""
        return self._labelled(Z, y)[1]

    # ------------------------------------------------------------------ nested classifiers: the first k features, k = 1 .. K
    _nested_native = None   # (C, K) float64 offsets of the native path, built by the first nested call
    _nested_torch = None    # (C, K) offsets of the torch expression, in the dtype

    def _nested_offsets_native(self):
        """offset_k[c] (C, K) float64 from sqfa_gauss_class_factors_nested, once.  Its W has the bits of the constructor's
        factor pass, which stays in use; the classes were judged there, so its counter is not read."""
        if self._nested_native is None:
            lib = _lib.load()
            cov, C, K = self.covariances.detach().contiguous(), self.n_classes, self.n_features
            with _native._on_stream(cov.device) as stream:
                W = torch.empty_like(cov)
                offsets = torch.empty((C, K), dtype=torch.float64, device=cov.device)
                bad = torch.empty(1, dtype=torch.int32, device=cov.device)
                lp = self.log_priors.contiguous()
                _lib.check(lib.sqfa_gauss_class_factors_nested(_native._ptr(self._means_native), _native._ptr(cov),
                                                               _native._ptr(lp), C, K, _native._dtype_code(cov),
                                                               _native._ptr(W), _native._ptr(offsets), _native._ptr(bad),
                                                               stream), "sqfa_gauss_class_factors_nested")
            self._nested_native = offsets
        return self._nested_native

    def _nested_offsets_torch(self):
        """offset_k[c] (C, K) in the dtype, once: -sum_{i<k} log (L_c)_ii - k/2 log 2 pi + log pi_c."""
        if self._nested_torch is None:
            cov = self.covariances.detach()
            logdiag = torch.log(torch.diagonal(torch.linalg.cholesky_ex(cov)[0], dim1=-2, dim2=-1)).cumsum(-1)
            k = torch.arange(1, self.n_features + 1, dtype=cov.dtype, device=cov.device)
            self._nested_torch = -logdiag - 0.5 * math.log(2.0 * math.pi) * k + self.log_priors.to(cov.dtype)[:, None]
        return self._nested_torch

    def _use_nested_native(self, Z):
        return bool(NATIVE_NESTED) and self._use_native(Z)

    def _native_nested_call(self, Z, argmax=False, logsumexp=False, labels=None):
        """sqfa_gauss_scores_nested and, with labels, sqfa_gauss_label_scores_nested: (argmax (N,K) int64 | None, logsumexp
        (N,K) | None, ll (N,K) | None, flags (3,) int32 on the device: flagged samples and, with labels, labels outside
        [0, C) and labels on a class of prior 0)."""
        lib = _lib.load()
        Z = Z.detach().contiguous()
        W, offsets = self._factors[0], self._nested_offsets_native()
        N, K, C = Z.shape[0], self.n_features, self.n_classes
        code = _native._dtype_code(Z)
        logsumexp = logsumexp or labels is not None
        with _native._on_stream(Z.device) as stream:
            ws, nbytes = _native._workspace(lib.sqfa_gauss_scores_nested_workspace_bytes, N, C, K, code)
            out_a = torch.empty((N, K), dtype=torch.int64, device=Z.device) if argmax else None
            out_l = torch.empty((N, K), dtype=Z.dtype, device=Z.device) if logsumexp else None
            flags = torch.zeros(3, dtype=torch.int32, device=Z.device)
            mu = self._means_native
            _lib.check(lib.sqfa_gauss_scores_nested(_native._ptr(Z), N, _native._ptr(mu), _native._ptr(W),
                                                    _native._ptr(offsets), C, K, code, _native._ptr(out_a),
                                                    _native._ptr(out_l), _native._ptr(flags), _native._ptr(ws), nbytes,
                                                    stream), "sqfa_gauss_scores_nested")
            ll = None
            if labels is not None:
                ll = torch.empty((N, K), dtype=Z.dtype, device=Z.device)
                _lib.check(lib.sqfa_gauss_label_scores_nested(_native._ptr(Z), _native._ptr(labels), N, _native._ptr(mu),
                                                              _native._ptr(W), _native._ptr(offsets), C, K, code,
                                                              _native._ptr(out_l), _native._ptr(ll), _native._ptr(flags),
                                                              stream), "sqfa_gauss_label_scores_nested")
        return out_a, out_l, ll, flags

    def _torch_nested(self, Z, argmax=False, logsumexp=False, labels=None):
        """The same four as a torch expression without a graph: the chunked whitened differences of ``_torch_scores``, the
        cumulative sum of their squares over the feature axis plus the (C, K) offsets, and a running argmax, log-sum-exp
        and labelled score across the chunks, so that nothing of size (N, C, K) beyond one chunk is alive.  A sample with
        a NaN in any prefix is -1 / NaN in all K columns and counted."""
        with torch.no_grad():
            if self._torch is None:
                self._torch_factors()
            W, offsets = self._torch[0].detach(), self._nested_offsets_torch()
            Z = Z.detach()
            means = self.means.detach() if self.means is not None else None
            N, K, C = Z.shape[0], self.n_features, self.n_classes
            logsumexp = logsumexp or labels is not None
            step = max(1, min(C, FALLBACK_BYTES // max(1, 5 * N * K * Z.element_size())))
            nan = torch.zeros(N, dtype=torch.bool, device=Z.device)
            best = torch.full((K, N), -math.inf, dtype=Z.dtype, device=Z.device)
            arg = torch.zeros((K, N), dtype=torch.int64, device=Z.device)
            lse = torch.full((K, N), -math.inf, dtype=Z.dtype, device=Z.device)
            labelled = torch.zeros((K, N), dtype=Z.dtype, device=Z.device)
            inside = prior0 = None
            if labels is not None:
                inside = (labels >= 0) & (labels < C)
                yc = labels.clamp(0, C - 1)
                prior0 = inside & (self.log_priors[yc] == -math.inf)
            for c0 in range(0, C, step):
                Wc = W[c0:c0 + step]
                y = Wc @ Z.T if means is None else Wc @ (Z[None] - means[c0:c0 + step, None]).transpose(-1, -2)
                S = -0.5 * (y * y).cumsum(1) + offsets[c0:c0 + step, :, None]                 # (c, K, N)
                nan |= torch.isnan(S).flatten(0, 1).any(0)
                if argmax:
                    top, where = S.max(0)            # the first of equal maxima
                    better = top > best              # strictly: an earlier chunk keeps a tie
                    best = torch.where(better, top, best)
                    arg = torch.where(better, where + c0, arg)
                if logsumexp:
                    lse = torch.logaddexp(lse, torch.logsumexp(S, 0))
                if labels is not None:
                    mine = yc[None] == torch.arange(c0, c0 + Wc.shape[0], device=Z.device)[:, None]   # (c, N)
                    labelled = labelled + torch.where(mine[:, None], S, torch.zeros((), dtype=S.dtype, device=S.device)).sum(0)
            A = torch.where(nan[:, None], -1, arg.T) if argmax else None
            E = torch.where(nan[:, None], math.nan, lse.T) if logsumexp else None
            ll = None
            counts = [nan.sum()]
            if labels is not None:
                ll = (labelled.T - E).clamp(max=0.0) if C > 1 else torch.zeros_like(E)
                ll = torch.where((nan | ~inside | prior0)[:, None], math.nan, ll)
                counts += [(~inside).sum(), prior0.sum()]
            else:
                counts += [torch.zeros_like(counts[0])] * 2
            return A, E, ll, torch.stack(counts)

    def _nested(self, Z, argmax=False, logsumexp=False, labels=None):
        """(argmax, logsumexp, ll, the three counts as a device tensor) on whichever path applies."""
        Z = _samples(Z, self.covariances)
        if labels is not None:
            labels = _labels(labels, Z.shape[0], self.device)
        call = self._native_nested_call if self._use_nested_native(Z) else self._torch_nested
        return call(Z, argmax=argmax, logsumexp=logsumexp, labels=labels)

    def nested_predict(self, Z):
        """(N, K) int64: column k - 1 is ``predict`` of the classifier on the first k features; ties to the lowest index
        in every column."""
        A, _, _, flags = self._nested(Z, argmax=True)
        self._refuse(int(flags[0].item()))
        return A

    def nested_log_evidence(self, Z):
        """(N, K): column k - 1 is log p(z_n[:k]), the log evidence of the classifier on the first k features."""
        _, E, _, flags = self._nested(Z, logsumexp=True)
        self._refuse(int(flags[0].item()))
        return E

    def nested_accuracy(self, Z, y):
        """(K,) float64 CPU tensor: the share of samples predicted as y by the classifiers on the first 1 .. K features
        (one read from the device)."""
        labels = _labels(y, torch.as_tensor(Z).shape[0], self.device)
        A, _, _, flags = self._nested(Z, argmax=True)
        read = torch.cat(((A == labels[:, None]).sum(0), flags[:1].to(torch.int64))).tolist()
        self._refuse(read[-1])
        return torch.tensor(read[:-1], dtype=torch.float64) / A.shape[0]

    def nested_label_log_proba(self, Z, y):
        """(N, K) without a graph: column k - 1 is ``label_log_proba`` of the classifier on the first k features.  The
        refusals are those of ``label_log_proba``."""
        _, _, ll, flags = self._nested(Z, labels=y)
        _refuse_labelled(*flags.tolist(), self.n_classes)
        return ll

    def nested_log_loss(self, Z, y):
        """(K,) float64 CPU tensor: the log-loss of the classifiers on the first 1 .. K features, reduced over the samples
        in float64 (one read from the device, with the three flags)."""
        _, _, ll, flags = self._nested(Z, labels=y)
        read = torch.cat((ll.double().sum(0), flags.double())).tolist()
        _refuse_labelled(*(int(v) for v in read[-3:]), self.n_classes)
        return -torch.tensor(read[:-3], dtype=torch.float64) / ll.shape[0]


    # ------------------------------------------------------------------ top-k and the label's rank
    def _use_topk_native(self, Z):
        return bool(NATIVE_TOPK) and self._use_native(Z)

    def _sample_chunks(self, N, per_sample):
        """Ranges of samples whose temporaries of `per_sample` bytes each stay below FALLBACK_BYTES."""
        step = max(1, min(N, FALLBACK_BYTES // max(1, per_sample)))
        return [(n0, min(N, n0 + step)) for n0 in range(0, N, step)]

    def _native_topk(self, Z, k, scores):
        """One sqfa_gauss_scores_topk call: (indices (N,k) int64, scores (N,k) | None, the count of NaN rows (1,) int32)."""
        lib = _lib.load()
        Z = Z.detach().contiguous()
        W, offset = self._factors
        N, K, C = Z.shape[0], self.n_features, self.n_classes
        code = _native._dtype_code(Z)
        with _native._on_stream(Z.device) as stream:
            ws, nbytes = _native._workspace(lib.sqfa_gauss_scores_topk_workspace_bytes, N, C, K, code, k)
            index = torch.empty((N, k), dtype=torch.int64, device=Z.device)
            score = torch.empty((N, k), dtype=Z.dtype, device=Z.device) if scores else None
            bad = torch.empty(1, dtype=torch.int32, device=Z.device)
            _lib.check(lib.sqfa_gauss_scores_topk(_native._ptr(Z), N, _native._ptr(self._means_native), _native._ptr(W),
                                                  _native._ptr(offset), C, K, code, k, _native._ptr(index),
                                                  _native._ptr(score), _native._ptr(bad), _native._ptr(ws), nbytes, stream),
                       "sqfa_gauss_scores_topk")
        return index, score, bad

    def _torch_topk(self, Z, k, scores):
        """The same three from ``_torch_scores`` and a stable descending sort (equal scores keep their class order;
        torch.topk does not promise that), a chunk of samples at a time."""
        with torch.no_grad():
            Z = Z.detach()
            N, K, C, esz = Z.shape[0], self.n_features, self.n_classes, Z.element_size()
            index, score, bad = [], [], torch.zeros((), dtype=torch.int64, device=Z.device)
            for n0, n1 in self._sample_chunks(N, C * (3 * K * esz + 3 * esz + 16)):
                S = self._torch_scores(Z[n0:n1]).detach()
                nan = torch.isnan(S).any(1)
                top, where = torch.sort(S, dim=1, descending=True, stable=True)
                index.append(torch.where(nan[:, None], -1, where[:, :k]))
                if scores:
                    score.append(torch.where(nan[:, None], math.nan, top[:, :k]))
                bad = bad + nan.sum()
            return torch.cat(index), torch.cat(score) if scores else None, bad.reshape(1)

    def predict_topk(self, Z, k, return_scores=False):
        """(N, k) int64: the k classes of the largest scores, best first, equal scores in the order of their indices, so
        column 0 is ``predict(Z)``; with ``return_scores`` also their (N, k) scores.  1 <= k <= n_classes (ValueError
        otherwise); k <= 8 runs natively."""
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= self.n_classes:
            raise ValueError(f"k must be an int in [1, {self.n_classes}], got {k!r}")
        Z = _samples(Z, self.covariances)
        call = self._native_topk if k <= NATIVE_TOPK_MAX and self._use_topk_native(Z) else self._torch_topk
        index, score, bad = call(Z, k, return_scores)
        self._refuse(int(bad.item()))
        return (index, score) if return_scores else index

    def _native_rank(self, Z, labels):
        """One sqfa_gauss_label_rank call: (ranks (N,) int64, flags (2,) int32 on the device: samples with a NaN in their
        score row, labels outside [0, C))."""
        lib = _lib.load()
        Z = Z.detach().contiguous()
        W, offset = self._factors
        N, K, C = Z.shape[0], self.n_features, self.n_classes
        code = _native._dtype_code(Z)
        with _native._on_stream(Z.device) as stream:
            ws, nbytes = _native._workspace(lib.sqfa_gauss_label_rank_workspace_bytes, N, C, K, code)
            rank = torch.empty(N, dtype=torch.int64, device=Z.device)
            flags = torch.empty(2, dtype=torch.int32, device=Z.device)
            _lib.check(lib.sqfa_gauss_label_rank(_native._ptr(Z), _native._ptr(labels), N, _native._ptr(self._means_native),
                                                 _native._ptr(W), _native._ptr(offset), C, K, code, _native._ptr(rank), None,
                                                 _native._ptr(flags), _native._ptr(ws), nbytes, stream),
                       "sqfa_gauss_label_rank")
        return rank, flags

    def _torch_rank(self, Z, labels):
        """The same two as the count ((S > s_y) | ((S == s_y) & (c < y))).sum(1), a chunk of samples at a time."""
        with torch.no_grad():
            Z = Z.detach()
            N, K, C, esz = Z.shape[0], self.n_features, self.n_classes, Z.element_size()
            inside = (labels >= 0) & (labels < C)
            yc = labels.clamp(0, C - 1)
            classes = torch.arange(C, device=Z.device)
            rank, bad = [], torch.zeros((), dtype=torch.int64, device=Z.device)
            for n0, n1 in self._sample_chunks(N, C * (3 * K * esz + 2 * esz + 16)):
                S = self._torch_scores(Z[n0:n1]).detach()
                y = yc[n0:n1, None]
                s_y = S.gather(1, y)
                nan = torch.isnan(S).any(1)
                count = ((S > s_y) | ((S == s_y) & (classes < y))).sum(1)
                rank.append(torch.where(nan | ~inside[n0:n1], -1, count))
                bad = bad + nan.sum()
            return torch.cat(rank), torch.stack((bad, (~inside).sum()))

    def _scores_rank(self, Z, labels):
        """The same two from the native scores (sqfa_gauss_scores) and the count on them, a chunk of samples at a time: the
        same ranks as ``_native_rank``, whose scores have these bits."""
        N, C = Z.shape[0], self.n_classes
        inside = (labels >= 0) & (labels < C)
        yc = labels.clamp(0, C - 1)
        classes = torch.arange(C, device=Z.device)
        rank, bad = [], torch.zeros((), dtype=torch.int64, device=Z.device)
        for n0, n1 in self._sample_chunks(N, C * (Z.element_size() + 16)):
            S = self._native_call(Z[n0:n1], scores=True)[0]
            y = yc[n0:n1, None]
            s_y = S.gather(1, y)
            nan = torch.isnan(S).any(1)
            count = ((S > s_y) | ((S == s_y) & (classes < y))).sum(1)
            rank.append(torch.where(nan | ~inside[n0:n1], -1, count))
            bad = bad + nan.sum()
        return torch.cat(rank), torch.stack((bad, (~inside).sum()))

    def _rank(self, Z, y):
        """(ranks, the two counts as a device tensor) on whichever path applies."""
        Z = _samples(Z, self.covariances)
        labels = _labels(y, Z.shape[0], self.device)
        if not self._use_topk_native(Z):
            return self._torch_rank(Z, labels)
        if self.n_features > RANK_WIDE_FEATURES and self.n_classes < RANK_WIDE_MIN_CLASSES:
            return self._scores_rank(Z, labels)
        return self._native_rank(Z, labels)

    def label_rank(self, Z, y):
        """(N,) int64: the number of classes placed before the labelled one (a higher score, or an equal score and a lower
        index): 0 where ``predict(Z) == y``.  A label on a class of prior 0 is ranked like any other.  ValueError, naming
        the count, for labels that are not (N,) integers or lie outside [0, C), and for samples with a non-finite score
        row."""
        rank, flags = self._rank(Z, y)
        n_nan, n_outside = flags.tolist()
        _refuse_labelled(n_nan, n_outside, 0, self.n_classes)
        return rank

    def topk_accuracy(self, Z, y, k=(1, 5)):
        """The shares of samples whose labelled class is among the k best, from one ``label_rank`` pass and one read from
        the device: a (len(k),) float64 CPU tensor, or a Python float for an int ``k``.  Any k >= 1 (k >= n_classes gives
        1.0)."""
        ks = list(k) if isinstance(k, (tuple, list)) else [k]
        if not ks or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in ks):
            raise ValueError(f"k must be an int >= 1 or a sequence of them, got {k!r}")
        rank, flags = self._rank(Z, y)
        below = rank[:, None] < torch.tensor(ks, dtype=torch.int64, device=rank.device)[None]
        read = torch.cat((below.sum(0), flags.to(torch.int64))).tolist()
        _refuse_labelled(read[-2], read[-1], 0, self.n_classes)
        shares = torch.tensor(read[:-2], dtype=torch.float64) / rank.shape[0]
        return shares[0].item() if isinstance(k, int) else shares


def gaussian_class_scores(Z, means, covariances, priors=None):
    """(N, C) scores log p(z_n, c) of the samples Z (N, K) under the class Gaussians: means (C, K) or None (zero means),
    covariances (C, K, K), priors None / "uniform" / (C,) non-negative weights.  Differentiable where an input asks for it
    (the torch expression)."""
    return GaussianClassifier(means, covariances, priors).scores(Z)


class _GaussLogLoss(torch.autograd.Function):
    """The native log-loss: the factor pass and sqfa_gauss_log_loss forward (one read: the bad-class count and the three
    flags), sqfa_gauss_log_loss_backward for whichever of Z, means, covariances asks for a gradient (no read)."""

    @staticmethod
    def forward(ctx, Z, means, covariances, y, log_priors):
        Zc, cov = Z.detach().contiguous(), covariances.detach().contiguous()
        mu = means.detach().contiguous() if means is not None else None
        W, offset, bad = _native_class_factors(mu, cov, log_priors)
        loss, _, lse, flags = _native_log_loss(Zc, y, mu, W, offset)
        n_bad, n_nan, n_outside, n_prior0 = torch.cat((bad, flags)).tolist()
        _refuse_bad_classes(n_bad, cov.shape[0])
        _refuse_labelled(n_nan, n_outside, n_prior0, cov.shape[0])
        ctx.save_for_backward(Zc, y, mu, W, offset, lse)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Z, y, mu, W, offset, lse = ctx.saved_tensors
        want_z, want_mu, want_cov = ctx.needs_input_grad[:3]
        lib = _lib.load()
        N, K, C = Z.shape[0], Z.shape[1], W.shape[0]
        code = _native._dtype_code(Z)
        with _native._on_stream(Z.device) as stream:
            ws, nbytes = _native._workspace(lib.sqfa_gauss_log_loss_backward_workspace_bytes, N, C, K, code)
            up = g.detach().to(Z.dtype).reshape(1).contiguous()   # stays on the device
            gZ = torch.empty_like(Z) if want_z else None
            gmu = torch.empty_like(mu) if want_mu and mu is not None else None
            gcov = torch.empty_like(W) if want_cov else None
            _lib.check(lib.sqfa_gauss_log_loss_backward(_native._ptr(Z), _native._ptr(y), N, _native._ptr(mu),
                                                        _native._ptr(W), _native._ptr(offset), C, K, code,
                                                        _native._ptr(lse), _native._ptr(up), _native._ptr(gZ),
                                                        _native._ptr(gmu), _native._ptr(gcov), _native._ptr(ws), nbytes,
                                                        stream), "sqfa_gauss_log_loss_backward")
        return gZ, gmu, gcov, None, None


def gaussian_log_loss(Z, y, means, covariances, priors=None):
    """The log-loss -1/N sum_n log p(y_n | z_n) of the samples Z (N, K) with labels y (N,) integers under the class
    Gaussians (means (C, K) or None, covariances (C, K, K), priors as in GaussianClassifier): a 0-dim tensor,
    differentiable in Z, means and covariances (priors get no gradient).  float32 / float64 tensors on one GPU with K <= 64
    run on the native kernels, gradients included; elsewhere the torch expression.  Both refuse the same things with a
    ValueError that names the count: labels that are not (N,) integers, lie outside [0, C) or belong to a class of prior 0,
    samples with a non-finite score row, classes that are not symmetric positive definite or not finite."""
    mu, cov = _class_inputs(means, covariances)
    C, K = cov.shape[0], cov.shape[-1]
    Z = _samples(Z, cov)
    y = _labels(y, Z.shape[0], cov.device)
    if NATIVE_LOG_LOSS and K <= NATIVE_MAX_FEATURES and cov.is_cuda and cov.dtype in _NATIVE_DTYPES:
        return _GaussLogLoss.apply(Z, mu, cov, y, _log_priors(priors, C, cov.device))
    clf = GaussianClassifier(mu, cov, priors)
    return -clf._torch_label_log_proba(Z, y).mean()


def _statistics_and_priors(X, y, data_statistics, priors, estimator):
    """What from_model and feature_log_loss are given, resolved: (data_statistics, priors) with ``class_statistics`` of
    ``X, y`` where no statistics are given and "empirical" replaced by the class counts of ``y`` or of the ClassPoints."""
    counts = None
    if data_statistics is None:
        if X is None or y is None:
            raise ValueError("Either data_statistics or X and y must be provided.")
        data_statistics = class_statistics(X, y, estimator=estimator)
    if y is not None:
        counts = torch.bincount(torch.as_tensor(y).long().flatten())
    elif isinstance(data_statistics, ClassPoints):
        counts = data_statistics.counts
    if isinstance(priors, str) and priors == "empirical":
        if counts is None:
            raise ValueError("priors='empirical' needs the labels y or a ClassPoints (its class counts)")
        priors = counts
    return data_statistics, priors


def _class_gaussians(model, data_statistics, regularized):
    """(means | None, covariances (C,K,K)) of the class Gaussians in the feature space of ``model`` (SQFA: means and
    covariances; SecondMomentsSQFA: zero means and second moments), with whatever graph the model's methods build."""
    if hasattr(model, "_feature_statistics"):   # SQFA: the class Gaussians themselves
        stats = model._feature_statistics(data_statistics, regularized)
        means, cov = stats["means"], stats["covariances"]
    else:                                        # SecondMomentsSQFA: zero-mean Gaussians of the second moments
        means, cov = None, model._feature_scatters(data_statistics, regularized)
    if cov.dim() == 2:
        cov = cov[None]
    return means, cov


def _pad_priors(priors, n_classes):
    if torch.is_tensor(priors) and priors.shape[0] < n_classes:   # labels that stop short of the last class
        priors = torch.nn.functional.pad(priors, (0, n_classes - priors.shape[0]))
    return priors


def _feature_log_loss(model, X, y, data_statistics, priors, regularized):
    X = torch.as_tensor(X).to(device=model.filters.device, dtype=model.filters.dtype)
    means, cov = _class_gaussians(model, data_statistics, regularized)
    return gaussian_log_loss(model.transform(X), y, means, cov, _pad_priors(priors, cov.shape[0]))


def feature_log_loss(model, X, y, data_statistics=None, priors="uniform", regularized=True, estimator="empirical"):
    """The log-loss of the labelled points X (N, D), y (N,) under the class Gaussians in the feature space of the model's
    CURRENT filters, differentiable in the model's parameters: Z = model.transform(X) and the class Gaussians chosen as
    ``FeatureClassifier.from_model`` chooses them (``data_statistics``: a dict, a ClassPoints, for SecondMomentsSQFA a
    (C,D,D) tensor; None: class_statistics of ``X, y`` with ``estimator``), with the graph kept."""
    data_statistics, priors = _statistics_and_priors(X, y, data_statistics, priors, estimator)
    return _feature_log_loss(model, X, y, data_statistics, priors, regularized)


def fit_log_loss(model, X, y, data_statistics=None, priors="uniform", max_epochs=50, lr=0.1, atol=1e-6, **lbfgs_kwargs):
    """Refine the model's filters by L-BFGS on ``feature_log_loss`` (the Gaussian-likelihood objective; SQFA filters are its
    natural starting point).  The statistics are built once; the closure is eager.  Stops as the model's fit does: when the
    loss changes by less than ``atol`` for three consecutive epochs.  Extra keyword arguments go to torch.optim.LBFGS.
    Returns (losses, times), one entry per epoch."""
    data_statistics, priors = _statistics_and_priors(X, y, data_statistics, priors, "empirical")
    optimizer = torch.optim.LBFGS(list(model.parameters()), lr=lr, **lbfgs_kwargs)

    def closure():
        optimizer.zero_grad()
        loss = _feature_log_loss(model, X, y, data_statistics, priors, True)
        loss.backward()
        return loss

    losses, times = [], []
    start = time.time()
    previous, streak = 0.0, 0
    for _ in range(max_epochs):
        value = optimizer.step(closure).item()
        times.append(time.time() - start)
        losses.append(value)
        streak = streak + 1 if abs(previous - value) < atol else 0
        previous = value
        if streak >= 3:
            break
    return torch.tensor(losses), torch.tensor(times)


class FeatureClassifier:
    """A GaussianClassifier behind a snapshot of a model's filters: its methods take raw points X (N, D).  Built by
    ``FeatureClassifier.from_model``; ``classifier`` is the GaussianClassifier in feature space, ``filters`` (K, D)."""

    def __init__(self, filters, classifier):
        self.filters = filters
        self.classifier = classifier

    @classmethod
    def from_model(cls, model, X=None, y=None, data_statistics=None, priors="uniform", regularized=True,
                   estimator="empirical"):
        """The class Gaussians in the feature space of ``model`` (SQFA: means and covariances; SecondMomentsSQFA: zero
        means and second moments), from ``X, y`` (class_statistics with ``estimator``) or ``data_statistics`` (what the
        model's fit takes: a dict, a ClassPoints, or for SecondMomentsSQFA a (C,D,D) tensor).  ``regularized`` adds the
        model's noise_mat, as the closures do.  priors: "uniform" (None), "empirical" (the class counts of ``y`` or of the
        ClassPoints) or (C,) weights."""
        data_statistics, priors = _statistics_and_priors(X, y, data_statistics, priors, estimator)
        with torch.no_grad():
            filters = model.filters.detach().clone()
            means, cov = _class_gaussians(model, data_statistics, regularized)
            classifier = GaussianClassifier(means.detach() if means is not None else None, cov.detach(),
                                            _pad_priors(priors, cov.shape[0]))
        return cls(filters, classifier)

    n_classes = property(lambda self: self.classifier.n_classes)
    n_features = property(lambda self: self.classifier.n_features)
    log_priors = property(lambda self: self.classifier.log_priors)

    def transform(self, X):
        """(N, D) points -> (N, K) features through the snapshot of the filters."""
        X = torch.as_tensor(X).to(device=self.filters.device, dtype=self.filters.dtype)
        return X @ self.filters.T

    def scores(self, X):
        return self.classifier.scores(self.transform(X))

    def predict(self, X):
        return self.classifier.predict(self.transform(X))

    def log_evidence(self, X):
        return self.classifier.log_evidence(self.transform(X))

    def predict_log_proba(self, X):
        return self.classifier.predict_log_proba(self.transform(X))

    def predict_proba(self, X):
        return self.classifier.predict_proba(self.transform(X))

    def accuracy(self, X, y):
        return self.classifier.accuracy(self.transform(X), y)

    def label_log_proba(self, X, y):
        return self.classifier.label_log_proba(self.transform(X), y)

    def log_loss(self, X, y):
        return self.classifier.log_loss(self.transform(X), y)

    def nested_predict(self, X):
        return self.classifier.nested_predict(self.transform(X))

    def nested_log_evidence(self, X):
        return self.classifier.nested_log_evidence(self.transform(X))

    def nested_accuracy(self, X, y):
        return self.classifier.nested_accuracy(self.transform(X), y)

    def nested_label_log_proba(self, X, y):
        return self.classifier.nested_label_log_proba(self.transform(X), y)

    def nested_log_loss(self, X, y):
        return self.classifier.nested_log_loss(self.transform(X), y)

    def predict_topk(self, X, k, return_scores=False):
        return self.classifier.predict_topk(self.transform(X), k, return_scores)

    def label_rank(self, X, y):
        return self.classifier.label_rank(self.transform(X), y)

    def topk_accuracy(self, X, y, k=(1, 5)):
        return self.classifier.topk_accuracy(self.transform(X), y, k)
