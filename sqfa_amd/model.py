"""SQFA models with the reference's API (src/sqfa/model.py): ``SecondMomentsSQFA`` and
``SQFA`` with ``fit`` / ``fit_pca`` / ``transform`` / ``transform_scatters`` /
``get_class_distances``.  Orchestration only: the class statistics, the projection
F Sigma_c F^T, the parametrizations and LBFGS stay in PyTorch-ROCm; the pairwise distances
and their backward run on the HIP kernels (distances.py, _native.py).
"""
import collections

import torch
import torch.nn as nn
from torch.nn.utils.parametrize import register_parametrization, remove_parametrizations

from . import _native, distances
from . import divergences  # noqa: F401  (registers its operators with distances.class_pair_spec)
from . import logdet  # noqa: F401  (likewise)
from ._memo import TensorMemo
from ._optim import fitting_loop
from .constraints import FixedFilters, Identity, Orthogonal, Sphere, orthogonal
from .linalg import conjugate_matrix
from .statistics import ClassPoints, class_statistics, pca, pca_from_scatter

__all__ = ["SecondMomentsSQFA", "SQFA"]


def __dir__():
    return __all__


_DICT_KEYS = {"means", "covariances"}


def _check_statistics(data_statistics, needs_dict=False):
    """Accept a (C,D,D) tensor-like or a dict with 'means' and 'covariances'
    (reference: model.py:56-94; same exception types), or the labelled points themselves (statistics.ClassPoints), which
    stand for both forms."""
    if isinstance(data_statistics, ClassPoints):
        return
    if isinstance(data_statistics, dict):
        missing = _DICT_KEYS - set(data_statistics.keys())
        if missing:
            raise ValueError(
                f"`data_statistics` dictionary must contain the keys {_DICT_KEYS}. Missing keys: {missing}"
            )
        return
    if not hasattr(data_statistics, "shape"):
        raise TypeError(
            "`data_statistics` must be either a dict with 'means' and 'covariances' "
            "or a torch.Tensor of shape (n_classes, n_dim, n_dim)."
        )
    if needs_dict:
        raise TypeError(
            "`data_statistics` must be a dictionary with 'means' and 'covariances' when `needs_dict` is True."
        )


def _statistics_from_points(model, X, y, estimator, statistics):
    """What fit(X=, y=) hands to the fitting loop: the dense class statistics ("dense", the default) or the labelled
    points themselves ("points": statistics.ClassPoints, nothing of size (C,D,D) is formed)."""
    if statistics == "dense":
        return class_statistics(X, y, estimator=estimator)
    if statistics != "points":
        raise ValueError("statistics must be 'dense' or 'points'")
    if estimator != "empirical":
        raise ValueError("statistics='points' supports estimator='empirical' only: OAS shrinkage needs tr(S_c^2) of "
                         "every class in data space; use statistics='dense' for it")
    _refuse_sharded_points(model)
    return ClassPoints(X, y)


def _refuse_sharded_points(model):
    if model.class_shard is not None:
        raise NotImplementedError("class_shard works on dense class statistics only: points cannot be sharded over classes")


_scatters = TensorMemo(max_entries=4)   # (cov, mu) -> second moments; a handful of live statistics at most (C*D*D values each)


def _stats_to_scatter(statistics):
    """Second-moment matrices from either input form (reference: model.py:24-53).  For a dict the (C,D,D) sum
    cov + mu mu^T is formed ONCE per pair of input tensors (and versions) and the same tensor object is handed out
    again: the reference recomputes it inside every call, and a fresh tensor per call would also make
    every get_class_distances / transform_scatters call re-check the symmetry of (C,D,D) values."""
    if not isinstance(statistics, dict):
        return statistics
    _check_statistics(statistics)
    mu, cov = statistics["means"], statistics["covariances"]
    if not (torch.is_tensor(mu) and torch.is_tensor(cov)) or mu.requires_grad or cov.requires_grad:
        return cov + mu[:, :, None] * mu[:, None, :]
    hit = _scatters.get(cov, mu)
    return hit if hit is not None else _scatters.put(cov + mu[:, :, None] * mu[:, None, :], cov, mu)


# What one closure evaluation runs (SecondMomentsSQFA._closure_plan): the method _evaluate_<evaluator> and its static
# arguments.  scale: the pair kernels' scale, or the SQFA_GAUSS_* kind code; metric: "airm" | "bw" | "gauss" | None;
# weight: -1 / #pairs; shard, reducer: the pair tiles of a multi-GPU fit; inputs: the single node's (raw filters, scatters,
# means, parametrization kind, noise).  weight and inputs are None in a plan made without statistics.  pair_weights: the
# fit's normalised (C,C) per-pair weights (_native.normalized_pair_weights) that replace `weight`, or None (uniform).
ClosurePlan = collections.namedtuple("ClosurePlan", "evaluator scale sqrt_mode metric weight shard reducer inputs pair_weights",
                                     defaults=(None,))
_NATIVE_DTYPES = (torch.float32, torch.float64)


class SecondMomentsSQFA(nn.Module):
    """smSQFA: filters maximising the mean pairwise affine-invariant distance between the
    class second-moment matrices of the filtered data (reference: model.py:97-444)."""

    def __init__(self, n_dim, feature_noise=0, n_filters=2, filters=None, distance_fun=None,
                 constraint="sphere"):
        super().__init__()
        if filters is None:
            filters = torch.randn(n_filters, n_dim)
        else:
            filters = torch.as_tensor(filters, dtype=torch.float32)
        if filters.shape[0] > filters.shape[1]:
            raise ValueError("Number of filters must be less than or equal to the data dimension.")
        self.filters = nn.Parameter(filters)
        # the reference sizes this from n_filters even when `filters` is given;
        # sizing it from the filters is the superset behaviour
        self.register_buffer("noise_mat", self._noise_matrix(feature_noise, filters.shape[0]))
        self.distance_fun = distances.affine_invariant if distance_fun is None else distance_fun
        self.constraint = constraint
        self._add_constraint(constraint)
        self.pair_shard = None   # optional sqfa_amd.parallel.PairShard for multi-GPU fits
        self.class_shard = None  # optional sqfa_amd.parallel.ClassShard: statistics hold local classes only
        self._pair_weights = None  # the running fit's normalised per-pair weights (set and cleared by fitting_loop)

    @staticmethod
    def _noise_matrix(feature_noise, k):
        return torch.as_tensor(feature_noise, dtype=torch.float32) * torch.eye(k)

    # ------------------------------------------------------------------ transforms
    def transform_scatters(self, data_scatters):
        """(C,D,D) scatter matrices -> (C,K,K) feature scatters F S F^T (reference: model.py:172-188).
        float32 GPU inputs go through the single-pass streaming kernel (scatters are read from
        HBM once per closure, forward and backward together); other inputs use the torch
        expression of conjugate_matrix."""
        filters = self.filters
        native = _native.project_scatters(data_scatters, filters)
        if native is not None:
            return native.squeeze(0) if native.shape[0] == 1 else native
        return conjugate_matrix(data_scatters, filters)

    def transform(self, data_points):
        """(N,D) points -> (N,K) features (reference: model.py:222-237)."""
        return data_points @ self.filters.T

    # ------------------------------------------------------------------ distances
    def _feature_scatters(self, data_statistics, regularized):
        if isinstance(data_statistics, ClassPoints):   # second moments of the projected points: no (C,D,D) statistics
            S = data_statistics.feature_statistics(self.filters, second_moments=True)["second_moments"]
        else:
            S = self.transform_scatters(_stats_to_scatter(data_statistics))
        if regularized:
            S = S + self.noise_mat[None]
        return S

    def get_class_distances(self, data_statistics, regularized=False):
        """(C,C) pairwise distances between the class feature scatters
        (reference: model.py:190-220)."""
        S = self._feature_scatters(data_statistics, regularized)
        return self.distance_fun(S, S)

    # hooks used by the fitting loop ------------------------------------------------------
    def _prepare_statistics(self, data_statistics):
        # a dict is reduced to second moments once instead of inside every closure; symmetric float32 GPU
        # statistics of many classes are also packed once into their lower block triangle: every closure then streams
        # ~52 % of the bytes (sqfa_project_scatters_packed; _native.prepare_packed decides and keeps the packed copy)
        if isinstance(data_statistics, ClassPoints):
            _refuse_sharded_points(self)
            return data_statistics
        scatters = _stats_to_scatter(data_statistics)
        _native.prepare_packed(scatters, self.filters.shape[0])
        return scatters

    def _fused_input(self, prepared):
        return self._feature_scatters(prepared, True)

    _fused_kind = "spd"

    def _has_fused_closure(self):
        """True when distance_fun is a native operator this model's fused closure evaluates."""
        return self._closure_plan() is not None

    # the whole closure as ONE autograd node (8 / 11 launches instead of ~40): _native.FusedClosure
    SINGLE_NODE_CLOSURE = True

    def _single_node_inputs(self, prepared, allow_class_shard=False):
        """(raw parameter, scatters, means, kind) when the closure can run as one node: a single Sphere (kind True),
        Identity (False) or native Orthogonal (its `base` tensor) parametrization on the filters, supported shapes;
        class-sharded statistics only for the fitting loop's staged (graph) closure, which places the collectives itself."""
        if not self.SINGLE_NODE_CLOSURE or (self.class_shard is not None and not allow_class_shard):
            return None
        plist = getattr(getattr(self, "parametrizations", None), "filters", None)
        if plist is None or len(plist) != 1 or type(plist[0]) not in (Sphere, Identity, Orthogonal):
            return None
        raw = plist.original
        kind = type(plist[0]) is Sphere
        if type(plist[0]) is Orthogonal:
            kind = plist[0].native_base(raw)
            if kind is None:
                return None
        if isinstance(prepared, dict):
            scatters, means = prepared["covariances"], prepared["means"]
        else:
            scatters, means = prepared, None
        if not torch.is_tensor(scatters) or scatters.dim() != 3 or scatters.dtype != raw.dtype:
            return None
        if not (raw.is_cuda and raw.dim() == 2 and raw.is_contiguous()):
            return None
        if means is not None and not (means.is_cuda and means.dtype == scatters.dtype and means.dim() == 2
                                      and not means.requires_grad):
            return None
        # the streaming projection's conditions: symmetric float32/float64 scatters on the GPU, D % 4 == 0, K <= 64, 16-byte aligned
        return (raw, scatters, means, kind) if _native.native_projection_supported(scatters, raw) else None

    @staticmethod
    def _pair_weight(C):
        """-1 / #unordered class pairs: the kernels' sum over the pairs becomes the reference's -mean (src/sqfa/_optim.py:94)."""
        return -1.0 / (C * (C - 1) // 2)

    def _closure_plan(self, prepared=None, staged=False):
        """The ClosurePlan of this model's fused closure, or None: the fitting loop's generic closure, never captured in a
        graph.  THE place where an evaluator is chosen and where its limits are written.  Without `prepared` only the
        conditions that need no statistics apply (what the fitting loop arms its graph capture on; the pair family then
        names the chain); with it the plan is final: whatever it names, _fused_closure_loss evaluates.
        `staged`: the caller places the collectives itself (_optim.ShardedClosure): class-sharded statistics may take the
        single node."""
        fn, nm = self.distance_fun, self.noise_mat   # noise_mat: (K,K), the model's dtype (reading self.filters would run the parametrization)
        sharded = self.pair_shard is not None or self.class_shard is not None
        spec = distances.fused_spec(fn)
        pair = distances.class_pair_spec(fn)
        plan = inputs = None
        if pair is None and spec is not None and spec[0] == self._fused_kind:
            # affine-invariant / Bures-Wasserstein pair kernels: any device (through _pair_backend), any sharding
            shard, reducer = (self.pair_shard.shard, self.pair_shard.reduce) if self.pair_shard is not None else ((0, 1), None)
            plan = ClosurePlan("chain", spec[1], spec[2], spec[3], None, shard, reducer, None)
            if prepared is not None:
                single = self._single_node_inputs(prepared, allow_class_shard=staged)
                noise = self._noise_scalar() if single is not None else None   # a non-scalar noise_mat keeps the chain
                if noise is not None:
                    plan, inputs = plan._replace(evaluator="single_node"), single + (noise,)
        elif pair is not None and pair[1] == self._fused_kind:
            # the class-pair losses (bhattacharyya / hellinger / mahalanobis[_sq], log_euclidean[_sq], jeffreys[_spd][_root],
            # stein[_root]):
            # single process, filters within the family's limit, float32/64 GPU statistics of the model's input kind
            family, kind, mode = pair
            if sharded or nm.shape[0] > _native.pair_family(family).limit or nm.dtype not in _NATIVE_DTYPES:
                return None
            if prepared is not None and not self._class_pair_statistics(prepared, kind, nm.dtype):
                return None
            if family == "gauss":
                plan = ClosurePlan("gauss", mode, spec[2], "gauss", None, (0, 1), None, None)
            else:
                plan = ClosurePlan(family, None, mode, None, None, (0, 1), None, None)
        if plan is None or prepared is None:
            return plan
        return plan._replace(weight=self._pair_weight(self._n_classes_total(prepared)), inputs=inputs,
                             pair_weights=self._pair_weights)

    @staticmethod
    def _class_pair_statistics(prepared, kind, noise_dtype):
        """True when `prepared` is what a class-pair loss of input kind `kind` takes: a ClassPoints, a dict of means and
        covariances ("gaussian") or a (C,D,D) tensor ("spd"), at least two classes, on the GPU, the features float32/64."""
        if isinstance(prepared, ClassPoints):   # feature moments of the points' dtype, on their device
            return bool(prepared.points.is_cuda and prepared.n_classes >= 2
                        and torch.promote_types(prepared.dtype, noise_dtype) in _NATIVE_DTYPES)
        if kind == "gaussian":
            if not isinstance(prepared, dict):
                return False
            mu, cov = prepared["means"], prepared["covariances"]
            cov_dtype = torch.promote_types(cov.dtype, noise_dtype)   # of F cov F^T + noise_mat
            return bool(cov.is_cuda and cov.dim() == 3 and mu.dim() == 2 and cov.shape[0] >= 2 and cov_dtype in _NATIVE_DTYPES
                        and mu.dtype == cov_dtype and mu.device == cov.device)
        return bool(torch.is_tensor(prepared) and prepared.dim() == 3 and prepared.is_cuda and prepared.shape[0] >= 2
                    and torch.promote_types(prepared.dtype, noise_dtype) in _NATIVE_DTYPES)

    def _fused_closure_loss(self, prepared):
        """(loss, flags) through the fused loss+gradient evaluator of _closure_plan, or None when there is none (the
        fitting loop's generic closure)."""
        plan = self._closure_plan(prepared)
        return None if plan is None else getattr(self, "_evaluate_" + plan.evaluator)(plan, prepared)

    def _evaluate_single_node(self, plan, prepared):
        """The whole closure as ONE autograd node (_native.FusedClosure)."""
        raw, scatters, means, sphere, noise = plan.inputs
        return _native.FusedClosure.apply(raw, scatters, means, noise, plan.scale, plan.sqrt_mode, plan.weight, plan.shard,
                                          plan.reducer, sphere, plan.metric, plan.pair_weights)

    def _evaluate_chain(self, plan, prepared):
        """The same loss as a chain of autograd nodes (parametrization -> projection -> noise -> [embedding] ->
        PairwiseLoss): any parametrization or device, class-sharded statistics, a non-scalar noise_mat."""
        S = self._fused_input(prepared)
        if self.class_shard is not None:
            S = self.class_shard.gather(S)
        return _native.PairwiseLoss.apply(S, plan.scale, distances.EPSILON, plan.sqrt_mode, plan.weight, plan.shard,
                                          plan.reducer, plan.metric, plan.pair_weights)

    def _evaluate_class_pairs(self, plan, prepared):
        """parametrization -> projection (native where it applies) -> noise -> _native.ClassPairLoss (one fused pass over
        the class pairs): with the feature means and covariances (SQFA), or the feature scatters and no means
        (SecondMomentsSQFA)."""
        if self._fused_kind == "gaussian":
            stats = self._feature_statistics(prepared, True)
            mu, cov = stats["means"], stats["covariances"]
        else:
            mu, cov = None, self._feature_scatters(prepared, True)
        mode = int(plan.scale) if plan.evaluator == "gauss" else plan.sqrt_mode
        return _native.ClassPairLoss.apply(mu, cov, plan.evaluator, mode, distances.EPSILON, plan.weight, plan.pair_weights)

    _evaluate_gauss = _evaluate_log_euclidean = _evaluate_jeffreys = _evaluate_class_pairs
    _evaluate_stein = _evaluate_class_pairs

    def _noise_scalar(self):
        """feature_noise as a host scalar when noise_mat is (still) noise * I, else None; read back once
        per buffer state, never inside a graph capture."""
        key = (self.noise_mat.data_ptr(), self.noise_mat._version, tuple(self.noise_mat.shape))
        cached = getattr(self, "_noise_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        if torch.cuda.is_current_stream_capturing():
            return None
        nm = self.noise_mat.detach()
        value = float(nm[0, 0])
        if not bool(torch.equal(nm, value * torch.eye(nm.shape[0], dtype=nm.dtype, device=nm.device))):
            value = None
        self._noise_cache = (key, value)
        return value

    def _sync_gradients(self):
        """Called by the fitting loop after backward: sums the filter gradient over class shards."""
        if self.class_shard is not None:
            self.class_shard.reduce_gradients(self.parameters())

    def _n_classes_total(self, prepared):
        if self.class_shard is not None:
            return self.class_shard.n_classes
        if isinstance(prepared, ClassPoints):
            return prepared.n_classes
        return prepared["means"].shape[0] if isinstance(prepared, dict) else prepared.shape[0]

    # ------------------------------------------------------------------ fitting
    def fit_pca(self, X=None, data_statistics=None):
        """Set the filters to PCA directions (of X, or via ``pca_from_scatter``)
        (reference: model.py:239-268)."""
        if X is None and data_statistics is None:
            raise ValueError("Either X or data_statistics must be provided.")
        if isinstance(data_statistics, ClassPoints):
            raise TypeError("fit_pca takes the points themselves as X= (or dense data_statistics), not a ClassPoints: "
                            "call fit_pca(X=class_points.points)")
        k = self.filters.shape[0]
        if data_statistics is None:
            components = pca(X, k)
        elif self.class_shard is not None:
            # statistics hold the local classes only: average the scatters over all ranks first
            local_sum = _stats_to_scatter(data_statistics).sum(dim=0)
            torch.distributed.all_reduce(local_sum, group=self.class_shard.group)
            if k > local_sum.shape[-1]:
                raise ValueError("n_components must be less than or equal to n_dim.")
            components = pca(local_sum / self.class_shard.n_classes, n_components=k)
        else:
            components = pca_from_scatter(_stats_to_scatter(data_statistics), k)
        self._replace_filters(components)

    def _replace_filters(self, new_filters, n_row_fixed=0):
        remove_parametrizations(self, "filters")
        self.filters = nn.Parameter(new_filters)
        self._add_constraint(self.constraint)
        if n_row_fixed:
            register_parametrization(self, "filters", FixedFilters(n_row_fixed=n_row_fixed))

    def fit(self, X=None, y=None, data_statistics=None, max_epochs=300, lr=0.1, estimator="empirical",
            pairwise=False, show_progress=True, return_loss=False, atol=1e-6, pair_weights=None, statistics="dense",
            **kwargs):
        """Fit the filters with LBFGS (reference: model.py:270-414).  Either ``X, y`` or
        ``data_statistics``; ``pairwise=True`` learns the filters two at a time, holding the
        earlier ones fixed.  ``pair_weights``: optional symmetric, non-negative (C,C) weights W of the class pairs; the
        loss becomes -sum_{i>j} W_ij D_ij / sum_{i>j} W_ij (the diagonal is ignored; every stage of a pairwise fit uses the
        same weights).  ``statistics`` (with ``X, y``): "dense" (default) builds the (C,D,D) class statistics once;
        "points" keeps the labelled points (statistics.ClassPoints, also accepted as ``data_statistics``) and every closure
        computes the class moments of the projected points: nothing of size (C,D,D) is formed (empirical estimator only;
        for OAS shrinkage without (C,D,D) statistics pass ``data_statistics=ClassPoints(X, y, estimator="oas")``).
        Extra keyword arguments go to torch.optim.LBFGS."""
        if data_statistics is None:
            if X is None or y is None:
                raise ValueError("Either data_statistics or X and y must be provided.")
            data_statistics = _statistics_from_points(self, X, y, estimator, statistics)
        _check_statistics(data_statistics)
        loop = dict(max_epochs=max_epochs, lr=lr, show_progress=show_progress, return_loss=True,
                    atol=atol, pair_weights=pair_weights, **kwargs)
        if not pairwise:
            loss, elapsed = fitting_loop(model=self, data_statistics=data_statistics, **loop)
        else:
            loss, elapsed = self._fit_pairwise(data_statistics, loop)
        return (loss, elapsed) if return_loss else None

    def _fit_pairwise(self, data_statistics, loop):
        k_total = self.filters.shape[0]
        if k_total % 2 != 0:
            raise ValueError("Number of filters must be even for pairwise training.")
        start_filters = self.filters.detach().clone()
        noise_level = self.noise_mat.detach().clone()[0, 0]
        loss = torch.tensor([])
        elapsed = torch.tensor([])
        for stage in range(k_total // 2):
            done = 2 * stage
            learned = self.filters.detach().clone()
            fresh = start_filters[done:done + 2]
            init = fresh.contiguous() if stage == 0 else torch.cat((learned, fresh))
            self._replace_filters(init, n_row_fixed=done)
            self.register_buffer(
                "noise_mat", noise_level * torch.eye(done + 2, dtype=noise_level.dtype, device=noise_level.device))
            stage_loss, stage_time = fitting_loop(model=self, data_statistics=data_statistics, **loop)
            # drop the FixedFilters layer again
            remove_parametrizations(self, "filters")
            self._add_constraint(self.constraint)
            if elapsed.numel() > 0:
                stage_time = stage_time + elapsed[-1]
            loss = torch.cat((loss, stage_loss))
            elapsed = torch.cat((elapsed, stage_time))
        return loss, elapsed

    def _add_constraint(self, constraint="none"):
        """'none' | 'sphere' | 'orthogonal' (reference: model.py:416-431)."""
        if constraint == "none":
            register_parametrization(self, "filters", Identity())
        elif constraint == "sphere":
            register_parametrization(self, "filters", Sphere())
        elif constraint == "orthogonal":
            orthogonal(self, "filters")

    def __dir__(self):
        return ["filters", "noise_mat", "distance_fun", "constraint", "transform_scatters",
                "get_class_distances", "transform", "fit_pca"]


class SQFA(SecondMomentsSQFA):
    """SQFA: uses class means and covariances; the default discriminability measure is the
    Calvo-Oller lower bound of the Fisher-Rao distance (reference: model.py:447-630)."""

    _fused_kind = "gaussian"

    def __init__(self, n_dim, feature_noise=0, n_filters=2, filters=None, distance_fun=None,
                 constraint="sphere"):
        super().__init__(
            n_dim=n_dim, feature_noise=feature_noise, n_filters=n_filters, filters=filters,
            distance_fun=distances.fisher_rao_lower_bound if distance_fun is None else distance_fun,
            constraint=constraint,
        )

    def _feature_statistics(self, data_statistics, regularized):
        if isinstance(data_statistics, ClassPoints):   # means and covariances of the projected points
            stats = data_statistics.feature_statistics(self.filters)
            cov = stats["covariances"] + self.noise_mat[None] if regularized else stats["covariances"]
            return {"means": stats["means"], "covariances": cov}
        cov = self.transform_scatters(data_statistics["covariances"])
        if regularized:
            cov = cov + self.noise_mat[None]
        return {"means": self.transform(data_statistics["means"]), "covariances": cov}

    def get_class_distances(self, data_statistics, regularized=False):
        """(C,C) pairwise distances between the class feature Gaussians
        (reference: model.py:508-546)."""
        if not isinstance(data_statistics, (dict, ClassPoints)):
            raise TypeError("data_statistics must be a dictionary with 'means' and 'covariances' keys.")
        stats = self._feature_statistics(data_statistics, regularized)
        return self.distance_fun(stats, stats)

    def _prepare_statistics(self, data_statistics):
        if isinstance(data_statistics, ClassPoints):
            _refuse_sharded_points(self)
            return data_statistics
        if not isinstance(data_statistics, dict):
            raise TypeError("data_statistics must be a dictionary with 'means' and 'covariances' keys.")
        _native.prepare_packed(data_statistics["covariances"], self.filters.shape[0])   # see SecondMomentsSQFA._prepare_statistics
        return data_statistics

    def _fused_input(self, prepared):
        return distances.embed_gaussian(self._feature_statistics(prepared, True))

    def fit(self, X=None, y=None, data_statistics=None, max_epochs=300, lr=0.1, estimator="empirical",
            pairwise=False, show_progress=True, return_loss=False, atol=1e-6, pair_weights=None, statistics="dense",
            **kwargs):
        """Fit with LBFGS (reference: model.py:548-630); ``data_statistics`` must be a dict or a ClassPoints.  ``pair_weights``
        and ``statistics`` as in SecondMomentsSQFA.fit."""
        if data_statistics is None:
            if X is None or y is None:
                raise ValueError("Either data_statistics or X and y must be provided.")
            data_statistics = _statistics_from_points(self, X, y, estimator, statistics)
        else:
            _check_statistics(data_statistics, needs_dict=True)
        out = super().fit(data_statistics=data_statistics, max_epochs=max_epochs, lr=lr, estimator=estimator,
                          pairwise=pairwise, show_progress=show_progress, return_loss=True, atol=atol,
                          pair_weights=pair_weights, **kwargs)
        return out if return_loss else None
