"""Class statistics and PCA initialisation (reference: src/sqfa/statistics.py).

Runs once per fit, before the hot path, on the input's device (the reference allocates on the CPU only).
float32 / float64 points on the GPU go through the native segmented SYRK (sqfa_class_moments: no sorted or padded
copy of the points, exactly symmetric outputs); CPU tensors and other dtypes keep the batched torch expression.
ClassStatisticsAccumulator builds the same statistics from batches and merges partial results.
ClassPoints keeps the labelled points themselves as the statistics of a fit: every closure computes the class moments of
the projected points (sqfa_class_feature_moments) and nothing of size (C,D,D) is ever formed; with estimator="oas" the
covariances are shrunk as class_statistics shrinks them, from coefficients measured once (sqfa_class_shrinkage).
"""
import torch

__all__ = ["class_statistics", "ClassStatisticsAccumulator", "ClassPoints", "oas_covariance", "sample_covariance", "pca",
           "pca_from_scatter"]

# float32 / float64 points on the GPU take the native kernels; False keeps the batched torch expression everywhere
NATIVE_CLASS_STATISTICS = True
# ClassPoints on float32 / float64 GPU points takes the native kernels; False keeps its torch expression everywhere
NATIVE_CLASS_POINTS = True


def __dir__():
    return __all__


def sample_covariance(points, assume_centered=False):
    """Sample covariance of (n_points, n_dim) data; 1/(n-1) after centring, 1/n when the data
    is declared centred (reference: statistics.py:97-124)."""
    n = points.shape[0]
    if assume_centered:
        return points.T @ points / n
    centred = points - points.mean(dim=0)
    return centred.T @ centred / (n - 1)


def oas_covariance(points, assume_centered=False):
    """Oracle Approximating Shrinkage estimate, Chen et al. 2010 (reference: statistics.py:57-94)."""
    n, d = points.shape
    S = sample_covariance(points, assume_centered=assume_centered)
    tr = torch.trace(S)
    tr2 = (S * S).sum()
    rho = ((1 - 2 / d) * tr2 + tr * tr) / ((n + 1 - 2 / d) * (tr2 - tr * tr / d))
    rho = torch.clamp(rho, max=1.0)
    target = torch.eye(d, dtype=S.dtype, device=S.device) * (tr / d)
    return (1 - rho) * S + rho * target


# padded class batches hold at most this many point-matrix elements (x2 for the centred copy)
_BATCH_ELEMENTS = 1 << 27


def class_statistics(points, labels, estimator="empirical"):
    """Per-class mean, covariance and second moment.  Labels are integers 0..C-1
    (reference: statistics.py:8-54; keys 'means', 'covariances', 'second_moments').

    The reference selects each class with a boolean mask inside a Python loop (one
    ``nonzero`` host sync and ~8 small launches per class: launch-bound for many classes).
    Here the points are sorted by label once (stable), the class sizes come back in ONE host
    transfer, and classes of similar size are processed together as zero-padded batches
    ``(G, n_max, D)``: masked centring, one batched GEMM ``Xc^T Xc`` per group, batched OAS
    shrinkage.  Same estimators (centre first, then 1/(n-1)), different summation order."""
    if estimator not in ("empirical", "oas"):
        raise ValueError("estimator must be 'empirical' or 'oas'")
    labels = labels.to(points.device).long()   # the reference accepts float labels too (it compares with ==)
    n_classes = int(labels.max()) + 1
    if NATIVE_CLASS_STATISTICS and _native_applies(points):
        # the class count above is the only host read: sizes and offsets stay on the device
        from . import _native
        order, class_start = _native.grouped_rows(labels, n_classes)
        code = _native.COV_OAS if estimator == "oas" else _native.COV_EMPIRICAL
        means, covs, second = _native.class_moments(points, order, class_start, n_classes, code, True)
        return {"means": means, "covariances": covs, "second_moments": second}
    d = points.shape[-1]
    order = torch.sort(labels, stable=True).indices
    counts_dev = torch.bincount(labels, minlength=n_classes)
    counts = counts_dev.tolist()
    starts_dev = torch.cumsum(counts_dev, 0) - counts_dev
    sorted_points = points[order]
    means = points.new_zeros(n_classes, d)
    covs = points.new_zeros(n_classes, d, d)
    # groups of classes of similar size (little padding), bounded in memory
    by_size = sorted(range(n_classes), key=lambda c: counts[c])
    pos = 0
    while pos < n_classes:
        group = [by_size[pos]]
        pos += 1
        while pos < n_classes:
            n_max = max(counts[by_size[pos]], 1)
            if (len(group) + 1) * n_max * d > _BATCH_ELEMENTS or n_max > 2 * max(counts[group[0]], 16):
                break
            group.append(by_size[pos])
            pos += 1
        cls = torch.as_tensor(group, device=points.device)
        m, c = _batched_moments(sorted_points, starts_dev[cls], counts_dev[cls], max(counts[group[-1]], 1), estimator)
        means[cls] = m
        covs[cls] = c
    second = covs + means[:, :, None] * means[:, None, :]
    return {"means": means, "covariances": covs, "second_moments": second}


def _native_applies(points):
    return points.is_cuda and points.dim() == 2 and points.dtype in (torch.float32, torch.float64) and points.shape[1] >= 1


def _oas_shrink(S, n):
    """Batched OAS shrinkage of (G,D,D) sample covariances of n (G) points each (Chen et al. 2010, as oas_covariance)."""
    d = S.shape[-1]
    tr = torch.diagonal(S, dim1=1, dim2=2).sum(dim=1)
    tr2 = (S * S).sum(dim=(1, 2))
    rho = ((1 - 2 / d) * tr2 + tr * tr) / ((n + 1 - 2 / d) * (tr2 - tr * tr / d))
    rho = torch.clamp(rho, max=1.0)
    eye = torch.eye(d, dtype=S.dtype, device=S.device)
    return (1 - rho)[:, None, None] * S + (rho * tr / d)[:, None, None] * eye


class ClassStatisticsAccumulator:
    """Class statistics built from batches: running count, mean and centred sum M2 = sum (x - mu)(x - mu)^T per class,
    merged batch by batch with the pairwise update of Chan, Golub and LeVeque (no raw second moments: sum x x^T - n mu mu^T
    cancels in float32).  ``update`` is native on the GPU (sqfa_class_moments_update) and the same formulas in torch on the
    CPU; ``merge`` joins the partial statistics of several loaders or ranks; ``finalize`` returns what
    ``class_statistics`` returns, and after one ``update`` with all the data equals it to rounding."""

    def __init__(self, n_classes, n_dim, dtype=torch.float32, device=None):
        if n_classes < 1 or n_dim < 1:
            raise ValueError("n_classes and n_dim must be positive")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("ClassStatisticsAccumulator supports float32 and float64")
        self.n_classes, self.n_dim, self.dtype = int(n_classes), int(n_dim), dtype
        self.device = torch.device("cpu" if device is None else device)
        self._counts = torch.zeros(self.n_classes, dtype=torch.float64, device=self.device)
        self._means = torch.zeros(self.n_classes, self.n_dim, dtype=dtype, device=self.device)
        self._m2 = torch.zeros(self.n_classes, self.n_dim, self.n_dim, dtype=dtype, device=self.device)

    @property
    def counts(self):
        """Points seen per class (int64)."""
        return self._counts.round().long()

    def update(self, points, labels):
        """Merge a batch: points (n, n_dim), labels (n) in 0..n_classes-1 (float labels accepted, as class_statistics)."""
        points = points.to(device=self.device, dtype=self.dtype)
        labels = labels.to(self.device).long()
        if points.dim() != 2 or points.shape[1] != self.n_dim or labels.shape != points.shape[:1]:
            raise ValueError("points must be (n, n_dim) and labels (n)")
        if labels.numel() == 0:
            return self
        if int(labels.min()) < 0 or int(labels.max()) >= self.n_classes:
            raise ValueError(f"labels must lie in 0..{self.n_classes - 1}")
        if points.is_cuda:
            from . import _native
            order, class_start = _native.grouped_rows(labels, self.n_classes)
            _native.class_moments_update(points, order, class_start, self.n_classes, self._counts, self._means, self._m2)
            return self
        order = torch.sort(labels, stable=True).indices
        present, sizes = torch.unique_consecutive(labels[order], return_counts=True)
        pos = 0
        for c, n_b in zip(present.tolist(), sizes.tolist()):
            rows = points[order[pos:pos + n_b]]
            pos += n_b
            mean_b = rows.double().sum(dim=0).div(n_b).to(self.dtype)
            centred = rows - mean_b
            self._merge_class(c, float(n_b), mean_b, centred.T @ centred)
        return self

    def _merge_class(self, c, n_b, mean_b, m2_b):
        n_a = float(self._counts[c])
        if n_a == 0:
            self._means[c] = mean_b
            self._m2[c] += m2_b
        else:
            delta = mean_b - self._means[c]
            self._m2[c] += m2_b + (n_a * n_b / (n_a + n_b)) * (delta[:, None] * delta[None, :])
            self._means[c] += delta * (n_b / (n_a + n_b))
        self._counts[c] = n_a + n_b

    def merge(self, other):
        """Merge another accumulator's statistics into this one (elementwise over the classes)."""
        if (other.n_classes, other.n_dim, other.dtype) != (self.n_classes, self.n_dim, self.dtype):
            raise ValueError("accumulators must agree in n_classes, n_dim and dtype")
        n_a, n_b = self._counts, other._counts.to(self.device)
        mean_b, m2_b = other._means.to(self.device), other._m2.to(self.device)
        n = n_a + n_b
        safe = n.clamp(min=1.0)
        delta = torch.where((n_a > 0)[:, None], mean_b - self._means, torch.zeros_like(mean_b))
        w = (n_a * n_b / safe).to(self.dtype)
        self._m2 += m2_b + w[:, None, None] * (delta[:, :, None] * delta[:, None, :])
        moved = self._means + delta * (n_b / safe).to(self.dtype)[:, None]
        self._means = torch.where((n_b > 0)[:, None], torch.where((n_a > 0)[:, None], moved, mean_b), self._means)
        self._counts = n
        return self

    def finalize(self, estimator="empirical"):
        """{'means', 'covariances', 'second_moments'} as class_statistics returns them; a class never seen gives NaN."""
        if estimator not in ("empirical", "oas"):
            raise ValueError("estimator must be 'empirical' or 'oas'")
        nan = torch.full((), float("nan"), dtype=self.dtype, device=self.device)
        means = torch.where((self._counts > 0)[:, None], self._means, nan)
        if self._m2.is_cuda:
            from . import _native
            code = _native.COV_OAS if estimator == "oas" else _native.COV_EMPIRICAL
            covs, second = _native.class_moments_finalize(self._counts, means, self._m2, code, True)
            return {"means": means, "covariances": covs, "second_moments": second}
        n = self._counts.to(self.dtype)
        covs = torch.where((self._counts > 0)[:, None, None], self._m2 / (n - 1)[:, None, None], nan)
        if estimator == "oas":
            covs = _oas_shrink(covs, n)
        second = covs + means[:, :, None] * means[:, None, :]
        return {"means": means, "covariances": covs, "second_moments": second}


class ClassPoints:
    """Labelled points kept as the statistics of a fit: the closure then computes the class moments of the PROJECTED
    points,  F cov_c F^T = cov(F x | c)  and  F mu_c = mean(F x | c)  (empirical estimator), reading the (N,D) points once
    forward and once backward instead of (C,D,D) statistics that may be many times larger -- or not fit at all.

    Holds ``points`` as given (no sorted copy), ``order`` (the indices of a stable sort of the labels), ``class_start``
    (C+1), ``row_class`` (the sorted labels), ``means`` (C,D), ``counts`` (C), ``n_classes``, ``n_dim``.  The class count
    is the only host read (none when ``n_classes`` is given).  An empty class has NaN means and feature moments, a class
    of one point a NaN covariance, as ``class_statistics`` gives them.  float32 / float64 points on the GPU go through the
    native kernels (sqfa_class_means, sqfa_class_feature_moments); CPU tensors, other dtypes, more than 64 filters and
    NATIVE_CLASS_POINTS = False evaluate the same formulas as a torch expression.

    ``estimator="oas"`` shrinks every class covariance as ``class_statistics(estimator="oas")`` does, still without forming
    it:  OAS(S_c) = keep_c S_c + shift_c I  with keep_c = 1 - rho_c and shift_c = rho_c tr S_c / D, so that
    F OAS(S_c) F^T = keep_c cov(F x | c) + shift_c F F^T.  The coefficients are measured once, here: ``shrink_keep`` and
    ``shrink_shift`` (C, the points' dtype) and ``shrinkage`` (rho, float64), NaN for a class below two points; all three
    are None for "empirical".  Natively that is one pass over the points (sqfa_class_shrinkage: the SYRK of the dense OAS
    statistics without its stores, the same bits of keep and shift); the fallback takes one class at a time and the Gram
    of the centred rows on their smaller side."""

    def __init__(self, points, labels, n_classes=None, estimator="empirical"):
        if estimator not in ("empirical", "oas"):
            raise ValueError("estimator must be 'empirical' or 'oas'")
        if not torch.is_tensor(points) or points.dim() != 2 or not points.is_floating_point():
            raise TypeError("points must be a floating-point tensor of shape (n_points, n_dim)")
        labels = torch.as_tensor(labels).to(points.device).long()   # float labels too, as class_statistics
        if labels.shape != points.shape[:1]:
            raise ValueError("labels must have shape (n_points,)")
        if labels.numel() == 0:
            raise ValueError("ClassPoints needs at least one point")
        C = int(labels.max()) + 1 if n_classes is None else int(n_classes)
        if C < 1:
            raise ValueError("n_classes must be positive")
        self.points = points.detach().contiguous()
        self.labels = labels
        self.n_classes, self.n_dim = C, points.shape[1]
        self.counts = torch.bincount(labels, minlength=C)   # refuses negative labels itself
        if self.counts.shape[0] != C:
            raise ValueError(f"labels must lie in 0..{C - 1}")
        self.order = torch.sort(labels, stable=True).indices
        self.class_start = torch.zeros(C + 1, dtype=torch.int64, device=labels.device)
        self.class_start[1:] = torch.cumsum(self.counts, 0)
        self.row_class = labels[self.order]
        if NATIVE_CLASS_POINTS and _native_applies(self.points):
            from . import _native
            self.means = _native.class_means(self.points, self.order, self.class_start, C)
        else:
            sums = torch.zeros(C, self.n_dim, dtype=torch.float64, device=points.device)
            sums.index_add_(0, labels, self.points.double())
            self.means = (sums / self.counts.double()[:, None]).to(points.dtype)   # 0/0 = NaN for an empty class
        self.estimator = estimator
        self.shrink_keep = self.shrink_shift = self.shrinkage = None
        if estimator == "oas":
            if NATIVE_CLASS_POINTS and _native_applies(self.points):
                from . import _native
                self.shrink_keep, self.shrink_shift, self.shrinkage = _native.class_shrinkage(
                    self.points, self.order, self.class_start, self.means, C)
            else:
                self.shrink_keep, self.shrink_shift, self.shrinkage = self._torch_shrinkage()

    def _torch_shrinkage(self):
        """(keep, shift, rho) of the OAS shrinkage, one class at a time: S in the dtype through the Gram of the centred rows
        on their smaller side (||Z^T Z||_F = ||Z Z^T||_F and the traces agree), tr S and sum S o S in double, rho as
        oas_covariance.  Nothing of size (C,D,D); (D,D) only for a class of more than D points."""
        C, d = self.n_classes, self.n_dim
        rho = torch.full((C,), float("nan"), dtype=torch.float64, device=self.points.device)
        tr = torch.full_like(rho, float("nan"))
        sizes, starts = self.counts.tolist(), self.class_start.tolist()
        for c, n in enumerate(sizes):
            if n < 2:
                continue
            Z = self.points[self.order[starts[c]:starts[c] + n]] - self.means[c]
            S = ((Z @ Z.T) if n <= d else (Z.T @ Z)) / (n - 1)
            t = torch.diagonal(S).double().sum()
            t2 = (S.double() ** 2).sum()
            r = ((1 - 2 / d) * t2 + t * t) / ((n + 1 - 2 / d) * (t2 - t * t / d))   # 0/0 = NaN stays NaN under the clamp
            rho[c], tr[c] = torch.clamp(r, max=1.0), t
        return (1 - rho).to(self.points.dtype), (rho * tr / d).to(self.points.dtype), rho

    @property
    def dtype(self):
        return self.points.dtype

    @property
    def device(self):
        return self.points.device

    def feature_statistics(self, filters, second_moments=False, noise=0.0):
        """{'means' (C,K), 'covariances' (C,K,K)[, 'second_moments' (C,K,K)]} of the projected points, differentiable in
        `filters` (K,D); `noise` is added to the diagonal of the matrices."""
        if NATIVE_CLASS_POINTS and _native_applies(self.points):
            from . import _native
            if _native.class_feature_moments_supported(self.points, filters):
                out = _native.ClassFeatureMoments.apply(filters, self, bool(second_moments), float(noise))
                stats = {"means": out[0], "covariances": out[1]}
                if second_moments:
                    stats["second_moments"] = out[2]
                return stats
        return self._torch_feature_statistics(filters, second_moments, noise)

    # rows of outer products z z^T formed at a time by the torch expression
    _OUTER_ELEMENTS = 1 << 24

    def _torch_feature_statistics(self, filters, second_moments, noise):
        """The same formulas in torch: gather the class means, centre in D-space, project, index_add_ the outer products."""
        dtype = torch.promote_types(self.points.dtype, filters.dtype)
        F = filters.to(dtype)
        K, C = F.shape[0], self.n_classes
        means = self.means.to(dtype)
        centred = self.points.to(dtype) - means[self.labels]
        z = centred @ F.T
        gram = torch.zeros(C, K, K, dtype=dtype, device=z.device)
        step = max(1, self._OUTER_ELEMENTS // (K * K))
        for r0 in range(0, z.shape[0], step):
            zb = z[r0:r0 + step]
            gram = torch.index_add(gram, 0, self.labels[r0:r0 + step], zb[:, :, None] * zb[:, None, :])
        nan = torch.full((), float("nan"), dtype=dtype, device=z.device)
        # NaN where class_statistics has it (no covariance below two points, no mean of no point), placed by `where` so that
        # the gradient of the other classes stays finite
        denom = (self.counts - 1).clamp(min=1).to(dtype)
        full = (self.counts >= 2)[:, None, None]
        cov = gram / denom[:, None, None]
        if self.shrink_keep is not None:   # keep_c cov(F x | c) + shift_c F F^T; the NaN coefficients of the classes
            # below two points are replaced before the product, so that no gradient passes through them
            zero = torch.zeros((), dtype=dtype, device=z.device)
            keep = torch.where(full, self.shrink_keep.to(dtype)[:, None, None], zero)
            shift = torch.where(full, self.shrink_shift.to(dtype)[:, None, None], zero)
            cov = keep * cov + shift * (F @ F.T)
        cov = torch.where(full, cov, nan)
        if noise:
            cov = cov + noise * torch.eye(K, dtype=dtype, device=z.device)
        present = (self.counts > 0)[:, None]
        m = torch.where(present, torch.where(present, means, torch.zeros_like(means)) @ F.T, nan)
        stats = {"means": m, "covariances": cov}
        if second_moments:
            stats["second_moments"] = cov + m[:, :, None] * m[:, None, :]
        return stats

    def class_statistics(self, estimator=None):
        """The dense {'means', 'covariances', 'second_moments'} of the same points (for comparison: (C,D,D) tensors);
        `estimator` defaults to this object's own."""
        if estimator is None:
            estimator = self.estimator
        stats = class_statistics(self.points, self.labels, estimator=estimator)
        missing = self.n_classes - stats["means"].shape[0]   # classes beyond the largest label: empty
        if missing > 0:
            stats = {k: torch.cat([v, v.new_full((missing,) + tuple(v.shape[1:]), float("nan"))]) for k, v in stats.items()}
        return stats


def _batched_moments(sorted_points, starts, counts, n_max, estimator):
    """Mean and covariance of G classes stored contiguously in `sorted_points` (class g occupies
    rows starts[g] .. starts[g]+counts[g]), as one zero-padded (G, n_max, D) batch."""
    d = sorted_points.shape[-1]
    dtype = sorted_points.dtype
    r = torch.arange(n_max, device=sorted_points.device)
    mask = r[None, :] < counts[:, None]                                   # (G, n_max)
    idx = starts[:, None] + torch.minimum(r[None, :], (counts[:, None] - 1).clamp(min=0))
    idx = idx.clamp(max=sorted_points.shape[0] - 1)
    keep = mask[:, :, None].to(dtype)
    batch = sorted_points[idx].mul_(keep)                                 # (G, n_max, D), zero padded
    n = counts.to(dtype)
    mean = batch.sum(dim=1) / n[:, None]
    centred = batch.sub_(mean[:, None, :]).mul_(keep)                     # in place: padding stays zero
    S = torch.bmm(centred.transpose(1, 2), centred) / (n - 1)[:, None, None]
    if estimator == "oas":
        # Chen et al. 2010, as oas_covariance below, per class
        tr = torch.diagonal(S, dim1=1, dim2=2).sum(dim=1)
        tr2 = (S * S).sum(dim=(1, 2))
        rho = ((1 - 2 / d) * tr2 + tr * tr) / ((n + 1 - 2 / d) * (tr2 - tr * tr / d))
        rho = torch.clamp(rho, max=1.0)
        eye = torch.eye(d, dtype=dtype, device=S.device)
        S = (1 - rho)[:, None, None] * S + (rho * tr / d)[:, None, None] * eye
    return mean, S


def pca(points, n_components=None):
    """Leading principal directions as rows, by descending variance (reference: statistics.py:127-160)."""
    n, d = points.shape
    if n_components is None:
        n_components = min(n, d)
    if n_components > d:
        raise ValueError("n_components must be less than or equal to n_dim.")
    cov = sample_covariance(points)
    # One-off (D,D) eigh, run through LAPACK on the host like the reference: eigenvectors are
    # only defined up to sign (and up to a rotation inside degenerate eigenspaces), and
    # rocSOLVER makes different choices, which would start every fit from a different point.
    # LAPACK with one thread per CPU this process may actually use: with every hardware thread
    # of a large host under a small cgroup quota the (3072, 3072) case takes 5 s instead of ~2.
    saved = torch.get_num_threads()
    torch.set_num_threads(min(saved, usable_cpus()))
    try:
        _, vecs = torch.linalg.eigh(cov.cpu())
    finally:
        torch.set_num_threads(saved)
    return vecs[:, d - n_components:].flip(1).T.to(cov.device)


def usable_cpus():
    """CPUs this process is entitled to: the cgroup v2 quota when there is one, else the affinity mask."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def pca_from_scatter(scatters, n_components=None):
    """PCA initialisation from class scatter matrices.  NOTE (reference quirk, SURVEY.md Q1,
    statistics.py:189-190, pinned by its tests/test_training.py:184-188): the mean scatter
    matrix is handed to ``pca`` *as if it were a data matrix*, so the result is the PCA of
    its rows, not its leading eigenvectors.  Reproduced on purpose: it is the starting point
    of every ``fit_pca(data_statistics=...)`` trajectory."""
    d = scatters.shape[-1]
    if n_components is None:
        n_components = d
    if n_components > d:
        raise ValueError("n_components must be less than or equal to n_dim.")
    return pca(scatters.mean(dim=0), n_components=n_components)
