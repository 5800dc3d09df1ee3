"""float64 torch oracle of the Gaussian pair distances (sqfa_gauss_pair_terms, sqfa_gauss_pairwise_loss): the definitions,
written the way the reference forms them -- the mean covariance Sbar = (Sigma_i + Sigma_j)/2 of every pair materialised,
torch.linalg.solve and torch.logdet on it, gradients by autograd.

    Q_ij  = (mu_i - mu_j)^T Sbar_ij^-1 (mu_i - mu_j)                      mahalanobis_sq (kind 2); sqrt(Q + eps): kind 3
    Bh_ij = Q_ij / 8 + (logdet Sbar_ij - (logdet Sigma_i + logdet Sigma_j) / 2) / 2      bhattacharyya (kind 0)
    He_ij = sqrt(1 - exp(-Bh_ij) + eps)                                   hellinger (kind 1)

Pinned to the reference's recorded outputs (goldens G5b and G8) by tests/test_gauss_oracle.py, without a GPU.  `dtype`
evaluates the same expression in another precision: the float32 run is the yardstick of the float32 tolerances."""
import torch

EPS = 1e-6


def _rows_D(mu_r, cov_r, mu, cov, kind, clamp=False):
    """(R,C) distances of the classes (mu_r, cov_r) to all classes (mu, cov); the log-determinant term of a class with
    itself is not special-cased here: callers mask the diagonal.  clamp: a negative log-determinant term counts as 0,
    with derivative 0 (the yardstick of tests/test_gpu_close_classes.py: finite where the plain expression is NaN)."""
    Sbar = 0.5 * (cov_r[:, None] + cov[None])
    delta = mu_r[:, None] - mu[None]
    sol = torch.linalg.solve(Sbar, delta.unsqueeze(-1)).squeeze(-1)
    Q = (delta * sol).sum(-1)
    if kind == 2:
        return Q
    if kind == 3:
        return torch.sqrt(Q + EPS)
    det = 0.5 * (torch.logdet(Sbar) - 0.5 * (torch.logdet(cov_r)[:, None] + torch.logdet(cov)[None]))
    Bh = Q / 8 + (torch.where(det < 0, torch.zeros_like(det), det) if clamp else det)
    return Bh if kind == 0 else torch.sqrt(1 - torch.exp(-Bh) + EPS)


def _full_expression(mu, cov, kind, weight, dtype=torch.float64, clamp=False, W=None):
    """loss = weight * sum_{i>j} D_ij (W (C,C): sum_{i>j} W_ij D_ij), its gradients, and D with the reference's diagonal."""
    mu = mu.detach().to(dtype).requires_grad_(True)
    cov = cov.detach().to(dtype).requires_grad_(True)
    D = _rows_D(mu, cov, mu, cov, kind, clamp)
    C = mu.shape[0]
    rows, cols = torch.tril_indices(C, C, offset=-1)
    loss = weight * D[rows, cols].sum() if W is None else (W.to(dtype)[rows, cols] * D[rows, cols]).sum()
    gmu, gcov = torch.autograd.grad(loss, (mu, cov))
    D = D.detach().clone()
    D.fill_diagonal_(0.0 if kind in (0, 2) else EPS ** 0.5)
    return loss.detach(), gmu, gcov, D


def pair_terms(muA, covA, muB, covB, dtype=torch.float64):
    """Q (nA,nB) and LD (nA,nB) = logdet Sbar of every pair of an A class with a B class.  Differentiable with respect
    to whichever inputs require a gradient (inputs of another dtype are converted first)."""
    muA, covA, muB, covB = (t.to(dtype) for t in (muA, covA, muB, covB))
    Sbar = 0.5 * (covA[:, None] + covB[None])
    delta = muA[:, None] - muB[None]
    sol = torch.linalg.solve(Sbar, delta.unsqueeze(-1)).squeeze(-1)
    return (delta * sol).sum(-1), torch.logdet(Sbar)


def inputs(C, K, seed):
    """(C,K) means and (C,K,K) covariances, float64 on the CPU: classes that share most of their covariance
    (0.7 common + 0.3 own, both Wishart with 4K degrees of freedom) and means scaled by 1/sqrt(K), so that the
    distances keep their order of magnitude at every K and Hellinger stays away from saturation."""
    g = torch.Generator().manual_seed(seed)
    common = torch.randn(K, 4 * K, generator=g, dtype=torch.float64)
    common = common @ common.T / (4 * K)
    A = torch.randn(C, K, 4 * K, generator=g, dtype=torch.float64)
    cov = 0.7 * common + 0.3 * (A @ A.transpose(1, 2) / (4 * K))
    cov = 0.5 * (cov + cov.transpose(1, 2))   # bitwise symmetric: the kernels read the lower triangle only
    mu =(1.2 / K ** 0.5) * torch.randn(C, K, generator=g, dtype=torch.float64)
    return mu, cov
