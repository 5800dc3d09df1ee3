"""Float64 oracle of the Jeffreys divergence for the tests: the TEXTBOOK form

    J_ij = 1/2 [tr(P_j Sigma_i) + tr(P_i Sigma_j) - 2m + delta^T (P_i + P_j) delta],   P = inv(Sigma), delta = mu_i - mu_j

written with torch (a restatement of the definition, not of the package's explicit-difference expression), the closure
loss sum_{i>j} w_ij D_ij on top of it, and its gradients by autograd.  Inputs of the family the tests use:
Sigma = A A^T / (2m) + 0.1 I, means 0.3 randn, fixed seeds."""
import torch

EPS = 1e-6


def make_classes(n, m, seed, dtype=torch.float64):
    """(mu (n,m), cov (n,m,m)): well-conditioned classes, exactly symmetric covariances."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(n, m, 2 * m, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2) / (2 * m) + 0.1 * torch.eye(m, dtype=torch.float64)
    cov = 0.5 * (cov + cov.transpose(1, 2))
    mu = 0.3 * torch.randn(n, m, generator=g, dtype=torch.float64)
    return mu.to(dtype), cov.to(dtype)


def make_weights(n, seed, dtype=torch.float64):
    """Symmetric random (n,n) weights in [0.5, 1.5] with two zero entries (when the class count allows)."""
    g = torch.Generator().manual_seed(seed)
    W = 0.5 + torch.rand(n, n, generator=g, dtype=torch.float64)
    W = 0.5 * (W + W.t())
    if n >= 3:
        W[1, 0] = W[0, 1] = 0.0
        W[n - 1, 1] = W[1, n - 1] = 0.0
    return W.to(dtype)


def textbook(muA, covA, muB, covB):
    """(nA,nB) Jeffreys divergences in the textbook form; mu* None: zero means."""
    PA, PB = torch.linalg.inv(covA), torch.linalg.inv(covB)
    m = covA.shape[-1]
    t1 = torch.einsum("bkl,alk->ab", PB, covA)      # tr(P_j Sigma_i)
    t2 = torch.einsum("akl,blk->ab", PA, covB)      # tr(P_i Sigma_j)
    J = 0.5 * (t1 + t2 - 2 * m)
    if muA is not None:
        delta = muA[:, None] - muB[None]
        J = J + 0.5 * (torch.einsum("abk,akl,abl->ab", delta, PA, delta) + torch.einsum("abk,bkl,abl->ab", delta, PB, delta))
    return J


def loss_and_gradients(mu, cov, sqrt_mode, weight, W=None, fn=None):
    """dict(loss, dist, gmu, gcov) of sum_{i>j} w_ij D_ij for classes (mu or None, cov): dist the full unweighted (n,n)
    matrix, the diagonal 0 or sqrt(eps); gcov symmetrised (the gradient wrt a symmetric matrix).  `fn(muA, covA, muB,
    covB) -> J` selects another expression of J (default: the textbook form)."""
    fn = textbook if fn is None else fn
    n = cov.shape[0]
    cov_v = cov.clone().requires_grad_(True)
    mu_v = mu.clone().requires_grad_(True) if mu is not None else None
    J = fn(mu_v, cov_v, mu_v, cov_v)
    J = J - torch.diag(torch.diagonal(J))           # J_ii = 0 by definition (the textbook traces leave rounding there)
    D = torch.sqrt(J + EPS) if sqrt_mode else J
    r, c = torch.tril_indices(n, n, offset=-1)
    w = W[r, c] if W is not None else weight
    loss = (w * D[r, c]).sum()
    grads = torch.autograd.grad(loss, [cov_v] + ([mu_v] if mu is not None else []))
    gcov = 0.5 * (grads[0] + grads[0].transpose(1, 2))
    return {"loss": loss.detach(), "dist": D.detach(), "gmu": grads[1] if mu is not None else None, "gcov": gcov}
