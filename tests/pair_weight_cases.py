"""Test infrastructure of the per-pair class weights (fit(pair_weights=...)): the seeded weight generator every numeric test
uses, and the float64 weighted loss the closures are compared with."""
import torch


def make_weights(C, seed):
    """(C,C) float64 weights: symmetric, entries uniform in [0.25, 1.75], about 20 % of the pairs set exactly to zero, no
    class whose pairs are all zero (the zero pattern is drawn again, from the same generator, until that holds)."""
    g = torch.Generator().manual_seed(seed)
    U = 0.25 + 1.5 * torch.rand(C, C, generator=g, dtype=torch.float64)
    W = torch.tril(U, -1)
    for _ in range(1000):
        keep = torch.tril((torch.rand(C, C, generator=g) >= 0.2).to(torch.float64), -1)
        M = keep + keep.T
        if bool((M.sum(dim=1) > 0).all()):
            break
    W = W * keep
    W = W + W.T
    check_weights(W)
    return W


def check_weights(W):
    """The properties the issue asks of the test weights, asserted on the inputs."""
    C = W.shape[0]
    off = W[~torch.eye(C, dtype=torch.bool)]
    assert torch.equal(W, W.T)
    assert bool(((off == 0) | ((off >= 0.25) & (off <= 1.75))).all())
    assert bool((W.sum(dim=1) - W.diagonal() > 0).all()), "a class with all-zero weights"


def single_pair(C, a, b):
    """Weight 1 on the pair (a, b), a > b, and 0 on every other pair."""
    assert a > b
    W = torch.zeros(C, C, dtype=torch.float64)
    W[a, b] = W[b, a] = 1.0
    return W


def normalized(W):
    """Wn = -W / sum_{i>j} W with a zero diagonal (what _native.normalized_pair_weights returns), float64."""
    Wn = -W.double() / torch.tril(W.double(), -1).sum()
    Wn.fill_diagonal_(0.0)
    return Wn


def weighted_loss(W, D):
    """-sum_{i>j} W_ij D_ij / sum_{i>j} W_ij"""
    W = W.to(D.dtype).to(D.device)
    return -(torch.tril(W * D, -1)).sum() / torch.tril(W, -1).sum()
