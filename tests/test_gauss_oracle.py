"""The float64 oracle of the Gaussian pair distances (tests/gauss_oracle.py) against what the reference computed: golden
G8 (distances, closure loss and its gradients with respect to the feature statistics, four kinds, six cases) and golden
G5b (mahalanobis_sq = Q, self and cross batches).  No GPU: this is what lets the GPU tests of the kernel rows use the
oracle at shapes no golden records.  Bounds: the ones tests/test_gpu_gauss_closure.py puts on the same comparison."""
import pytest
import torch

import gauss_oracle
from conftest import load_golden, rel_err

G8 = load_golden("g8_gauss_closure.npz")
G8_CASES = [tuple(int(v) for v in c) for c in G8["cases"]]
G5B = load_golden("g5b_other_operators.npz")
G5B_CASES = [tuple(int(v) for v in c) for c in G5B["cases"]]
OPS = {"bhattacharyya": 0, "hellinger": 1, "mahalanobis_sq": 2, "mahalanobis": 3}


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("C,D,K", G8_CASES)
def test_full_expression_reproduces_golden_g8(C, D, K, op):
    key = f"C{C}_D{D}_K{K}"
    mu = torch.tensor(G8[f"{key}_fmu"], dtype=torch.float64)
    cov = torch.tensor(G8[f"{key}_fcov"], dtype=torch.float64)
    loss, gmu, gcov, Dm = gauss_oracle._full_expression(mu, cov, OPS[op], -1.0 / (C * (C - 1) // 2))
    assert rel_err(Dm, G8[f"{key}_{op}_D_f64"]) < 1e-10
    assert rel_err(loss, G8[f"{key}_{op}_loss_f64"]) < 1e-10
    assert rel_err(gmu, G8[f"{key}_{op}_gmu_f64"]) < 1e-7
    assert rel_err(gcov, G8[f"{key}_{op}_gcov_f64"]) < 1e-7


@pytest.mark.parametrize("nA,nB,K", G5B_CASES)
def test_pair_terms_reproduce_golden_g5b_mahalanobis_sq(nA, nB, K):
    key = f"A{nA}_B{nB}_K{K}"
    muA = torch.tensor(G5B[f"{key}_muA"], dtype=torch.float64)
    covA = torch.tensor(G5B[f"{key}_covA"], dtype=torch.float64)
    muB = torch.tensor(G5B[f"{key}_muB"], dtype=torch.float64) if nB else muA
    covB = torch.tensor(G5B[f"{key}_covB"], dtype=torch.float64) if nB else covA
    Q, LD = gauss_oracle.pair_terms(muA, covA, muB, covB)
    assert Q.dtype == LD.dtype == torch.float64 and Q.shape == LD.shape == (nA, nB or nA)
    ref = G5B[f"{key}_mahalanobis_sq_f64"]
    assert rel_err(Q.reshape(ref.shape), ref) < 1e-10
    # logdet of the pair (c, c) is logdet Sigma_c: the one value of LD with an independent expression
    if not nB:
        assert rel_err(LD.diagonal(), torch.linalg.slogdet(covA)[1]) < 1e-12


def test_inputs_are_seeded_and_well_conditioned():
    mu, cov = gauss_oracle.inputs(9, 7, 907)
    mu2, cov2 = gauss_oracle.inputs(9, 7, 907)
    assert torch.equal(mu, mu2) and torch.equal(cov, cov2)
    assert mu.shape == (9, 7) and cov.shape == (9, 7, 7) and mu.dtype == cov.dtype == torch.float64
    assert torch.equal(cov, cov.transpose(1, 2))
    assert torch.linalg.eigvalsh(cov).min() > 0
