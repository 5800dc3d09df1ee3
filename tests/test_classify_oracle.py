"""Pins tests/classify_oracle.py against scikit-learn's QuadraticDiscriminantAnalysis: fed sklearn's own means_, covariance_
and priors_, the oracle must predict the same classes and give the same log posteriors."""
import numpy as np
import pytest

import classify_oracle

discriminant_analysis = pytest.importorskip("sklearn.discriminant_analysis")


@pytest.mark.parametrize("C,K,N,sep", [(2, 1, 80, 1.0), (3, 3, 150, 1.0), (5, 8, 400, 0.0), (7, 16, 700, 1.0)])
def test_oracle_agrees_with_sklearn_qda(C, K, N, sep):
    Z, labels, _, _ = classify_oracle.problem(C, K, N, sep, seed=C + K)
    labels = labels.copy()
    labels[: N // 4] = 0   # unequal class sizes: non-uniform priors_
    qda = discriminant_analysis.QuadraticDiscriminantAnalysis(store_covariance=True).fit(Z, labels)
    rng = np.random.default_rng(1)
    Zt = Z[rng.permutation(N)[: N // 2]] + 0.1 * rng.standard_normal((N // 2, K))
    S = classify_oracle.scores(Zt, qda.means_, np.stack(qda.covariance_), qda.priors_)
    assert np.array_equal(classify_oracle.predict(S), qda.predict(Zt))
    log_post = S - classify_oracle.log_evidence(S)[:, None]
    assert np.abs(log_post - qda.predict_log_proba(Zt)).max() <= 1e-10
