"""CPU: the variance a full-covariance gradient step takes from the J' panel, var = sigma^2 + colsum(K o R A) with R = W^T (Lq Lq^T - I)
and A = W K, is as accurate as the W-form var - sum A^2 + sum (Lq^T A)^2 of the value-only and predict passes: against an 80-bit
evaluation, within 10x of the W-form error plus 1e-12 -- the rule and the cases of tests/test_cpu_rform_variance.py."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import rform_accuracy as ra  # noqa: E402
import zigp_oracle as o  # noqa: E402

CASES = ra.cases(full=False)
LD = np.longdouble


def _chol_ld(K):
    """Cholesky factor in 80-bit arithmetic (column by column)"""
    K = K.astype(LD)
    M = K.shape[0]
    L = np.zeros((M, M), dtype=LD)
    for j in range(M):
        L[j, j] = np.sqrt(K[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < M:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_lower_ld(L, B):
    X = np.zeros_like(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def variance_errors(Z, ellv, var, s, X, jit=1e-6, npts=48, seed=0):
    M = Z.shape[0]
    Lq = np.diag(s) + (0.1 / np.sqrt(M)) * np.tril(np.random.RandomState(seed).randn(M, M), -1)
    Kuu = o.rbf_K(Z, Z, ellv, var) + jit * np.eye(M)
    cond = np.linalg.cond(Kuu)
    L = sl.cholesky(Kuu, lower=True)
    Kuf = o.rbf_K(Z, X[:npts], ellv, var)
    W = sl.solve_triangular(L, np.eye(M), lower=True)           # the explicit inverse, as the engine forms it
    A = W @ Kuf
    var_w = var - np.sum(A ** 2, 0) + np.sum((Lq.T @ A) ** 2, 0)
    Rt = (Lq @ Lq.T - np.eye(M)) @ W                            # R^T = (T - I) W
    var_r = var + np.sum(Kuf * (Rt.T @ A), 0)
    Al = _solve_lower_ld(_chol_ld(Kuu), Kuf.astype(LD))
    var_t = LD(var) - np.sum(Al * Al, 0) + np.sum((Lq.astype(LD).T @ Al) ** 2, 0)
    ew = float(np.max(np.abs(var_w - var_t) / np.abs(var_t)))
    er = float(np.max(np.abs(var_r - var_t) / np.abs(var_t)))
    return cond, ew, er


@pytest.mark.parametrize('case', CASES, ids=[c[0].replace(' ', '_').replace('/', '-') for c in CASES])
def test_full_rform_variance_matches_wform_accuracy(case):
    name, Z, ellv, var, s, X = case
    cond, ew, er = variance_errors(Z, ellv, var, s, X)
    print('%s cond %.2e W-form %.2e R-form %.2e' % (name, cond, ew, er))
    assert er <= 10.0 * ew + 1e-12, (name, cond, ew, er)
