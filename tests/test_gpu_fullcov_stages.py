"""The M x M stage of a full-covariance call (zigp_set_q_full) for one latent, without a chunk loop, against NumPy (include/zigp_diag.h
zigp_test_q_full_forward / zigp_test_q_full_dlq, which run the functions the call runs: k_lq_stage, k_kl_white_full, the split-K
products T - I = Lq Lq^T - I and R^T = (T - I) W, and the dLq assembly tril(2 C1 Lq) - (tril(Lq) - diag(1 / Lq_ii))).

M = 16 (one block, 112 padded rows), 150 (two blocks), 300 (three blocks, every split-K range occurs).  Bound for T - I, R^T and dLq:
1e-12 relative to the largest entry (fp64 products of O(1) entries with inner length <= 300: <= 300 eps ~ 7e-14 in the worst case); the
KL to 1e-13 relative (a fixed-order sum of M (M + 1) / 2 + 2 M terms).  The input carries garbage above the diagonal and a few negative
diagonal entries; outputs in the padding never reach the caller."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SIZES = [16, 150, 300]


def _operands(M, seed):
    rs = np.random.RandomState(500 + seed)
    W = np.tril(rs.randn(M, M)) / np.sqrt(M) + np.eye(M)
    Lq = np.diag(0.3 + rs.rand(M)) + (0.1 / np.sqrt(M)) * np.tril(rs.randn(M, M), -1)
    neg = rs.choice(M, size=3, replace=False)
    Lq[neg, neg] *= -1.0
    raw = Lq + np.triu(5.0 + 50.0 * rs.randn(M, M), 1)          # what the caller passes: the strict upper triangle must be ignored
    B = rs.randn(M, M + 7)
    C1 = B @ B.T / M                                             # symmetric, like A G A^T
    return W, Lq, raw, rs.randn(M), C1


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize('M', SIZES)
def test_forward_stage(engine, M):
    W, Lq, raw, u, C1 = _operands(M, M)
    TmI, Rt, kl = engine.test_q_full_forward(W, raw, u)
    T_ref = Lq @ Lq.T - np.eye(M)
    Rt_ref = T_ref @ W
    kl_ref = 0.5 * (np.sum(u * u) + np.sum(Lq * Lq) - M - np.sum(np.log(np.diagonal(Lq) ** 2)))
    e_t, e_r, e_k = _rel(TmI, T_ref), _rel(Rt, Rt_ref), abs(kl - kl_ref) / abs(kl_ref)
    print('M=%d T - I rel %.2e, R^T rel %.2e, KL rel %.2e' % (M, e_t, e_r, e_k))
    assert np.all(np.isfinite(TmI)) and np.all(np.isfinite(Rt))
    assert e_t <= 1e-12 and e_r <= 1e-12 and e_k <= 1e-13
    assert np.array_equal(TmI, TmI.T)                            # both triangles from the same products in the same order
    again = engine.test_q_full_forward(W, raw, u)
    assert np.array_equal(again[0], TmI) and np.array_equal(again[1], Rt) and again[2] == kl


@pytest.mark.parametrize('M', SIZES)
def test_dlq_stage(engine, M):
    W, Lq, raw, u, C1 = _operands(M, M + 1)
    for include_kl in (True, False):
        got = engine.test_q_full_dlq(C1, raw, include_kl=include_kl)
        ref = np.tril(2.0 * C1 @ Lq)
        if include_kl:
            ref -= Lq - np.diag(1.0 / np.diagonal(Lq))
        e = _rel(got, ref)
        print('M=%d include_kl=%d dLq rel %.2e' % (M, include_kl, e))
        assert np.all(np.triu(got, 1) == 0.0) and e <= 1e-12


def test_zero_diagonal_is_refused(engine):
    W, Lq, raw, u, C1 = _operands(16, 0)
    raw[5, 5] = 0.0
    with pytest.raises(ValueError, match='zero diagonal'):
        engine.test_q_full_forward(W, raw, u)
    with pytest.raises(ValueError, match='zero diagonal'):
        engine.test_q_full_dlq(C1, raw)
