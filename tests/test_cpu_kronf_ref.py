"""Pins of tests/kronf_ref.py (no GPU): the restatements the fused Kronecker tile kernels are held to in tests/test_gpu_kronf_stages.py
must themselves be right, by a check that shares nothing with them.

* backward(): L = sum_n gm mean + gv st + dq0 q0 + dq1 q1 is written in torch float64 as a function of (Alpha, S2, P0, P1, K0, K1) and
  differentiated by autograd.  dL/dAlpha, dL/dS2, dL/dP_p must be backward()'s dAl, dS2, dP_p (P_p a free matrix: the unsymmetrised
  E_p K_p^T), and (dL/dK_p . K_p) Psi_p its moment matrices -- with a symmetric P_p, as K_p^-1 is, since the kernel's
  dK_p = gm B_p + 2 dq_p A_p + P_p dA_p uses P_p^T K_p = A_p.  Agreement within the restatement's own 16 eps S.
* forward(): its rows give the oracle's kron_predict latent means and variances on a tests/kron_nd.py fixture.
* frag_image() against the index rule written out as loops, latent() against its definition, the exact-tier inputs of the GPU test
  give integer sums below 2^53 (so any summation order gives the same bits).
"""
import numpy as np
import pytest
import torch

import kron_nd
import kronf_ref as kr

EPS = kr.EPS


def _spd_inverse(Z, ell, var, jitter, rs):
    d = (Z[:, None, :] - Z[None, :, :]) / ell
    K = var * np.exp(-0.5 * (d * d).sum(2)) + jitter * np.eye(Z.shape[0])
    P = np.linalg.inv(K)
    return 0.5 * (P + P.T)


def _problem(grid, D, N, seed):
    rs = np.random.RandomState(seed)
    M = grid
    Z = [rs.rand(M[q], D[q]) * 4.0 for q in range(2)]
    ell = [0.6 + rs.rand(D[q]) for q in range(2)]
    var = [1.7, 0.8]
    P = [_spd_inverse(Z[q], ell[q], var[q], 1e-2, rs) for q in range(2)]
    U = rs.randn(M[0], M[1])
    S2 = np.square(0.5 + rs.rand(M[0], M[1]))
    Al = P[0] @ U @ P[1]
    X = rs.rand(N, D[0] + D[1]) * 4.0
    cot = rs.randn(4, N)
    zc = [0.5 * (Z[q].min(0) + Z[q].max(0)) for q in range(2)]
    return Z, ell, var, P, Al, S2, X, cot, zc


@pytest.mark.parametrize('D', [(2, 1), (1, 3)])
@pytest.mark.parametrize('grid', [(6, 5), (20, 9), (10, 100)])
def test_backward_is_the_gradient_of_the_forward_sum(grid, D):
    N = 150
    Z, ell, var, P, Al, S2, X, cot, zc = _problem(grid, D, N, 11 + grid[0] + 7 * D[1])
    part, _ = kr.forward(P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N)
    b = kr.backward(P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N, part, cot[0], cot[1], cot[2], cot[3], zc[0], zc[1])
    # the same L in torch, from the K tiles on (they are inputs here: no exponential inside the differentiated function)
    K = [kr.ktile(Z[0], ell[0], var[0], X[:, :D[0]]), kr.ktile(Z[1], ell[1], var[1], X[:, D[0]:])]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)
    tAl, tS2, tP0, tP1, tK0, tK1 = (t(a) for a in (Al, S2, P[0], P[1], K[0], K[1]))
    gm, gv, dq0, dq1 = (torch.tensor(c, dtype=torch.float64) for c in cot)
    A0, A1 = tP0 @ tK0, tP1 @ tK1
    q0, q1 = (tK0 * A0).sum(0), (tK1 * A1).sum(0)
    mean = (tK0 * (tAl @ tK1)).sum(0)
    st = (A0 * A0 * (tS2 @ (A1 * A1))).sum(0)
    np.testing.assert_array_equal(np.stack([q0.detach().numpy(), q1.detach().numpy(), mean.detach().numpy(), st.detach().numpy()]).shape, part.shape)
    L = (gm * mean + gv * st + dq0 * q0 + dq1 * q1).sum()
    L.backward()
    got = dict(dAl=tAl.grad.numpy(), dS2=tS2.grad.numpy(), dP0=tP0.grad.numpy(), dP1=tP1.grad.numpy())
    for p, (tK, Kp) in enumerate(((tK0, K[0]), (tK1, K[1]))):
        Xp = X[:, :D[0]] if p == 0 else X[:, D[0]:]
        got['Kr%d' % p] = (tK.grad.numpy() * Kp) @ kr.psi(Xp, zc[p])
    for k, (val, S) in b.items():
        assert val.shape == got[k].shape, k
        ratio = np.max(np.abs(val - got[k]) / (EPS * S))
        print('%s grid %s D %s: max |restatement - autograd| / (eps S) = %.2f' % (k, grid, D, ratio))
        assert ratio <= 16.0, (k, ratio)
    # the check has teeth: a moment matrix built from dq_p A_p instead of 2 dq_p A_p is far outside it
    A = [P[0] @ K[0], P[1] @ K[1]]
    wrong = b['Kr0'][0] - ((cot[2] * A[0]) * K[0]) @ kr.psi(X[:, :D[0]], zc[0])
    assert np.max(np.abs(wrong - got['Kr0']) / (EPS * b['Kr0'][1])) > 1e6


def test_forward_rows_are_the_oracles_latent_moments():
    name = 'd21-mix2'                       # f (10, 30), g (30, 10)
    X, Y, p = kron_nd.problem(name)
    ref = kron_nd.oracle_predict(name, 0.0)
    import zigp_oracle as o
    N = X.shape[0]
    for tag, (im, iv) in (('f', (3, 4)), ('g', (5, 6))):
        Z, ell, var = p['Z' + tag], p['ell_' + tag], [float(np.squeeze(v)) for v in p['var_' + tag]]
        P = [np.linalg.inv(o.rbf_K(Z[q], None, ell[q], var[q]) + kron_nd.JITTER * np.eye(Z[q].shape[0])) for q in range(2)]
        M0, M1 = Z[0].shape[0], Z[1].shape[0]
        U, S2 = p['u_%sm' % tag].reshape(M0, M1), np.square(p['u_%ss_sqrt' % tag]).reshape(M0, M1)
        Al = kr.latent(P[0], P[1], U)['Al'][0]
        part, S = kr.forward(P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N)
        mean, v = part[2], var[0] * var[1] - part[0] * part[1] + part[3]
        # the same factored algebra with the oracle's kernel function: rounding only
        mu2, vv2 = kron_nd._factored_with_oracle_inverse(X, p, tag, kron_nd.JITTER)
        assert kron_nd._relerr(mean, mu2) <= 1e-11 and kron_nd._relerr(v, vv2) <= 1e-11
        # the literal dense oracle: within the fixture's op-order floor (<= 1e-8, pinned by test_cpu_kron_nd.py)
        assert kron_nd._relerr(mean, ref[im]) <= 1e-8, kron_nd._relerr(mean, ref[im])
        assert kron_nd._relerr(v, ref[iv]) <= 1e-8, kron_nd._relerr(v, ref[iv])
        assert np.all(S >= np.abs(part))


@pytest.mark.parametrize('shape', [(16, 16), (32, 16), (16, 112), (32, 32)])
def test_frag_image_is_the_index_rule_of_kf_write_frag(shape):
    R, Cc = shape
    A = np.arange(R * Cc, dtype=np.float64).reshape(R, Cc)
    for transposed in (False, True):
        nbr, ksn = (Cc // 16, R // 4) if transposed else (R // 16, Cc // 4)
        F = np.empty(R * Cc)
        for idx in range(R * Cc):                       # kf_write_frag, line by line
            ln, blk = idx & 63, idx >> 6
            ks, rb = blk % ksn, blk // ksn
            row, k = 16 * rb + (ln & 15), 4 * ks + (ln >> 4)
            F[idx] = A[k, row] if transposed else A[row, k]
        np.testing.assert_array_equal(kr.frag_image(A, transposed), F)
        assert sorted(F) == sorted(A.reshape(-1))       # a permutation: every element exactly once
    np.testing.assert_array_equal(kr.frag_image(A, True), kr.frag_image(np.ascontiguousarray(A.T), False))


def test_latent_and_work_image():
    rs = np.random.RandomState(5)
    P0, P1, U = rs.randn(6, 6), rs.randn(5, 5), rs.randn(6, 5)
    lt = kr.latent(P0, P1, U)
    ld = kr.latent(P0, P1, U, dtype=np.longdouble)
    np.testing.assert_allclose(lt['Al'][0], np.einsum('ia,ab,bj->ij', P0, U, P1), rtol=0, atol=16 * EPS * np.max(lt['Al'][1]))
    for k in lt:
        assert np.all(np.abs(lt[k][0] - ld[k][0]) <= 4 * EPS * lt[k][1])
    b = {k: (rs.randn(*s), None) for k, s in (('dAl', (6, 5)), ('dS2', (6, 5)), ('dP0', (6, 6)), ('dP1', (5, 5)), ('Kr0', (6, 5)), ('Kr1', (5, 3)))}
    w = kr.work_image(b, (6, 5), (2, 1), (2, 2))
    assert w.size == 4 * 32 * 32 + 2 * 32 * 16                      # KF_W_TOTAL of csrc/zigp_kronf.hip
    sp = kr.work_split(w, (2, 2))
    for k in b:
        v = b[k][0]
        np.testing.assert_array_equal(sp[k][:v.shape[0], :v.shape[1]], v)
        assert np.count_nonzero(sp[k]) == v.size
    assert kr.work_image(b, (6, 5), (2, 1), (1, 7)).size == 3 * 16 * 112 + 112 * 112 + 16 * 16 + 112 * 16


EXACT_CASES = [((6, 5), None, (2, 1), 17, 0.0), ((6, 5), (20, 20), (2, 1), 1025, 0.0), ((32, 32), None, (1, 1), 33000, 0.0),
               ((16, 112), (9, 50), (1, 1), 8211, 0.0), ((10, 100), None, (7, 7), 1025, 0.0), ((17, 31), None, (3, 2), 1000, 0.0),
               ((20, 9), (9, 20), (2, 1), 1025, 0.25), ((10, 100), None, (2, 1), 1000, 0.25)]


@pytest.mark.parametrize('grid_f,grid_g,D,N,jitter', EXACT_CASES)
def test_exact_tier_inputs_give_integer_sums(grid_f, grid_g, D, N, jitter):
    """The exact tier of the GPU test rests on this: with its inputs every term of every sum over points is an integer (with the dyadic
    jitter: a multiple of 2^-24) and the sum of their absolute values stays below 2^53 units, so the sums have the same bits in any order
    and in any precision >= float64 -- and they are what the closed forms of kronf_ref.exact_problem say, which restate nothing of
    kronf_ref.backward (one scatter-add per sum)."""
    e = kr.exact_problem(grid_f, grid_g, D, N, jitter, seed=3)
    unit = 1.0 if jitter == 0.0 else 2.0 ** -24
    for L in e['lat']:
        for dtype in (np.float64, np.longdouble) if N <= 1025 else (np.float64,):      # (the long double products of the larger cases take 10+ s)
            part, Sp = kr.forward(*L['stage'], e['X'], N, dtype=dtype)
            b = kr.backward(*L['stage'], e['X'], N, part, *L['cot'], *L['zc'], dtype=dtype)
            np.testing.assert_array_equal(np.asarray(part, dtype=np.float64), L['part'])
            for k, (v, S) in b.items():
                v64 = np.asarray(v, dtype=np.float64)
                assert np.all(v64 / unit == np.rint(v64 / unit)), k
                assert float(np.max(S)) / unit < 2.0 ** 53, (k, float(np.max(S)))
                np.testing.assert_array_equal(v64, L['sums'][k])
        assert np.count_nonzero(L['sums']['dAl']) > 0 and np.count_nonzero(L['sums']['Kr1']) > 0
        lt = kr.latent(L['P'][0], L['P'][1], L['U'])
        np.testing.assert_array_equal(lt['Al'][0], L['stage'][2])
