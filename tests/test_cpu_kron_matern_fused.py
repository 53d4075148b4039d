"""CPU side of the fused Matern tests (tests/test_gpu_kron_matern_fused.py): what makes their tolerances mean something.

* The fixtures.  The fused-eligible cases of kron_matern_ref.FIXTURES are held to floor <= 1e-8 and cond(K_p + 1e-5 I) <= 1e5 by
  tests/test_cpu_kron_matern.py; the four cases kronf_matern_ref.NEW_KINDS adds are held to the same two conditions here, with the same
  function (kron_matern_ref.fixture_floor_and_cond), and the table carries every one of the nine (kind0, kind1) pairs.
* tests/kronf_matern_ref.py, the restatement the stage tests compare the kernels with: with every kind RBF it returns kronf_ref's bits;
  its Matern tiles are kron_matern_ref's kernels, and its K' is -dK / d(r2 / 2) as torch differentiates those kernels."""
import numpy as np
import pytest
import torch

import kron_nd
import kron_matern_ref as kmr
import kronf_matern_ref as fm
import kronf_ref as R

pytestmark = pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)
LD = np.longdouble


def test_the_table_is_fused_eligible_and_has_every_pair_of_kinds():
    table = fm.fixture_kinds()
    assert set(fm.PINNED) <= set(kmr.FIXTURES) and not set(fm.NEW_KINDS) & set(kmr.FIXTURES)
    pairs = set()
    for name, (kf, kg) in table.items():
        case = kron_nd.CASES[name]
        assert name in kron_nd.FUSED and max(case['D']) <= 7
        pairs |= {tuple(kf), tuple(kg)}
    assert pairs == set(kmr.PAIRS)
    assert any(k != 'rbf' for name in fm.NEW_KINDS for pair in table[name] for k in pair)


@pytest.mark.parametrize('name', list(fm.NEW_KINDS))
def test_new_fixtures_hold_the_floor_and_the_conditioning(name):
    X, Y, p = fm.fixture(name)
    floor, cond = kmr.fixture_floor_and_cond(X, p, kron_nd.JITTER)
    print('%s f %s g %s: op-order floor %.2e, cond %s' % (name, p['kern_f'], p['kern_g'], floor, {k: '%.2e' % v for k, v in cond.items()}))
    assert floor <= 1e-8
    assert max(cond.values()) <= 1e5


def _small(seed=3, M=(5, 7), D=(2, 1), N=23):
    rs = np.random.RandomState(seed)
    Z = [rs.rand(M[q], D[q]) * 3 for q in range(2)]
    ell = [0.5 + rs.rand(D[q]) for q in range(2)]
    var = [1.7, 0.8]
    X = rs.rand(N, D[0] + D[1]) * 3
    P = [np.linalg.inv(fm.factor_K('rbf', Z[q], ell[q], var[q], 1e-5)) for q in range(2)]
    Al, S2 = rs.randn(*M), rs.rand(*M) + 0.1
    cot = rs.randn(4, N)
    zc = [0.5 * (Z[q].min(0) + Z[q].max(0)) for q in range(2)]
    return (P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1]), X, N, cot, zc


@pytest.mark.parametrize('dtype', [np.float64, LD])
def test_every_kind_rbf_returns_the_bits_of_kronf_ref(dtype):
    stage, X, N, cot, zc = _small()
    a, b = fm.forward(('rbf', 'rbf'), *stage, X, N, dtype=dtype), R.forward(*stage, X, N, dtype=dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ga = fm.backward(('rbf', 'rbf'), *stage, X, N, None, cot[0], cot[1], cot[2], cot[3], zc[0], zc[1], dtype=dtype)
    gb = R.backward(*stage, X, N, None, cot[0], cot[1], cot[2], cot[3], zc[0], zc[1], dtype=dtype)
    for k in gb:
        assert np.array_equal(ga[k][0], gb[k][0]) and np.array_equal(ga[k][1], gb[k][1]), k
    assert ga['Kd0'] is None and ga['Kd1'] is None
    for q in range(2):
        Z, ell, var = stage[4 + q], stage[6 + q], stage[8 + q]
        k, e = fm.ktile('rbf', Z, ell, var, X[:, :2] if q == 0 else X[:, 2:], dtype, True)
        k2, e2 = R.ktile(Z, ell, var, X[:, :2] if q == 0 else X[:, 2:], dtype, True)
        assert np.array_equal(k, k2) and np.array_equal(e, e2)


@pytest.mark.parametrize('kind', ['matern32', 'matern52'])
def test_matern_tiles_are_the_reference_kernels_and_kd_is_their_derivative(kind):
    """K against kron_matern_ref.factor_K (GPflow's Matern, direct differences); K' through the identity the reverse pass uses:
    d / dz_md sum W . K = sum_n W K' (x_nd - z_md) / ell_d^2, the left side from torch autograd on the reference kernel."""
    stage, X, N, cot, zc = _small(seed=5)
    Z, ell, var, Xp = stage[4], stage[6], stage[8], X[:, :2]
    K, eK, Kd, eKd = fm.ktile(kind, Z, ell, var, Xp, LD, grad=True)
    Zt = torch.tensor(Z, requires_grad=True)
    Kt = kmr.factor_K(kind, Zt, torch.tensor(Xp), torch.tensor(ell), var)
    assert np.max(np.abs(np.asarray(K, dtype=np.float64) - Kt.detach().numpy())) <= 1e-13 * var
    assert np.all(eK >= np.abs(K)) and np.all(eKd >= np.abs(Kd))
    W = np.random.RandomState(1).randn(*Kt.shape)
    (Kt * torch.tensor(W)).sum().backward()
    diff = Xp[None, :, :] - Z[:, None, :]
    mine = np.einsum('mn,mnd->md', W * np.asarray(Kd, dtype=np.float64), diff) / ell ** 2
    assert np.max(np.abs(mine - Zt.grad.numpy())) <= 1e-11 * np.max(np.abs(Zt.grad.numpy()))
    # and K_p(Z, Z) + jitter as the factor kernel builds it
    Kzz = fm.factor_K(kind, Z, ell, var, 1e-5, LD)
    ref = kmr.factor_K_np(kind, Z, None, ell, var) + 1e-5 * np.eye(Z.shape[0])
    assert np.max(np.abs(np.asarray(Kzz, dtype=np.float64) - ref)) <= 1e-13 * var


def test_matern_moment_block_splits_between_k_and_kd():
    """column 0 of Kr_p is kronf_ref's (dK . K); with a Matern factor the other columns and Kd_p come from K' -- the value differs from
    the RBF-style block by far more than rounding, and Kd_p is the zeroth moment of the same t'"""
    stage, X, N, cot, zc = _small(seed=7)
    kinds = ('matern32', 'matern52')
    g = fm.backward(kinds, *stage, X, N, None, cot[0], cot[1], cot[2], cot[3], zc[0], zc[1], dtype=LD)
    t = fm._Tiles(kinds, stage[0], stage[1], *stage[4:], X, N, LD)
    for p in range(2):
        Kr, Kd = g['Kr%d' % p][0], g['Kd%d' % p][0]
        ratio = t.Kd[p] / t.K[p]
        assert np.max(np.abs(ratio - 1)) > 0.1                      # K' is not K
        assert Kr.shape == (stage[4 + p].shape[0], 1 + 2 * stage[4 + p].shape[1]) and Kd.shape == (Kr.shape[0],)
        assert np.all(g['Kr%d' % p][1] >= np.abs(Kr)) and np.all(g['Kd%d' % p][1] >= np.abs(Kd))
