"""zigp.transforms.LowerTriangular and the optimiser plumbing for a transform whose free size differs from the value's (no GPU needed)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
from zigp.transforms import LowerTriangular, positive  # noqa: E402
from zigp.optim import P, ParamSet, AdamGroups, lbfgsb  # noqa: E402


@pytest.mark.parametrize('M', [1, 2, 7])
def test_round_trip_free_size_and_order(M):
    t = LowerTriangular(M)
    n = M * (M + 1) // 2
    assert t.free_size() == n
    x = np.arange(1.0, n + 1.0) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)     # negative entries, the diagonal included: unconstrained
    y = t.forward(x)
    assert y.shape == (M, M) and np.all(np.triu(y, 1) == 0.0)
    assert np.array_equal(y[np.tril_indices(M)], x)                              # row-major order of the lower triangle
    assert np.array_equal(t.backward(y), x) and np.array_equal(t.backward(y[:, :, None]), x)
    garbage = y + np.triu(np.full((M, M), 9.0), 1)
    assert np.array_equal(t.backward(garbage), x)                                # the strict upper triangle has no free variable
    with pytest.raises(ValueError):
        t.forward(np.zeros(n + 1))


def test_chain_rule_against_central_differences():
    M = 5
    t = LowerTriangular(M)
    rs = np.random.RandomState(0)
    C = rs.randn(M, M)

    def f(y):                      # a function of the value that also looks at the (always zero) upper triangle
        return float(np.sum(C * y) + 0.5 * np.sum(y * y) + np.sum(np.sin(y)))

    x = rs.randn(t.free_size())
    y = t.forward(x)
    dy = C + y + np.cos(y)
    g = t.grad_free(x, dy.reshape(-1))
    assert g.shape == x.shape
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = 1e-6
        fd = (f(t.forward(x + e)) - f(t.forward(x - e))) / 2e-6
        assert abs(fd - g[i]) <= 1e-8 * max(1.0, abs(fd)), i


def _pset(M=4):
    return ParamSet(OrderedDict([('a', P(np.array([0.5, 2.0]), positive)), ('L', P(np.eye(M)[:, :, None], LowerTriangular(M))),
                                 ('b', P(np.array([[1.0, -1.0]])))]))


def test_paramset_with_a_smaller_free_vector():
    M = 4
    ps = _pset(M)
    x = ps.get_free()
    assert x.size == 2 + M * (M + 1) // 2 + 2
    x2 = x + 0.1 * np.arange(x.size)
    ps.set_free(x2)
    assert ps.params['L'].value.shape == (M, M, 1) and np.all(np.triu(ps.params['L'].value[:, :, 0], 1) == 0.0)
    assert np.allclose(ps.get_free(), x2, rtol=0, atol=1e-14)
    assert np.array_equal(ps.params['b'].value, (x2[-2:]).reshape(1, 2))          # the block behind L starts at the right offset
    g = ps.free_grad(dict(a=np.ones(2), L=np.arange(16.0).reshape(M, M, 1), b=np.array([[3.0, 4.0]])))
    assert g.size == x.size and np.array_equal(g[2:2 + 10], np.arange(16.0).reshape(M, M)[np.tril_indices(M)]) and np.array_equal(g[-2:], [3.0, 4.0])


def test_lbfgsb_and_adam_fit_a_lower_triangular_factor():
    """maximise -0.5 |L L^T - S|^2 over lower-triangular L: both optimisers run on the M(M+1)/2 free entries and keep the upper triangle 0"""
    M = 3
    rs = np.random.RandomState(1)
    B = np.tril(rs.randn(M, M)) + 2 * np.eye(M)
    S = B @ B.T

    def vg(values):
        L = values['L'][:, :, 0]
        E = L @ L.T - S
        return -0.5 * float(np.sum(E * E)), dict(L=(-2.0 * E @ L)[:, :, None])

    ps = ParamSet(OrderedDict([('L', P(np.eye(M)[:, :, None], LowerTriangular(M)))]))
    v0 = vg(ps.values())[0]
    res = lbfgsb(ps, vg, maxiter=200)
    L = ps.params['L'].value[:, :, 0]
    assert res.x.size == 6 and np.all(np.triu(L, 1) == 0.0) and np.allclose(L @ L.T, S, atol=1e-4)
    ps = ParamSet(OrderedDict([('L', P(np.eye(M)[:, :, None], LowerTriangular(M), learning_rate=0.05))]))
    opt = AdamGroups(ps)
    assert opt.m['L'].size == 6
    for _ in range(50):
        opt.step(vg(ps.values())[1])
    L = ps.params['L'].value
    assert L.shape == (M, M, 1) and np.all(np.triu(L[:, :, 0], 1) == 0.0) and vg(ps.values())[0] > v0


def test_engine_parameter_packing_checks_the_full_factor():
    """DenseEngine's host-side checks of p['q_diag'] = False (no library needed): shapes (M, M) and (M, M, 1), the zero-diagonal, wrong-shape
    and whiten-off refusals."""
    from zigp.engine import _Packed
    M, Mg, D = 5, 3, 2
    rs = np.random.RandomState(0)
    p = dict(Zf=rs.rand(M, D), Zg=rs.rand(Mg, D), u_fm=rs.randn(M, 1), u_gm=rs.randn(Mg, 1), u_fs_sqrt=np.eye(M) - 2.0 * np.diag(np.arange(M) == 1),
             u_gs_sqrt=np.eye(Mg)[:, :, None], ell_f=0.3, ell_g=np.array([0.2, 0.4]), var_f=1.0, var_g=2.0, noise=0.1, whiten=True, q_diag=False)
    pk = _Packed(p)
    assert pk.q_full and pk.arr['u_fs_sqrt'].shape == (M, M) and pk.arr['u_gs_sqrt'].shape == (Mg, Mg)      # a negative diagonal entry is legal
    assert not _Packed(dict(p, q_diag=True, u_fs_sqrt=np.ones(M), u_gs_sqrt=np.ones(Mg))).q_full
    with pytest.raises(ValueError, match='whiten'):
        _Packed(dict(p, whiten=False))
    with pytest.raises(ValueError, match='zero diagonal'):
        _Packed(dict(p, u_fs_sqrt=np.eye(M) - np.diag(np.arange(M) == 2)))
    for bad in (np.ones(M), np.ones((M, 1)), np.ones((M, M, 2)), np.ones((M + 1, M + 1))):
        with pytest.raises(ValueError, match='u_fs_sqrt'):
            _Packed(dict(p, u_fs_sqrt=bad))
