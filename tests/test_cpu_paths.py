"""CPU side of the sample paths (include/zigp.h "sample paths"): the draw's random features reproduce each
kernel, zigp.pathwise.weights_np is the linear map whose implied mean and variance are those of the existing restatements, and the
Python-side refusals are raised before the library is touched (no GPU needed)."""
import math

import numpy as np
import pytest

from conftest import make_problem, relerr
import paths_ref as pr
from zigp import pathwise, _lib


@pytest.mark.parametrize('kind', ['rbf', 'matern32', 'matern52'])
def test_random_features_reproduce_the_kernel(kind):
    """(2 / R) sum_r cos(w_r . x + b_r) cos(w_r . x' + b_r) -> k(x, x') / var.  R = 2^18 features, P = 1000 pairs at D = 3 with unequal
    lengthscales; the bound is Hoeffding's for terms in [-2, 2] over the P pairs at failure probability 1e-6:
    sqrt(8 ln(2 P / 1e-6) / R) = 0.0256 -- not a tuned number.  The other two kinds' formulas lie further from the estimate than the bound on these pairs
    (Matern 3/2 and 5/2 differ by 0.049 at most, whatever the pairs; RBF is 0.1 and more away), so a wrong nu or a wrong scaling of the
    frequencies fails."""
    R, P, D = 2 ** 18, 1000, 3
    ell = np.array([0.3, 0.5, 0.8])
    rs = np.random.RandomState(20201)
    X1 = rs.rand(P, D)
    X2 = X1 + ell * rs.randn(P, D) * 0.7
    d = pathwise.draw(kind, R, D, 1, 1, np.random.RandomState(7))
    omega = d['omega0'] / ell[None, :]
    import torch
    t1, t2, est = torch.from_numpy(X1), torch.from_numpy(X2), torch.zeros(P, dtype=torch.float64)
    for r0 in range(0, R, 16384):              # float64 throughout; torch only because its cosine runs on every core
        om, b = torch.from_numpy(omega[r0:r0 + 16384]), torch.from_numpy(d['phase'][r0:r0 + 16384])
        est += torch.sum(torch.cos(t1 @ om.T + b) * torch.cos(t2 @ om.T + b), 1)
    est = est.numpy() * (2.0 / R)
    k = {kd: np.diagonal(pr.kern_np(kd, X1, X2, ell, 1.0)) for kd in ('rbf', 'matern32', 'matern52')}
    bound = math.sqrt(8.0 * math.log(2.0 * P / 1e-6) / R)
    err = float(np.max(np.abs(est - k[kind])))
    print('%s: max error %.4f, bound %.4f' % (kind, err, bound))
    assert abs(bound - 0.0256) < 5e-5
    assert err <= bound
    for other in k:
        if other != kind:
            away = float(np.max(np.abs(k[other] - k[kind])))
            print('  %s is %.3f away' % (other, away))
            assert away > 0.045 and np.max(np.abs(est - k[other])) > bound
    assert np.all((d['phase'] >= 0) & (d['phase'] < 2 * np.pi))


def _modes(p):
    import fullcov_ref as fr
    return (('diag', dict(p)), ('white', dict(p, whiten=True)), ('white_full', fr.make_lq(p, seed=3)))


def test_weights_are_the_right_linear_map():
    """Unit vectors through weights_np: eps -> V gives A (M, M), f_Z -> V gives -B with B = Kuu^-1, and eps = 0, f_Z = 0 gives the mean
    weights.  With the prior draw's covariance K, a path then has mean k V0 and variance Kxx - k B k^T + k A A^T k^T
    (= Kxx - KxZ Kuu^-1 KZx + KxZ Kuu^-1 S_u Kuu^-1 KZx, S_u = Kuu A A^T Kuu): equal to fmean, fvar, gmean, gvar of the existing
    restatements for all three parametrisations, to the 1e-9 of their own comparison with the explicit model on its fixture
    (test_cpu_whiten_ref.py: D = 8, lengthscale 0.6, cond(Kuu) <= 1e5)."""
    import matern_ref as mr
    import whiten_ref as wr
    import fullcov_ref as fr
    X, Y, p0 = make_problem(200, 150, 8, seed=1450, Mg=100, ell=0.6)
    p0['mean_a'], p0['mean_b'] = np.linspace(-0.3, 0.4, 8), 0.25
    jitter, g_off = 1e-6, -1.0
    for mode, p in _modes(p0):
        ref = {'diag': mr.build_predict, 'white': wr.build_predict, 'white_full': fr.build_predict}[mode](X, p, jitter, g_off)
        rows = {'f': (ref[3], ref[4]), 'g': (ref[5], ref[6])}
        if mode == 'white_full':
            (fm, fv, gm, gv), _ = fr.explicit_full_cov(X, p, jitter, g_off)
            rows_x = {'f': (fm, fv), 'g': (gm, gv)}
        for tag in 'fg':
            Z, ell, var = p['Z' + tag], p['ell_' + tag], float(p['var_' + tag])
            M = Z.shape[0]
            Kuu = pr.kern_np('rbf', Z, Z, ell, var) + jitter * np.eye(M)
            assert np.linalg.cond(Kuu) <= 1e5
            kw = dict(whiten=p.get('whiten', False), q_diag=p.get('q_diag', True))
            u, s = p['u_%sm' % tag], p['u_%ss_sqrt' % tag]
            zero, eye = np.zeros((M, M)), np.eye(M)
            V0 = pathwise.weights_np(Kuu, u, s, np.zeros((M, 1)), np.zeros((M, 1)), **kw)
            A = pathwise.weights_np(Kuu, u, s, eye, zero, **kw) - V0
            B = -(pathwise.weights_np(Kuu, u, s, zero, eye, **kw) - V0)
            assert relerr(B @ Kuu, eye) < 1e-9                      # f_Z enters as -Kuu^-1 f_Z
            k = pr.kern_np('rbf', X, Z, ell, var)
            mean = (k @ V0).reshape(-1)
            if tag == 'f':
                mean = mean + X @ p['mean_a'] + p['mean_b']
            else:
                mean = mean + g_off
            kA = k @ A
            v = var - np.sum((k @ B) * k, 1) + np.sum(kA * kA, 1)
            for name, got, want in (('mean', mean, rows[tag][0]), ('var', v, rows[tag][1])):
                e = relerr(got, want)
                print('%s %s%s relerr %.2e' % (mode, tag, name, e))
                assert e < 1e-9, (mode, tag, name, e)
            if mode == 'white_full':
                assert relerr(mean, rows_x[tag][0]) < 1e-9 and relerr(v, rows_x[tag][1]) < 1e-9


def test_restatement_collapses_onto_the_posterior_mean():
    """sample_paths_np with eps = 0 and a = 0 is fmean / gmean of the restatements (every sample the same row), gf = link(g) f"""
    import matern_ref as mr
    X, Y, p = make_problem(60, 20, 3, seed=5, Mg=13)
    p.update(kern_g='matern52', mean_b=0.4)
    draws = {t: pathwise.draw(p.get('kern_' + t, 'rbf'), 32, 3, M, 4, np.random.RandomState(h)) for h, (t, M) in enumerate((('f', 20), ('g', 13)))}
    r = pr.sample_paths_np(p, X, pr.zero_draws(draws), 1e-6, g_offset=-1.0)
    ref = mr.build_predict(X, p, 1e-6, -1.0)
    for s in range(4):
        assert relerr(r['f'][s], ref[3]) < 1e-9 and relerr(r['g'][s], ref[5]) < 1e-9
    assert np.array_equal(r['gf'], pr.link(r['g']) * r['f'])


def test_python_side_refusals():
    """D > 8, S = 0, S > 256 and mismatched table shapes raise ValueError before the library is touched"""
    from zigp.engine import DenseEngine
    e = DenseEngine.__new__(DenseEngine)          # no context: a refusal that reached the library would fail on the missing attribute
    rs = np.random.RandomState(0)

    def lat(M=4, R=6, D=2, S=3, **kw):
        q = dict(kind='rbf', Z=rs.rand(M, D), ell=0.5, var=1.0, V=rs.randn(M, S), omega=rs.randn(R, D), phase=rs.rand(R), amp=rs.randn(R, S))
        q.update(kw)
        return q
    with pytest.raises(ValueError, match='D = 9'):
        e.path_rows([lat(D=9)], rs.rand(5, 9), 3)
    with pytest.raises(ValueError, match='S = 0'):
        e.path_rows([lat()], rs.rand(5, 2), 0)
    with pytest.raises(ValueError, match='S = 257'):
        e.path_rows([lat()], rs.rand(5, 2), 257)
    for key, bad in (('V', rs.randn(4, 2)), ('amp', rs.randn(6, 4)), ('omega', rs.randn(6, 3)), ('lin', np.ones(3)), ('Z', rs.rand(4, 3))):
        with pytest.raises(ValueError, match=key):
            e.path_rows([lat(**{key: bad})], rs.rand(5, 2), 3)
    with pytest.raises(ValueError, match='one or two'):
        e.path_rows([lat(), lat(), lat()], rs.rand(5, 2), 3)
    with pytest.raises(ValueError, match='kernel'):
        e.path_rows([lat(kind='cosine')], rs.rand(5, 2), 3)
    # sample_paths: the sizes, then the draws against the model
    X, Y, p9 = make_problem(10, 4, 9)
    with pytest.raises(ValueError, match='D = 9'):
        e.sample_paths(p9, X, n_samples=4)
    X, Y, p = make_problem(10, 4, 2, Mg=5)
    for S in (0, 257):
        with pytest.raises(ValueError, match='S = %d' % S):
            e.sample_paths(p, X, n_samples=S)
    draws = {t: pathwise.draw('rbf', 8, 2, M, 3, rs) for t, M in (('f', 4), ('g', 5))}
    with pytest.raises(ValueError, match=r'draw_f\.a must be \(8, 4\)'):
        e.sample_paths(p, X, n_samples=4, draws=draws)                      # drawn for 3 samples
    with pytest.raises(ValueError, match=r'draw_g\.omega0'):
        e.sample_paths(p, X, n_samples=3, draws=dict(draws, g=dict(draws['g'], omega0=rs.randn(8, 3))))
    with pytest.raises(ValueError, match='Xnew'):
        e.sample_paths(p, rs.rand(10, 3), n_samples=3, draws=draws)
    with pytest.raises(ValueError, match='D = 9'):
        pathwise.draw('rbf', 8, 9, 4, 3, rs)


def test_binding_matches_the_header():
    """the four path entry points are bound with as many arguments as include/zigp.h declares, and the two structs have the header's
    layout (LP64)"""
    import ctypes as C
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name in ('zigp_path_rows', 'zigp_path_rows_device', 'zigp_sample_paths', 'zigp_sample_paths_device'):
        decl = re.search(r'int %s\((.*?)\);' % name, hdr, re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == decl.count(',') + 1, name
    assert C.sizeof(_lib.zigp_path_latent) == 16 + 8 * 9 and C.sizeof(_lib.zigp_path_draw) == 8 + 8 * 4
    assert '#define ZIGP_PATH_MAX_S %d' % _lib.PATH_MAX_S in hdr
