"""CPU checks of tests/dense_head_ref.py, the restatement the GPU tests of the dense heads compare against (tests/test_gpu_dense_head.py),
and of what onoffgpf.SVGP does before it needs a GPU."""
import numpy as np
import pytest
import torch

import zigp_oracle as zo
import zigp_oracle_torch as ot
import dense_head_ref as hr
import matern_ref as mr
import fullcov_ref as fr
from zigp_oracle_torch import _t

LD = np.longdouble


def _fixture(seed=5, N=24, M=6, D=2):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    Yg = np.sin(3 * X[:, :1]) + 0.3 * rs.randn(N, 1)
    Yb = (rs.rand(N, 1) < 0.5) * 1.0
    Yb[:3] = 2.0                                          # a label that is neither 0 nor 1 counts as off
    g = np.stack(np.meshgrid(np.linspace(0.1, 0.9, 3), np.linspace(0.2, 0.8, 2), indexing='ij'), -1).reshape(-1, 2)
    p = dict(Zf=g + 0.02 * rs.randn(M, D), u_fm=0.5 * rs.randn(M, 1), u_fs_sqrt=0.3 + rs.rand(M, 1), ell_f=np.array([0.3, 0.4]), var_f=1.3,
             noise=0.07)
    return X, Yg, Yb, p


def _Y(lik, Yg, Yb):
    return Yg if lik == 'gaussian' else Yb


def _kron_form(X, p):
    """the same model as a 6 x 1 Kronecker grid: the second factor is one point at 0 with variance 1, the rows carry a zero column"""
    pk = dict(Zf=[p['Zf'], np.zeros((1, 1))], ell_f=[p['ell_f'], np.ones(1)], var_f=[p['var_f'], 1.0], u_fm=p['u_fm'], u_fs_sqrt=p['u_fs_sqrt'],
              noise=p['noise'])
    return np.hstack([X, np.zeros((X.shape[0], 1))]), pk


def test_gaussian_data_term_is_the_oracles_formula():
    """ve of the Gaussian head == oracle.variational_expectations(fmean, fvar, 0, Y, noise), element for element: one formula."""
    rs = np.random.RandomState(0)
    fm, fv, Y = rs.randn(50, 1), rs.rand(50, 1), rs.randn(50, 1)
    a = hr.head_ve('gaussian', _t(fm), _t(fv), _t(Y), _t(0.07))
    b = ot.variational_expectations(_t(fm), _t(fv), 0.0, _t(Y), _t(0.07))
    assert torch.equal(a, b)
    assert np.array_equal(a.numpy(), zo.variational_expectations(fm, fv, 0.0, Y, 0.07))


# relative distances measured on this fixture (cond(Kuu) = 6.8), the restatement (Cholesky) against the oracle (LU inverse).  The Bernoulli
# data term measured 0 (the same double): one eps, the precision of the format, stands in for it so that the bound is not "equal"
MEASURED = dict(gaussian=dict(data=2.1e-16, kl=6.3e-16, rows=1.2e-15), bernoulli=dict(data=2.3e-16, kl=6.3e-16, rows=1.2e-15))


@pytest.mark.parametrize('lik', hr.LIKS)
def test_both_heads_match_the_kronecker_oracle(lik):
    """M = 6, D = 2, jitter 0 against oracle.kron_head_elbo / kron_head_predict on the one-factor-equivalent grid.  The two differ in
    operation order only (Cholesky and triangular solves here, tf.matrix_inverse there).  Measured relative distances: data term 2.0e-16
    (Gaussian) / 0 (Bernoulli), KL 6.2e-16, predict rows 1.1e-15 at most; asserted: 10 x those (MEASURED)."""
    X, Yg, Yb, p = _fixture()
    Y = _Y(lik, Yg, Yb)
    K = mr.kern_K_np('rbf', p['Zf'], None, p['ell_f'], p['var_f'])
    c = np.linalg.cond(K)
    assert c <= 1e4, c
    Xk, pk = _kron_form(X, p)
    elbo_o, data_o, kl_o = zo.kron_head_elbo(Xk, Y, pk, lik, 0.0, scale=1.7)
    elbo_r, data_r, kl_r, _ = hr.elbo_and_grad(X, Y, p, lik, 0.0, scale=1.7)
    rows_o = zo.kron_head_predict(Xk, pk, lik, 0.0)
    rows_r = hr.head_predict(X, p, lik, 0.0)
    if lik == 'gaussian':
        pairs = [(rows_r[0], rows_o[0]), (rows_r[1], rows_o[1]), (rows_r[2], rows_o[0]), (rows_r[3], rows_o[1] + p['noise'])]
    else:
        pairs = [(rows_r[0], rows_o[2]), (rows_r[1], rows_o[3]), (rows_r[2], rows_o[0]), (rows_r[3], rows_o[1])]
    e_rows = max(float(np.max(np.abs(a.reshape(-1) - b.reshape(-1))) / np.max(np.abs(b))) for a, b in pairs)
    e_d, e_k = abs(data_r - data_o) / abs(data_o), abs(kl_r - kl_o) / abs(kl_o)
    print('dense head restatement against the Kronecker oracle, %s: cond(Kuu) %.2e, data %.2e, kl %.2e, predict rows %.2e' % (lik, c, e_d, e_k, e_rows))
    m = MEASURED[lik]
    assert e_d <= 10 * m['data'] and e_k <= 10 * m['kl'] and e_rows <= 10 * m['rows']
    assert abs(elbo_r - elbo_o) <= 10 * (m['data'] * abs(1.7 * data_o) + m['kl'] * abs(kl_o))


# ---- the bound in numpy.longdouble, for central differences ----
def _ld_erf(x):
    import mpmath as mp
    mp.mp.dps = 40
    out = np.empty(x.shape, dtype=LD)
    for i, v in np.ndenumerate(x):
        hi = float(v)
        r = mp.erf(mp.mpf(hi) + mp.mpf(float(v - LD(hi))))
        rh = float(r)
        out[i] = LD(rh) + LD(float(r - mp.mpf(rh)))
    return out


def _ld_chol(K):
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - np.sum(L[j, :j] ** 2))
        for i in range(j + 1, n):
            L[i, j] = (K[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return L


def _ld_solve_lower(L, B):
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _ld_kern(kind, A, B, ell, var):
    d = (A[:, None, :] - B[None, :, :]) / ell
    r2 = np.sum(d * d, 2)
    if kind == 'rbf':
        return var * np.exp(-r2 / 2)
    r = np.sqrt(r2 + LD(mr.FLOOR))
    s5 = np.sqrt(LD(5))
    return var * (1 + s5 * r + LD(5) / 3 * r * r) * np.exp(-s5 * r)


def _ld_elbo(X, Y, p, lik, kind, mode, jitter, scale):
    """scale * sum ve - KL_f in longdouble: the formulas of matern_ref.conditional / latent_kl and of dense_head_ref.head_ve"""
    q = {k: np.asarray(v, dtype=LD) for k, v in p.items()}
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD).reshape(-1, 1)
    M = q['Zf'].shape[0]
    u = q['u_fm'].reshape(M, 1)
    Kmm = _ld_kern(kind, q['Zf'], q['Zf'], q['ell_f'], q['var_f']) + np.eye(M, dtype=LD) * LD(jitter)
    L = _ld_chol(Kmm)
    A = _ld_solve_lower(L, _ld_kern(kind, q['Zf'], X, q['ell_f'], q['var_f']))
    fvar = q['var_f'] - np.sum(A * A, 0)
    if mode == 'diag':
        A = _ld_solve_lower(L.T[::-1, ::-1], A[::-1])[::-1]
    fmean = A.T @ u
    if mode == 'white_full':
        Lq = np.tril(q['u_fs_sqrt'].reshape(M, M))
        fvar = fvar + np.sum((Lq.T @ A) ** 2, 0)
    else:
        fvar = fvar + np.sum((A * q['u_fs_sqrt'].reshape(M, 1)) ** 2, 0)
    fmean, fvar = fmean.reshape(-1, 1), fvar.reshape(-1, 1)
    if 'mean_a' in q:
        fmean = fmean + X @ q['mean_a'].reshape(-1, 1)
    if 'mean_b' in q:
        fmean = fmean + q['mean_b']
    if lik == 'gaussian':
        ve = -LD(0.5) * np.log(2 * LD(np.pi)) - LD(0.5) * np.log(q['noise']) - LD(0.5) * ((Y - fmean) ** 2 + fvar) / q['noise']
    else:
        pr = LD(0.5) * (1 + _ld_erf(fmean / np.sqrt(1 + fvar) / np.sqrt(LD(2)))) * (1 - LD(2e-3)) + LD(1e-3)
        ve = np.log(np.where(Y == 1, pr, 1 - pr))
    if mode == 'diag':
        s = q['u_fs_sqrt'].reshape(M, 1)
        alpha = _ld_solve_lower(L, u)
        Li = _ld_solve_lower(L, np.eye(M, dtype=LD))
        kl = LD(0.5) * (np.sum(alpha ** 2) - M - np.sum(np.log(s ** 2)) + np.sum(np.diag(Li.T @ Li).reshape(M, 1) * s ** 2)
                        + np.sum(np.log(np.diag(L) ** 2)))
    elif mode == 'white':
        s = q['u_fs_sqrt'].reshape(M, 1)
        kl = LD(0.5) * (np.sum(u ** 2) - M - np.sum(np.log(s ** 2)) + np.sum(s ** 2))
    else:
        Lq = np.tril(q['u_fs_sqrt'].reshape(M, M))
        kl = LD(0.5) * (np.sum(u ** 2) - M - np.sum(np.log(np.diag(Lq) ** 2)) + np.sum(Lq ** 2))
    return LD(scale) * np.sum(ve) - kl


@pytest.mark.parametrize('mode,kind,mean', [('diag', 'rbf', False), ('white', 'matern52', True), ('white_full', 'rbf', True)])
@pytest.mark.parametrize('lik', hr.LIKS)
def test_autograd_against_central_differences(lik, mode, kind, mean):
    """Every block's autograd gradient of scale * data - KL against central differences of the same bound evaluated in numpy.longdouble
    (steps h = 1e-6: truncation ~h^2 = 1e-12 relative to the third derivative, rounding 1e-19 / h).  Bound: 1e-7 of the block's largest
    entry -- six orders above both error terms, five below the 1e-6 the GPU gradients are held to."""
    X, Yg, Yb, p = _fixture()
    Y = _Y(lik, Yg, Yb)
    if mode == 'white':
        p['whiten'] = True
    if mode == 'white_full':
        p = {k: v for k, v in fr.make_lq(dict(p, Zg=p['Zf'], u_gm=p['u_fm'], u_gs_sqrt=p['u_fs_sqrt']), seed=1, negative=1).items() if k not in ('Zg', 'u_gm', 'u_gs_sqrt')}
    if kind != 'rbf':
        p['kern_f'] = kind
    if mean:
        p['mean_a'], p['mean_b'] = np.array([0.25, -0.5]), 0.37
    jitter, scale = 1e-6, 1.7
    elbo, data, kl, g = hr.elbo_and_grad(X, Y, p, lik, jitter, scale=scale)
    num = {k: v for k, v in p.items() if k not in ('whiten', 'q_diag', 'kern_f')}
    base = _ld_elbo(X, Y, num, lik, kind, mode, jitter, scale)
    assert abs(float(base) - elbo) <= 1e-12 * abs(elbo)
    h = LD(1e-6)
    for k in [k for k in g if not (k == 'noise' and lik == 'bernoulli')]:
        v0 = np.asarray(num[k], dtype=LD)
        fd = np.zeros(v0.shape, dtype=np.float64)
        idx = list(np.ndindex(*v0.shape)) if v0.ndim else [()]
        if k == 'u_fs_sqrt' and mode == 'white_full':
            idx = [i for i in idx if i[1] <= i[0]]                    # the strict upper triangle is not read
        for i in idx:
            up, dn = v0.copy(), v0.copy()
            up[i] += h
            dn[i] -= h
            fd[i] = float((_ld_elbo(X, Y, dict(num, **{k: up}), lik, kind, mode, jitter, scale)
                           - _ld_elbo(X, Y, dict(num, **{k: dn}), lik, kind, mode, jitter, scale)) / (2 * h))
        e = np.max(np.abs(fd - np.asarray(g[k]).reshape(fd.shape))) / np.max(np.abs(fd))
        print('%s %s %s grad %-10s autograd against longdouble central differences %.2e' % (lik, mode, kind, k, e))
        assert e <= 1e-7, (k, e)
    if lik == 'bernoulli':
        assert not np.any(g['noise'])


def test_hand_derived_cotangents_are_the_autograd_ones():
    """dfm, dfv, dnoise as the kernel forms them (head_cotangents) against autograd of head_ve at random points: 1e-12 relative."""
    rs = np.random.RandomState(3)
    fm, fv, noise = rs.randn(200) * 2, rs.rand(200) * 3 + 1e-3, 0.3
    for lik in hr.LIKS:
        y = rs.randn(200) if lik == 'gaussian' else np.where(rs.rand(200) < 0.4, 1.0, np.where(rs.rand(200) < 0.5, 0.0, 2.0))
        a, b, n = (_t(v).clone().requires_grad_(True) for v in (fm, fv, noise))
        torch.sum(hr.head_ve(lik, a, b, _t(y), n)).backward()
        dfm, dfv, dnoise = hr.head_cotangents(lik, fm, fv, y, noise)
        for name, got, ref in (('dfm', dfm, a.grad.numpy()), ('dfv', dfv, b.grad.numpy())):
            assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref)), (lik, name)
        if lik == 'gaussian':
            assert abs(np.sum(dnoise) - float(n.grad)) <= 1e-12 * abs(float(n.grad))
        else:
            assert n.grad is None or float(n.grad) == 0.0


@pytest.mark.parametrize('mistake', hr.MISTAKES)
def test_each_deliberate_mistake_is_caught(mistake):
    """The checks above, run on a restatement with one planted error, fail: fv left out of the Gaussian q, the 1e-3 clamp dropped,
    y > 0 in place of y == 1 (the fixture has labels 2.0), the sign of dfv, the placeholder's KL left in (jitter 1e-2, where that KL is
    2.5e-5; at jitter 0 and in the whitened models it is exactly 0, which is why nothing shows there)."""
    X, Yg, Yb, p = _fixture()
    Xk, pk = _kron_form(X, p)
    lik = 'gaussian' if mistake in ('no_fv', 'placeholder_kl') else 'bernoulli'
    Y = _Y(lik, Yg, Yb)
    if mistake == 'dfv_sign':
        rs = np.random.RandomState(3)
        fm, fv = rs.randn(50), rs.rand(50) + 0.1
        for lk, y in (('gaussian', rs.randn(50)), ('bernoulli', (rs.rand(50) < 0.5) * 1.0)):
            good, bad = hr.head_cotangents(lk, fm, fv, y, 0.3)[1], hr.head_cotangents(lk, fm, fv, y, 0.3, mistake=mistake)[1]
            assert np.max(np.abs(bad - good)) > 1e-3 * np.max(np.abs(good))
        return
    if mistake == 'placeholder_kl':      # (at jitter > 0 the Kronecker oracle is another model: it adds the jitter to the one-point factor too)
        num = {k: v for k, v in p.items()}
        ld = float(_ld_elbo(X, Y, num, lik, 'rbf', 'diag', 1e-2, 1.0))
        good = hr.elbo_and_grad(X, Y, p, lik, 1e-2, need_grad=False)
        bad = hr.elbo_and_grad(X, Y, p, lik, 1e-2, need_grad=False, mistake=mistake)
        assert abs(good[0] - ld) <= 1e-12 * abs(ld)                 # the check of test_autograd_against_central_differences
        assert not abs(bad[0] - ld) <= 1e-12 * abs(ld)
        assert 2.4e-5 < bad[2] - good[2] < 2.6e-5 and bad[1] == good[1]
        return
    jitter = 0.0
    elbo_o, data_o, kl_o = zo.kron_head_elbo(Xk, Y, pk, lik, jitter)
    good = hr.elbo_and_grad(X, Y, p, lik, jitter, need_grad=False)
    bad = hr.elbo_and_grad(X, Y, p, lik, jitter, need_grad=False, mistake=mistake)
    m = MEASURED[lik]
    ok = lambda r: abs(r[1] - data_o) <= 10 * m['data'] * abs(data_o) and abs(r[2] - kl_o) <= 10 * m['kl'] * abs(kl_o)      # noqa: E731
    assert ok(good)
    assert not ok(bad), mistake


# ---- onoffgpf.SVGP before it needs a GPU ----
def test_svgp_packing_and_refusals_without_a_gpu():
    from onoffgpf import SVGP, kernels, likelihoods, mean_functions, OnOffLikelihood
    rs = np.random.RandomState(0)
    X, Y = rs.rand(30, 2), rs.randn(30, 1)
    Z = X[:5].copy()
    m = SVGP(X, Y, kernels.Matern52(2, lengthscales=0.5), likelihoods.Gaussian(), Z)      # GPflow's defaults: q_diag=False, whiten=True
    assert m.whiten and not m.q_diag and m.q_mu.value.shape == (5, 1) and m.q_sqrt.value.shape == (5, 5, 1)
    assert float(m.likelihood.variance.value[0]) == 1.0
    v = m._values()
    assert set(v) == {'Zf', 'u_fm', 'u_fs_sqrt', 'ell_f', 'var_f', 'noise', 'whiten', 'q_diag', 'kern_f'}
    assert v['whiten'] is True and v['q_diag'] is False and v['kern_f'] == 'matern52' and np.array_equal(v['ell_f'], [0.5, 0.5])
    ps = m._pset()
    assert list(ps.params) == ['Zf', 'u_fm', 'u_fs_sqrt', 'ell_f', 'var_f', 'noise']
    assert ps.get_free().size == 10 + 5 + 15 + 1 + 1 + 1           # the lower triangle of q_sqrt, one shared lengthscale
    g = m._fold_grads(dict(Zf=np.ones((5, 2)), u_fm=np.ones(5), u_fs_sqrt=np.ones((5, 5)), ell_f=np.array([1.0, 2.0]), var_f=0.5, noise=0.25))
    assert g['ell_f'].tolist() == [3.0] and g['u_fs_sqrt'].shape == (5, 5, 1) and g['noise'].tolist() == [0.25]
    assert ps.free_grad(g).size == ps.get_free().size
    b = SVGP(X, (Y > 0) * 1.0, kernels.RBF(2, ARD=True), likelihoods.Bernoulli(), Z, mean_function=mean_functions.Constant(), q_diag=True, whiten=False,
             minibatch_size=10)
    assert list(b._pset().params)[:5] == ['Zf', 'u_fm', 'u_fs_sqrt', 'ell_f', 'var_f'] and 'noise' not in b._pset().params
    assert 'noise' not in b._values() and 'kern_f' not in b._values() and 'mean_b' in b._values() and b.q_sqrt.value.shape == (5, 1)
    assert b.minibatch_size == 10 and b._sample_rows().shape == (10,)
    assert not hasattr(likelihoods.Bernoulli(), 'variance')
    with pytest.raises(NotImplementedError):
        SVGP(X, Y, kernels.RBF(2), likelihoods.Gaussian(), Z, q_diag=False, whiten=False)
    with pytest.raises(TypeError):
        SVGP(X, Y, kernels.RBF(2), OnOffLikelihood(), Z)
    with pytest.raises(ValueError):
        SVGP(X, Y[:, 0], kernels.RBF(2), likelihoods.Gaussian(), Z)
    with pytest.raises(ValueError):
        SVGP(X, Y, kernels.RBF(2), likelihoods.Gaussian(), Z[:, :1])
    X9 = rs.rand(30, 9)
    with pytest.raises(ValueError, match='Matern'):
        SVGP(X9, Y, kernels.Matern32(9), likelihoods.Gaussian(), X9[:4])
    with pytest.raises(ValueError, match='Linear'):
        SVGP(X9, Y, kernels.RBF(9), likelihoods.Gaussian(), X9[:4], mean_function=mean_functions.Linear(np.zeros((9, 1)), 0.0))
    import pickle
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._engine_obj is None and np.array_equal(m2.Z.value, m.Z.value)
    ve = likelihoods.Gaussian(0.3).variational_expectations(np.zeros(3), np.ones(3), np.ones(3))
    assert np.allclose(ve, -0.5 * np.log(2 * np.pi * 0.3) - 0.5 * 2 / 0.3)


def test_head_entry_points_and_placeholder_without_a_gpu():
    """The symbols resolve; head_placeholder is the documented latent; the engine's Python-side refusals need no context."""
    import zigp
    from zigp import _lib
    lib = _lib.load()
    for name in ('zigp_head_elbo', 'zigp_head_predict', 'zigp_head_predict_device', 'zigp_test_pointwise_head'):
        assert getattr(lib, name) is not None
    assert lib.zigp_head_elbo(None, None, 1, 1e-6, 1.0, 0, 0, 1, None, None, None) == _lib.ZIGP_EARG
    assert lib.zigp_head_predict(None, None, 1, None, 0, 1e-6, None) == _lib.ZIGP_EARG
    ph = zigp.head_placeholder(3)
    assert ph['Zg'].shape == (1, 3) and not ph['Zg'].any() and ph['u_gm'].tolist() == [0.0] and ph['u_gs_sqrt'].tolist() == [1.0]
    assert ph['ell_g'].tolist() == [1.0] * 3 and ph['var_g'] == 1.0 and ph['kern_g'] == 'rbf'
    assert zigp.head_placeholder(2, q_full=True)['u_gs_sqrt'].shape == (1, 1)
    assert zigp.HEAD_PARAM_KEYS == hr.HEAD_KEYS
