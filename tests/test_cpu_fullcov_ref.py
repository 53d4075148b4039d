"""Pins tests/fullcov_ref.py, the CPU restatement of the full-covariance q(u) on the whitened model that the GPU tests compare against
(no GPU needed)."""
import numpy as np

from conftest import make_problem, relerr
import fullcov_ref as fr
import whiten_ref as wr


def _cond(p, tag, jitter):
    import zigp_oracle as o
    K = o.rbf_K(p['Z' + tag], None, p['ell_' + tag], p['var_' + tag]) + jitter * np.eye(p['Z' + tag].shape[0])
    return np.linalg.cond(K)


def test_equals_the_explicit_full_covariance_model():
    """q(u) = N(L u, L Lq Lq^T L^T) pushed through the unwhitened full-covariance formulas with dense inverses: latent means and variances
    and the KL to 1e-9 relative -- the case and the bound of test_cpu_whiten_ref.py's comparison (cond(Kuu) <= 1e5, asserted)."""
    X, Y, p = make_problem(1300, 150, 8, seed=1450, Mg=100, ell=0.6)
    jitter = 1e-6
    cf, cg = _cond(p, 'f', jitter), _cond(p, 'g', jitter)
    print('cond(Kuu) f %.2e g %.2e' % (cf, cg))
    assert max(cf, cg) <= 1e5
    p = fr.make_lq(p, seed=1)
    p['mean_a'], p['mean_b'] = np.linspace(-0.3, 0.4, 8), 0.25
    for g_off in (0.0, -1.0):
        out = fr.build_predict(X, p, jitter, g_off)
        (fm, fv, gm, gv), kl = fr.explicit_full_cov(X, p, jitter, g_off)
        for name, a, b in (('fmean', out[3], fm), ('fvar', out[4], fv), ('gmean', out[5], gm), ('gvar', out[6], gv)):
            e = relerr(a, b)
            print('  g_offset %+.0f %s relerr %.2e' % (g_off, name, e))
            assert e < 1e-9, (name, e)
    _, _, kl_w, _ = fr.elbo_and_grad(X[:8], Y[:8], p, jitter, need_grad=False)
    print('  KL %.12e explicit %.12e' % (kl_w, kl))
    assert abs(kl_w - kl) <= 1e-9 * abs(kl)


def test_diagonal_factor_equals_the_diagonal_whitened_reference():
    """Lq = diag(s): predict rows, data term, KL and every shared gradient block equal whiten_ref's to 1e-12 (the same sums, one of them
    written as a matrix product); diag(dLq) is its ds."""
    X, Y, p = make_problem(500, 40, 3, seed=5, Mg=23, ell=0.4)
    p['mean_b'] = 0.2
    q = dict(p, u_fs_sqrt=np.diag(p['u_fs_sqrt'].reshape(-1)), u_gs_sqrt=np.diag(p['u_gs_sqrt'].reshape(-1))[:, :, None])
    jitter = 1e-6
    for i, (a, b) in enumerate(zip(fr.build_predict(X, q, jitter, -1.0), wr.build_predict(X, p, jitter, -1.0))):
        assert relerr(a, b) < 1e-12, i
    e_f, d_f, k_f, g_f = fr.elbo_and_grad(X, Y, q, jitter, scale=1.3)
    e_w, d_w, k_w, g_w = wr.elbo_and_grad(X, Y, p, jitter, scale=1.3)
    assert abs(d_f - d_w) <= 1e-12 * abs(d_w) and abs(k_f - k_w) <= 1e-12 * abs(k_w)
    for k in g_w:
        a = np.asarray(g_f[k])
        if k in ('u_fs_sqrt', 'u_gs_sqrt'):
            a = np.diagonal(a.reshape(a.shape[0], a.shape[1]))
        assert relerr(a.reshape(-1), np.asarray(g_w[k]).reshape(-1)) < 1e-10, k


def test_strict_upper_triangle_is_ignored_and_has_zero_gradient():
    X, Y, p = make_problem(300, 30, 2, seed=8, Mg=19, ell=0.5)
    a, b = fr.make_lq(p, seed=2), fr.make_lq(p, seed=2, garbage=True)
    for tag in 'fg':
        k = 'u_%ss_sqrt' % tag
        assert np.array_equal(np.tril(a[k]), np.tril(b[k])) and np.all(np.abs(np.triu(b[k], 1)[np.triu_indices(b[k].shape[0], 1)]) > 0)
    jitter = 1e-6
    assert np.array_equal(fr.build_predict(X, a, jitter), fr.build_predict(X, b, jitter))
    ra, rb = fr.elbo_and_grad(X, Y, a, jitter), fr.elbo_and_grad(X, Y, b, jitter)
    assert ra[:3] == rb[:3]
    for k in ra[3]:
        assert np.array_equal(ra[3][k], rb[3][k]), k
    for k in ('u_fs_sqrt', 'u_gs_sqrt'):
        g = rb[3][k]
        assert g.shape == b[k].shape and np.all(np.triu(g, 1) == 0.0) and np.any(np.tril(g, -1) != 0.0)


def test_negative_diagonal_entries():
    """The sign of a column of Lq does not change Lq Lq^T, so the model is the same: KL (log of the SQUARED diagonal, main.py:224),
    predict rows and the ELBO to 1e-12; the gradient of a flipped column flips with it.  And against the explicit model."""
    X, Y, p = make_problem(300, 30, 2, seed=8, Mg=19, ell=0.5)
    a = fr.make_lq(p, seed=3)
    b = dict(a)
    flip = {}
    for tag, cols in (('f', [0, 7, 29]), ('g', [3, 18])):
        k = 'u_%ss_sqrt' % tag
        sgn = np.ones(a[k].shape[0])
        sgn[cols] = -1.0
        b[k] = a[k] * sgn[None, :]
        flip[k] = sgn
        assert np.sum(np.diagonal(b[k]) < 0) == len(cols)
    jitter = 1e-6
    for i, (u, v) in enumerate(zip(fr.build_predict(X, a, jitter), fr.build_predict(X, b, jitter))):
        assert relerr(v, u) < 1e-12, i
    ra, rb = fr.elbo_and_grad(X, Y, a, jitter), fr.elbo_and_grad(X, Y, b, jitter)
    assert np.isfinite(rb[2]) and abs(ra[2] - rb[2]) <= 1e-12 * abs(ra[2]) and abs(ra[1] - rb[1]) <= 1e-12 * abs(ra[1])
    for k in ra[3]:
        want = ra[3][k] * flip[k][None, :] if k in flip else ra[3][k]
        assert relerr(rb[3][k], want) < 1e-10, k
    (fm, fv, gm, gv), kl = fr.explicit_full_cov(X, b, jitter)
    out = fr.build_predict(X, b, jitter)
    assert relerr(out[4], fv) < 1e-9 and relerr(out[6], gv) < 1e-9 and abs(rb[2] - kl) <= 1e-9 * abs(kl)


def test_autograd_gradients_match_central_differences():
    """As test_cpu_whiten_ref.py: every block along random directions, relative step 1e-6, bound 1e-5."""
    X, Y, p = make_problem(400, 24, 2, seed=9, Mg=17, ell=0.5)
    p = fr.make_lq(p, seed=4, negative=2)
    jitter, scale = 1e-6, 1.4
    _, _, _, g = fr.elbo_and_grad(X, Y, p, jitter, scale=scale, g_offset=-0.5)
    rs = np.random.RandomState(0)
    for k in g:
        v = np.asarray(p[k], dtype=np.float64)
        d = rs.randn(*v.shape) if v.ndim else np.float64(1.0)
        h = 1e-6 * max(1.0, float(np.max(np.abs(v))))
        vals = []
        for sgn in (1.0, -1.0):
            q = dict(p)
            q[k] = v + sgn * h * d
            vals.append(fr.elbo_and_grad(X, Y, q, jitter, scale=scale, g_offset=-0.5, need_grad=False)[0])
        fd = (vals[0] - vals[1]) / (2 * h)
        an = float(np.sum(np.asarray(g[k]).reshape(np.shape(d)) * d))
        print('%-10s autograd %.8e central %.8e' % (k, an, fd))
        assert abs(an - fd) <= 1e-5 * max(abs(fd), abs(an), 1e-3 * abs(vals[0])), k
