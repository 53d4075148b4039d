"""Pins tests/whiten_ref.py, the CPU restatement of the whitened parametrisation the GPU tests compare against (no GPU needed)."""
import numpy as np

from conftest import make_problem, relerr
import whiten_ref as wr


def _cond(p, tag, jitter):
    import zigp_oracle as o
    K = o.rbf_K(p['Z' + tag], None, p['ell_' + tag], p['var_' + tag]) + jitter * np.eye(p['Z' + tag].shape[0])
    return np.linalg.cond(K)


def test_equals_the_explicit_full_covariance_model():
    """q(u) = N(L u, L diag(s^2) L^T) pushed through the unwhitened full-covariance formulas with dense inverses: latent means and
    variances and the KL to 1e-9 relative.  The explicit inverse costs ~cond * eps, so the case is a well-conditioned one (D = 8, lengthscale 0.6:
    cond(Kuu) <= 1e5 for both latents, asserted)."""
    X, Y, p = make_problem(1300, 150, 8, seed=1450, Mg=100, ell=0.6)
    jitter = 1e-6
    cf, cg = _cond(p, 'f', jitter), _cond(p, 'g', jitter)
    print('cond(Kuu) f %.2e g %.2e' % (cf, cg))
    assert max(cf, cg) <= 1e5
    p['mean_a'], p['mean_b'] = np.linspace(-0.3, 0.4, 8), 0.25
    for g_off in (0.0, -1.0):
        out = wr.build_predict(X, p, jitter, g_off)
        (fm, fv, gm, gv), kl = wr.explicit_full_cov(X, p, jitter, g_off)
        for name, a, b in (('fmean', out[3], fm), ('fvar', out[4], fv), ('gmean', out[5], gm), ('gvar', out[6], gv)):
            e = relerr(a, b)
            print('  g_offset %+.0f %s relerr %.2e' % (g_off, name, e))
            assert e < 1e-9, (name, e)
    _, _, kl_w, _ = wr.elbo_and_grad(X[:8], Y[:8], p, jitter, need_grad=False)
    print('  KL %.12e explicit %.12e' % (kl_w, kl))
    assert abs(kl_w - kl) <= 1e-9 * abs(kl)


def test_one_inducing_point_equals_the_unwhitened_oracle():
    """M = 1: L is the scalar sqrt(k(z,z) + jitter), so the whitened model at (u, s) IS the unwhitened one at (u L, s L): predict rows, data
    term and KL against oracle/zigp_oracle_torch.py to 1e-12."""
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    jitter = 1e-6
    for D, seed in ((1, 3), (3, 4)):
        X, Y, p = make_problem(300, 1, D, seed=seed, ell=0.6)
        q = dict(p)
        for tag in ('f', 'g'):
            L = np.sqrt(p['var_' + tag] + jitter)
            q['u_%sm' % tag] = p['u_%sm' % tag] * L
            q['u_%ss_sqrt' % tag] = p['u_%ss_sqrt' % tag] * L
        out = wr.build_predict(X, p, jitter, -1.0)
        ref = o.build_predict(X, q, jitter, -1.0)
        for i in range(9):
            assert relerr(out[i], np.asarray(ref[i]).reshape(-1)) < 1e-12, i
        e_w, d_w, k_w, _ = wr.elbo_and_grad(X, Y, p, jitter, scale=1.3, need_grad=False)
        e_r, d_r, k_r, _ = ot.elbo_and_grad(X, Y, q, jitter, scale=1.3, need_grad=False)
        assert abs(d_w - d_r) <= 1e-12 * abs(d_r) and abs(k_w - k_r) <= 1e-12 * max(abs(k_r), 1.0) and abs(e_w - e_r) <= 1e-12 * abs(e_r)


def test_autograd_gradients_match_central_differences():
    """Every gradient block of elbo_and_grad against central differences of its own value along random directions (relative step 1e-6:
    truncation ~1e-12 |f'''|, rounding ~eps |ELBO| / step ~ 1e-7 of a directional derivative of the ELBO's own size -- bound 1e-5)."""
    X, Y, p = make_problem(400, 24, 2, seed=9, Mg=17, ell=0.5)
    p['mean_a'], p['mean_b'] = np.array([0.2, -0.1]), 0.3
    jitter, scale = 1e-6, 1.4
    _, _, _, g = wr.elbo_and_grad(X, Y, p, jitter, scale=scale, g_offset=-0.5)
    rs = np.random.RandomState(0)
    for k in g:
        v = np.asarray(p[k], dtype=np.float64)
        d = rs.randn(*v.shape) if v.ndim else np.float64(1.0)
        h = 1e-6 * max(1.0, float(np.max(np.abs(v))))
        vals = []
        for sgn in (1.0, -1.0):
            q = dict(p)
            q[k] = v + sgn * h * d
            vals.append(wr.elbo_and_grad(X, Y, q, jitter, scale=scale, g_offset=-0.5, need_grad=False)[0])
        fd = (vals[0] - vals[1]) / (2 * h)
        an = float(np.sum(np.asarray(g[k]).reshape(np.shape(d)) * d))
        print('%-10s autograd %.8e central %.8e' % (k, an, fd))
        assert abs(an - fd) <= 1e-5 * max(abs(fd), abs(an), 1e-3 * abs(vals[0])), k
