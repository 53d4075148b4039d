"""GPU parity of the Kronecker path and its heads with Matern 3/2 and 5/2 FACTORS (zigp_set_kron_kernel; p['kern_f'] / p['kern_g'] as a
name or a pair per factor), against tests/kron_matern_ref.py -- the oracle's literal dense order with a kernel kind per factor.

Fixtures: kron_matern_ref.FIXTURES, cases of kron_nd.CASES with mixed kinds, every (kind0, kind1) pair on some latent;
tests/test_cpu_kron_matern.py holds the reference's own floor on each at 1e-8 and cond(K_p + 1e-5 I) at 1e5, which is what makes the
project's relative tolerance of 1e-6 valid here.  Every test prints its figures (pytest -s; profiles/kron_matern_parity.log keeps a run's)."""
import functools
import math

import numpy as np
import pytest

import kron_nd
import kron_matern_ref as kmr
import kronpaths_ref as kr
import paths_ref as pr
from conftest import relerr
from test_gpu_kron_nd import _bit_identical, _check_grads, KERN_KEYS, VEC_KEYS, PRED_NAMES

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)]
TOL = 1e-6
J = kron_nd.JITTER
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def _ref_grad(name):
    X, Y, p = kmr.fixture(name)
    return kmr.kron_elbo_and_grad(X, Y, p, J, scale=kron_nd.case_scale(name), g_offset=-0.5, f_mu=0.2)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(kmr.FIXTURES))
def test_predict_elbo_and_gradient_match_the_restatement(engine, name):
    """kron_predict (g_offset 0 and -1, an f_mu), kron_elbo value, KL and every gradient block -- the Z and lengthscale blocks also per
    input dimension -- at 1e-6; the value-only call and the call without the KL return the gradient call's data term bit for bit."""
    X, Y, p = kmr.fixture(name)
    for goff, fmu in ((0.0, None), (-1.0, 0.3)):
        out = engine.kron_predict(p, X, jitter=J, g_offset=goff, f_mu=fmu)
        ref = kmr.kron_build_predict(X, p, J, goff, fmu)
        errs = [relerr(out[i], ref[i]) for i in range(9)]
        print('%s f %s g %s g_offset %g: %s' % (name, p['kern_f'], p['kern_g'], goff, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs))))
        assert max(errs) < TOL, (name, goff, errs)
    scale = kron_nd.case_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2)
    e_r, d_r, kl_r, g_r = _ref_grad(name)
    print('%s elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e' % (name, ed - kl, e_r, abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r)))
    assert abs(ed - scale * d_r) <= TOL * abs(scale * d_r)
    assert abs(kl - kl_r) <= TOL * abs(kl_r)
    worst = _check_grads(name, kron_nd.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS + ('f_mu',), tol=TOL)
    print('%s worst gradient figure %.2e' % (name, worst))
    v = engine.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2, need_grad=False)
    assert v[0] == ed and v[1] == kl and v[2] is None
    nk = engine.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2, include_kl=False, need_grad=False)
    assert nk[0] == ed and nk[1] == 0.0


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('name', ['d21-12', 'd31', 'p43', 'L32'])
def test_heads_match_the_restatement(engine, name, lik):
    X, Y, p = kmr.fixture(name)
    Y = (Y > 0) * 1.0 if lik == 'bernoulli' else Y
    hp = dict(kron_nd.head_params(p), kern_f=p['kern_f'])
    f_mu = 0.0 if lik == 'gaussian' else 0.2
    out = engine.kron_head_predict(hp, X, lik, jitter=J, f_mu=f_mu)
    ref = kmr.kron_head_predict(X, hp, lik, J, f_mu)
    errs = [relerr(out[i], ref[i]) for i in range(4)]
    print('%s %s f %s predict fmean %.1e fvar %.1e pfmean %.1e pfvar %.1e' % ((name, lik, hp['kern_f']) + tuple(errs)))
    assert max(errs) < TOL
    scale = kron_nd.case_scale(name)
    ed, kl, g = engine.kron_head_elbo(hp, X, Y, lik, jitter=J, scale=scale, f_mu=f_mu)
    e_r, d_r, kl_r, g_r = kmr.kron_head_elbo_and_grad(X, Y, hp, lik, J, scale=scale, f_mu=f_mu)
    assert abs(ed - scale * d_r) <= TOL * abs(scale * d_r) and abs(kl - kl_r) <= TOL * abs(kl_r)
    _check_grads('%s %s' % (name, lik), kron_nd.CASES[name]['D'], g, g_r, ('Zf', 'ell_f', 'var_f'),
                 ('u_fm', 'u_fs_sqrt', 'f_mu') + (('noise',) if lik == 'gaussian' else ()), tol=TOL)
    v = engine.kron_head_elbo(hp, X, Y, lik, jitter=J, scale=scale, f_mu=f_mu, need_grad=False)
    assert v[0] == ed and v[1] == kl


def test_matern_time_factor_moves_fmean_and_matches_the_restatement(engine):
    """d21-12 with a Matern-3/2 TIME factor on f: fmean differs from the RBF result by far more than the tolerance (a build that drops
    kern_f returns the RBF numbers and fails here) and is the restatement's."""
    X, Y, p = kron_nd.problem('d21-12')
    q = kmr.with_kinds(p, ('rbf', 'matern32'))
    rbf = engine.kron_predict(p, X, jitter=J)
    mat = engine.kron_predict(q, X, jitter=J)
    ref = kmr.kron_build_predict(X, q, J)
    moved = relerr(mat[3], rbf[3])
    print('d21-12 Matern32 time factor: fmean moves by %.2e of its size; against the restatement %.1e' % (moved, relerr(mat[3], ref[3])))
    assert moved > 1e3 * TOL
    assert relerr(mat[3], ref[3]) < TOL and relerr(mat[4], ref[4]) < TOL
    engine.set_kron_panels(True)      # the Matern call ran on the panels (d21-12 alone would run fused): g kept its RBF factors there
    try:
        rbf_panels = engine.kron_predict(p, X, jitter=J)
    finally:
        engine.set_kron_panels(False)
    assert np.array_equal(mat[5], rbf_panels[5]) and np.array_equal(mat[6], rbf_panels[6])      # the same launches for g: the same bits
    engine.kron_predict(q, X, jitter=J)
    assert engine.get_kron_kernel('f', 1) == 'matern32' and engine.get_kron_kernel('f', 0) == 'rbf' and engine.get_kron_kernel('g', 1) == 'rbf'
    assert np.array_equal(engine.kron_predict(p, X, jitter=J), rbf)                 # and the kinds of the last call do not leak
    assert engine.get_kron_kernel('f', 1) == 'rbf'


def test_rows_of_the_resident_set_equal_host_rows(engine):
    for name in ('d21-mix', 'p43'):
        X, Y, p = kmr.fixture(name)
        N = X.shape[0]
        engine.set_data(X, Y)
        for lo, hi in ((0, N), (5, N - 3), (7, 7)):
            a = engine.kron_elbo(p, X[lo:hi], Y[lo:hi], jitter=J, scale=2.5)
            b = engine.kron_elbo(p, rows=(lo, hi), jitter=J, scale=2.5)
            _bit_identical(a, b)
        hp = dict(kron_nd.head_params(p), kern_f=p['kern_f'])
        _bit_identical(engine.kron_head_elbo(hp, X[5:N - 3], Y[5:N - 3], 'gaussian', jitter=J, scale=2.5),
                       engine.kron_head_elbo(hp, lik='gaussian', rows=(5, N - 3), jitter=J, scale=2.5))
        assert a[0] == 0.0 and a[1] != 0.0      # the empty row set: no data term, the KL as usual
        st = engine.kron_stepper(p)
        _bit_identical(st(p, rows=(5, N - 3), jitter=J, scale=2.5), engine.kron_elbo(p, rows=(5, N - 3), jitter=J, scale=2.5))


@pytest.mark.parametrize('name', ['d21-12', 'L32'])
def test_two_shards_add_up(engine, name):
    """two uneven shards, the KL counted once, against the whole batch: the bounds of test_gpu_kron_nd.py::test_shard_additivity_many_tiles"""
    X, Y, p = kmr.fixture(name)
    cut = 131
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=J, scale=1.0)
    a = engine.kron_elbo(p, X[:cut], Y[:cut], jitter=J, scale=1.0, include_kl=True)
    b = engine.kron_elbo(p, X[cut:], Y[cut:], jitter=J, scale=1.0, include_kl=False)
    print('%s shards vs whole: value %.1e' % (name, abs((a[0] + b[0]) - ed) / abs(ed)))
    assert abs((a[0] + b[0]) - ed) <= 1e-11 * abs(ed) and a[1] == kl and b[1] == 0.0
    for k in VEC_KEYS:
        s_ = np.asarray(a[2][k]) + np.asarray(b[2][k])
        assert np.max(np.abs(s_ - np.asarray(g[k]))) <= 1e-9 * max(np.max(np.abs(np.asarray(g[k]))), 1e-300), k
    for k in KERN_KEYS:
        for q in range(2):
            s_ = np.asarray(a[2][k][q]) + np.asarray(b[2][k][q])
            ref = np.asarray(g[k][q])
            assert np.max(np.abs(s_ - ref)) <= 1e-8 * max(np.max(np.abs(ref)), 1e-300), (k, q)


def test_routing_is_by_kind_not_by_switch(engine):
    """d11 is a grid the fused kernels cover: with a Matern factor the call runs on the panels by itself, so set_kron_panels changes no bit;
    the fused-step hook refuses the step with its own text; with every kind RBF the same grid runs fused again."""
    X, Y, p = kmr.fixture('d11')
    a = engine.kron_elbo(p, X, Y, jitter=J, scale=3.0)
    pa = engine.kron_predict(p, X, jitter=J, g_offset=-1.0)
    with pytest.raises(ValueError, match='does not run on the fused Kronecker kernels'):
        engine.set_kron_kernel('g', 1, 'matern32')
        engine.test_kron_fused_step(kron_nd.problem('d11')[2], X, Y, taps=False)
    engine.set_kron_panels(True)
    try:
        b = engine.kron_elbo(p, X, Y, jitter=J, scale=3.0)
        pb = engine.kron_predict(p, X, jitter=J, g_offset=-1.0)
    finally:
        engine.set_kron_panels(False)
    _bit_identical(a, b)
    assert np.array_equal(pa, pb)
    for t in 'fg':
        for q in (0, 1):
            engine.set_kron_kernel(t, q, 'rbf')
    r = engine.test_kron_fused_step(kron_nd.problem('d11')[2], X, Y, taps=False)
    assert np.isfinite(r['elbo_data'])


def test_all_rbf_equals_a_fresh_context_bit_for_bit(engine):
    """after Matern calls on this context, RBF calls -- kinds absent, named 'rbf', or given as pairs -- return what a context that never
    saw a Matern factor returns: elbo, predict, both heads, the paths"""
    from zigp.engine import DenseEngine
    X, Y, p = kron_nd.problem('d21-12')
    Xp, Yp, pp = kron_nd.problem('p43')
    hp = kron_nd.head_params(p)
    d = kr.model_draws('d21-12')

    def calls(e, q, qp, hq):
        return (e.kron_elbo(q, X, Y, jitter=J, scale=2.0), e.kron_elbo(qp, Xp, Yp, jitter=J, scale=2.0),
                e.kron_predict(q, X, jitter=J, g_offset=-1.0), e.kron_predict(qp, Xp, jitter=J),
                e.kron_head_elbo(hq, X, Y, 'gaussian', jitter=J), e.kron_head_predict(hq, X, 'bernoulli', jitter=J, f_mu=0.2),
                e.kron_sample_paths(q, X, n_samples=kr.MODEL_S, draws=d, jitter=J, g_offset=-1.0))

    fresh = DenseEngine(device=0)
    try:
        want = calls(fresh, p, pp, hp)
    finally:
        fresh.close()
    mq = kmr.fixture('d21-12')[2]
    engine.kron_elbo(mq, X, Y, jitter=J)
    engine.kron_head_predict(dict(hp, kern_f='matern52'), X, 'gaussian', jitter=J)
    engine.kron_sample_paths(mq, X, n_samples=kr.MODEL_S, draws=d, jitter=J)
    for q, qp, hq in ((p, pp, hp), (kmr.with_kinds(p, 'rbf', 'rbf'), kmr.with_kinds(pp, ('rbf', 'rbf'), 'RBF'), dict(hp, kern_f=('rbf', 'rbf')))):
        got = calls(engine, q, qp, hq)
        _bit_identical(got[0], want[0]); _bit_identical(got[1], want[1]); _bit_identical(got[4], want[4])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[5], want[5])
        for k in ('f', 'g', 'gf'):
            assert np.array_equal(got[6][k], want[6][k]), k
        engine.kron_predict(mq, X, jitter=J)


def test_fit_loops_refuse_by_name_and_the_context_stays_usable(engine):
    import ctypes as C
    from zigp import _lib
    from zigp.engine import ZigpError  # noqa: F401
    X, Y, p = kron_nd.fit_problem('d31')
    engine.set_data(X, Y)
    base = engine.kron_elbo(p, rows=(0, 500), jitter=J, scale=6.0)
    shape = dict(M0f=6, M1f=5, M0g=6, M1g=5, D0=3, D1=1)
    n = 2 * (6 * 3 + 5 * 1 + 2 * 30 + 3 + 1 + 2) + 1
    x, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    # the engine refuses before the library is touched, with the library's naming
    with pytest.raises(ValueError, match='Matern52 kernel on factor 1 of latent f'):
        engine.kron_fit_steps(dict(shape, kern_f=('rbf', 'matern52')), x, m, v, [1e-3] * 17, [0] * 17, 0, [0, 500], 500, jitter=J)
    with pytest.raises(ValueError, match='Matern32 kernel on factor 0 of latent f'):
        engine.kron_head_fit_steps(dict(shape, kern_f='matern32'), 'gaussian', x[:91], m[:91], v[:91], [1e-3] * 10, [0] * 10, [1] * 10, 0, [0], 500, jitter=J)
    # and so does the library: the C refusals
    lib, ctx = engine.lib, engine.ctx
    s = _lib.zigp_kron_params()
    for k, val in shape.items():
        setattr(s, k, val)
    o = _lib.zigp_kron_fit_opts()
    o.beta1, o.beta2, o.eps = 0.9, 0.999, 1e-8
    rb = np.zeros(1, dtype=np.int64)
    ed, kl = np.full(1, 7.0), np.full(1, 7.0)
    engine.set_kron_kernel('g', 0, 'matern32')
    rc = lib.zigp_kron_fit_steps(ctx, C.byref(s), C.byref(o), x.ctypes.data, m.ctypes.data, v.ctypes.data, n, 0, 1, rb.ctypes.data, 500, None, None,
                                 J, 6.0, 1, ed.ctypes.data, kl.ctypes.data)
    msg = lib.zigp_last_error(ctx).decode()
    assert rc == _lib.ZIGP_EARG and 'zigp_kron_fit_steps' in msg and 'Matern32 kernel on factor 0 of latent g' in msg, msg
    assert not x.any() and ed[0] == 7.0 and lib.zigp_kron_fit_steps_applied(ctx) == 0
    ho = _lib.zigp_kron_head_fit_opts()
    ho.beta1, ho.beta2, ho.eps = 0.9, 0.999, 1e-8
    # the head fits f only: a Matern factor on g does not concern it (it fails later, on n_free); one on f is named
    engine.set_kron_kernel('f', 1, 'matern52')
    rc = lib.zigp_kron_head_fit_steps(ctx, C.byref(s), _lib.LIK_GAUSSIAN, C.byref(ho), x.ctypes.data, m.ctypes.data, v.ctypes.data, 91, 0, 1, rb.ctypes.data,
                                      500, None, None, J, 6.0, 1, ed.ctypes.data, kl.ctypes.data)
    msg = lib.zigp_last_error(ctx).decode()
    assert rc == _lib.ZIGP_EARG and 'zigp_kron_head_fit_steps' in msg and 'Matern52 kernel on factor 1 of latent f' in msg, msg
    # argument checks of the setter name the argument
    for args, word in (((2, 0, 0), 'latent'), ((0, 2, 0), 'factor'), ((0, 0, 3), 'kind'), ((0, 0, -1), 'kind')):
        assert lib.zigp_set_kron_kernel(ctx, *args) == _lib.ZIGP_EARG and word in lib.zigp_last_error(ctx).decode()
    assert lib.zigp_set_kron_kernel(None, 0, 0, 0) == _lib.ZIGP_EARG and lib.zigp_get_kron_kernel(ctx, 0, 2) == _lib.ZIGP_EARG
    assert engine.get_kron_kernel('f', 1) == 'matern52' and engine.get_kron_kernel(1, 0) == 'matern32'
    with pytest.raises(ValueError):
        engine.set_kron_kernel('f', 0, 'matern12')
    # the context answers a following RBF call as before
    _bit_identical(engine.kron_elbo(p, rows=(0, 500), jitter=J, scale=6.0), base)


# ---- paths ------------------------------------------------------------------------------------------------------------------------------
def _factor(kind, X, Z, ell, var, dt=np.float64):
    """(k (N, M), s (N, M)) of one factor from direct differences in `dt`: s is the element's relative first-order sensitivity to the
    roundings of r2 -- (K' / K) c / 2 with c = r2 + 2 sum_d |t_d| (|z_d| + |x_d|) / ell_d (tests/test_gpu_kron_matern_stages.py); for the
    RBF kind the exponent r2 / 2, as kronpaths_ref.factor_np states it"""
    f = lambda a: np.asarray(a, dtype=dt)
    ell = f(ell).reshape(1, 1, -1)
    d = (f(Z)[None, :, :] - f(X)[:, None, :]) / ell
    r2 = np.sum(d * d, 2)
    if kind == 'rbf':
        return dt(var) * np.exp(-r2 / 2), r2 / 2
    c = r2 + 2 * np.sum(np.abs(d) * (np.abs(f(Z))[None, :, :] + np.abs(f(X))[:, None, :]) / ell, 2)
    r = np.sqrt(r2 + dt(1e-12))
    if kind == 'matern32':
        t = np.sqrt(dt(3.0)) * r
        return dt(var) * (1 + t) * np.exp(-t), dt(3.0) / (1 + t) * c / 2
    t = np.sqrt(dt(5.0)) * r
    poly = 1 + t + dt(5.0) / dt(3.0) * r * r
    return dt(var) * poly * np.exp(-t), dt(5.0) / dt(3.0) * (1 + t) / poly * c / 2


def _path_sum_np(lat, X, dt=np.float64):
    """kronpaths_ref.kron_path_sum_np with the latent's kinds: (out (S, N), mag (S, N))"""
    kinds = kmr.pair_of(lat.get('kinds', 'rbf'))
    X = np.asarray(X, dtype=dt)
    D0 = np.shape(lat['Z'][0])[1]
    e0, e1 = kr._ells(lat, dt)
    v0, v1 = kr._vars(lat)
    k0, a0 = _factor(kinds[0], X[:, :D0], lat['Z'][0], e0, v0, dt)
    k1, a1 = _factor(kinds[1], X[:, D0:], lat['Z'][1], e1, v1, dt)
    M0, M1 = k0.shape[1], k1.shape[1]
    V = np.asarray(lat['V'], dtype=dt).reshape(M0, M1, -1)
    out = np.einsum('ni,nj,ijs->ns', k0, k1, V)
    Va = np.abs(V)
    mag = np.einsum('ni,nj,ijs->ns', k0 * (1 + a0), k1, Va) + np.einsum('ni,nj,ijs->ns', k0, k1 * a1, Va)
    phase = np.asarray(lat['phase'], dtype=dt).reshape(-1)
    if phase.size:
        om, amp = np.asarray(lat['omega'], dtype=dt), np.asarray(lat['amp'], dtype=dt)
        c = np.cos(X @ om.T + phase[None, :])
        out = out + c @ amp
        mag = mag + (np.abs(c) * (1.0 + np.abs(X) @ np.abs(om).T + np.abs(phase)[None, :])) @ np.abs(amp)
    shift = dt(float(lat.get('shift', 0.0)))
    return (out + shift).T, (mag + abs(shift)).T


def _path_sum_mp(lat, X, rows, cols):
    """the sum at rows x cols in 50-digit arithmetic from the doubles as given (kronpaths_ref.kron_path_sum_mp with the kinds)"""
    import mpmath as mp
    kinds = kmr.pair_of(lat.get('kinds', 'rbf'))
    X = np.asarray(X, dtype=np.float64)
    Z0, Z1 = np.asarray(lat['Z'][0]), np.asarray(lat['Z'][1])
    D0, D1 = Z0.shape[1], Z1.shape[1]
    e0, e1 = kr._ells(lat)
    v0, v1 = kr._vars(lat)
    M0, M1 = Z0.shape[0], Z1.shape[0]
    V = np.asarray(lat['V']).reshape(M0, M1, -1)
    phase = np.asarray(lat['phase']).reshape(-1)
    R = phase.size
    om = np.asarray(lat['omega']).reshape(R, D0 + D1) if R else None
    amp = np.asarray(lat['amp']) if R else None
    out = np.zeros((len(cols), len(rows)))
    with mp.workdps(50):
        def fac(kind, x, Z, ell, var):
            el = [mp.mpf(float(v)) for v in ell]
            res = []
            for z in Z:
                r2 = mp.fsum(((mp.mpf(float(z[d])) - x[d]) / el[d]) ** 2 for d in range(len(el)))
                if kind == 'rbf':
                    res.append(mp.mpf(var) * mp.exp(-r2 / 2))
                    continue
                r = mp.sqrt(r2 + mp.mpf(1e-12))
                if kind == 'matern32':
                    t = mp.sqrt(3) * r
                    res.append(mp.mpf(var) * (1 + t) * mp.exp(-t))
                else:
                    t = mp.sqrt(5) * r
                    res.append(mp.mpf(var) * (1 + t + mp.mpf(5) / 3 * r * r) * mp.exp(-t))
            return res
        for jn, n in enumerate(rows):
            x = [mp.mpf(float(v)) for v in X[n]]
            k0, k1 = fac(kinds[0], x[:D0], Z0, e0, v0), fac(kinds[1], x[D0:], Z1, e1, v1)
            cs = [mp.cos(mp.fsum(mp.mpf(float(om[r, d])) * x[d] for d in range(D0 + D1)) + mp.mpf(float(phase[r]))) for r in range(R)]
            for js, s in enumerate(cols):
                acc = mp.mpf(float(lat.get('shift', 0.0)))
                for i in range(M0):
                    acc += k0[i] * mp.fdot([mp.mpf(float(v)) for v in V[i, :, s]], k1)
                if R:
                    acc += mp.fdot([mp.mpf(float(v)) for v in amp[:, s]], cs)
                out[js, jn] = float(acc)
    return out


# grid(s), dims, R, S, N, kinds per latent, sampled rows x cols.  S = 1 and 16: one sample tile a pass; 17 and 40: two; 64: four.  1 x 1;
# 3 x 5 (M1 no multiple of 4); 32 x 32 (two row tiles a wave, four waves); 10 x 100 (one row tile, four waves); 128 x 128 at N = 17 (one
# row tile, two waves); a pair of latents with different kinds, one of them RBF x RBF inside a launch of the kinds kernel.
PATH_CASES = {
    '1x1': ([(1, 1)], (1, 1), 0, 1, 1, [('matern32', 'matern52')], 1, 1),
    '3x5': ([(3, 5)], (2, 1), 7, 17, 33, [('rbf', 'matern32')], 6, 6),
    '32x32': ([(32, 32)], (1, 7), 64, 64, 129, [('matern52', 'matern32')], 6, 6),
    '10x100': ([(10, 100)], (2, 1), 7, 40, 129, [('matern52', 'rbf')], 5, 5),
    '128x128': ([(128, 128)], (2, 1), 0, 3, 17, [('matern32', 'rbf')], 3, 3),
    'pair': ([(3, 7), (10, 12)], (2, 1), 9, 16, 300, [('rbf', 'rbf'), ('matern52', 'matern52')], 6, 5),
}


@pytest.mark.parametrize('name', list(PATH_CASES))
def test_path_kernel_against_50_digits(engine, name, monkeypatch):
    """zigp_kron_path_rows with per-record kinds under the point-wise rule err_gpu <= 4 err_np + 16 eps S at sampled elements, and the whole
    block against NumPy; the result does not depend on the sample tiles a pass (ZIGP_PATH_TILES 1, 2, 4)."""
    grids, dims, R, S, N, kinds, n_rows, n_cols = PATH_CASES[name]
    rs = np.random.RandomState(8100 + list(PATH_CASES).index(name))
    lats = [dict(kr.random_latent(rs, g[0], g[1], dims[0], dims[1], R, S, shift=0.3 - h), kinds=kinds[h]) for h, g in enumerate(grids)]
    X = rs.rand(N, dims[0] + dims[1])
    out = engine.kron_path_rows(lats, X, S, dims)
    assert out.shape == (len(lats), S, N) and np.all(np.isfinite(out))
    rows, cols = pr.pick(N, n_rows), pr.pick(S, n_cols)
    for h, lat in enumerate(lats):
        ref_np, mag = _path_sum_np(lat, X)
        ref_mp = _path_sum_mp(lat, X, rows, cols)
        ix = np.ix_(cols, rows)
        ratio, excess = kr.pointwise_ratio(out[h][ix], ref_np[ix], ref_mp, mag[ix])
        print('%s latent %d %s: %d elements, largest err_gpu / (eps S) = %.3f' % (name, h, kinds[h], len(rows) * len(cols), ratio))
        assert excess <= 0.0
        n_terms = grids[h][0] * grids[h][1] + R + 8
        assert np.all(np.abs(out[h] - ref_np) <= (16 + n_terms) * kr.EPS * mag)
        if kinds[h] != ('rbf', 'rbf'):
            assert not np.array_equal(out[h], engine.kron_path_rows([dict(lat, kinds='rbf')], X, S, dims)[0]) or R == 0 and not lat['V'].any()
    for cap in ('1', '2', '4'):
        monkeypatch.setenv('ZIGP_PATH_TILES', cap)
        assert np.array_equal(engine.kron_path_rows(lats, X, S, dims), out), cap
    monkeypatch.delenv('ZIGP_PATH_TILES')
    if name == 'pair':      # the RBF x RBF latent inside the kinds launch has the bits of the RBF kernel
        assert np.array_equal(engine.kron_path_rows([lats[0]], X, S, dims)[0], out[0])
        import ctypes as C
        recs, keep = engine._kron_path_latents(lats, dims, S)
        recs[1].reserved = 3
        o2 = np.zeros_like(out)
        rc = engine.lib.zigp_kron_path_rows(engine.ctx, C.cast(recs, C.c_void_p), 2, dims[0], dims[1], S, X.ctypes.data, N, o2.ctypes.data)
        assert rc == -1 and b'kinds = 3' in engine.lib.zigp_last_error(engine.ctx)


def _matrices(p, tag, jitter, dt=np.float64):
    kinds = kmr.kinds_of(p)['fg'.index(tag)]
    out = []
    for q in range(2):
        Z = np.asarray(p['Z' + tag][q])
        ell = np.broadcast_to(np.asarray(p['ell_' + tag][q], dtype=np.float64).reshape(-1), (Z.shape[1],))
        out.append(_factor(kinds[q], Z, Z, ell, float(np.squeeze(p['var_' + tag][q])), dt)[0] + dt(jitter) * np.eye(Z.shape[0], dtype=dt))
    return out


def _path_bound(p, tags, jitter):
    """kronpaths_ref.path_bound on the factor matrices of p's kinds: min(max(1e-9, 1e-13 c), 1e-6), c = cond(K0) cond(K1)"""
    c = 0.0
    for t in tags:
        K0, K1 = _matrices(p, t, jitter)
        c = max(c, float(np.linalg.cond(K0) * np.linalg.cond(K1)))
    return min(max(1e-9, 1e-13 * c), 1e-6), c


def _tables(p, tag, draw, jitter):
    """kronpaths_ref.kron_latent_tables with Matern K_p: the latent dict zigp_kron_sample_paths forms (zigp.pathwise.kron_weights_np)"""
    from zigp import pathwise
    Z = [np.asarray(p['Z' + tag][0]), np.asarray(p['Z' + tag][1])]
    D = [Z[0].shape[1], Z[1].shape[1]]
    ell = [np.broadcast_to(np.asarray(p['ell_' + tag][q], dtype=np.float64).reshape(-1), (D[q],)).copy() for q in range(2)]
    var = [float(np.squeeze(p['var_' + tag][q])) for q in range(2)]
    R, S = int(draw['R']), np.shape(draw['eps'])[1]
    omega = np.asarray(draw['omega0']).reshape(R, D[0] + D[1]) / np.concatenate(ell)[None, :]
    amp = np.asarray(draw['a']).reshape(R, S) * (math.sqrt(2.0 * var[0] * var[1] / R) if R else 0.0)
    G = pathwise.kron_grid(Z[0], Z[1])
    fZ = (np.cos(G @ omega.T + np.asarray(draw['phase'])[None, :]) @ amp) if R else np.zeros((G.shape[0], S))
    K0, K1 = _matrices(p, tag, jitter)
    V = pathwise.kron_weights_np(K0, K1, p['u_%sm' % tag], p['u_%ss_sqrt' % tag], draw['eps'], fZ)
    return dict(Z=Z, ell=ell, var=var, V=V, omega=omega, phase=np.asarray(draw['phase']), amp=amp, kinds=kmr.kinds_of(p)['fg'.index(tag)])


@functools.lru_cache(maxsize=None)
def _draws(name):
    """seeded kron_draw of a fixture with its kinds (R = 200, S = 20): computed once, shared, never written to"""
    from zigp import pathwise
    X, Y, p = kmr.fixture(name)
    D0, D1 = kron_nd.CASES[name]['D']
    rs = np.random.RandomState(4100 + list(kmr.FIXTURES).index(name))
    return {t: pathwise.kron_draw(kmr.kinds_of(p)['fg'.index(t)], kr.MODEL_R, D0, D1, p['Z' + t][0].shape[0], p['Z' + t][1].shape[0], kr.MODEL_S, rs)
            for t in 'fg'}


@pytest.mark.parametrize('name', ['d21-12', 'd21-mix', 'd31'])
def test_sample_paths_zero_and_real_draws(engine, name):
    """zero draws: every path is kron_predict's fmean / gmean; real draws (kron_draw with the fixture's kinds): f, g, gf against the NumPy
    restatement (kron_weights_np on Matern K_p) -- both under the path bound of tests/test_gpu_kron_paths.py on the factor matrices of these
    kinds; host and device calls agree bit for bit; the heads follow the f kinds."""
    import torch
    X, Y, p = kmr.fixture(name)
    d = _draws(name)
    bound, c = _path_bound(p, 'fg', J)
    z = pr.zero_draws(d)
    got = engine.kron_sample_paths(p, X, n_samples=kr.MODEL_S, draws=z, jitter=J, g_offset=-1.0, f_mu=0.7)
    ref = engine.kron_predict(p, X, jitter=J, g_offset=-1.0, f_mu=0.7)
    ef = max(kr.plane_err(got['f'][s], ref[3]) for s in range(kr.MODEL_S))
    eg = max(kr.plane_err(got['g'][s], ref[5]) for s in range(kr.MODEL_S))
    print('%s zero draws: cond product %.2e, bound %.2e, f %.2e, g %.2e' % (name, c, bound, ef, eg))
    assert ef <= bound and eg <= bound
    got = engine.kron_sample_paths(p, X, n_samples=kr.MODEL_S, draws=d, jitter=J, g_offset=-1.0, f_mu=0.25)
    lf, lg = _tables(p, 'f', d['f'], J), _tables(p, 'g', d['g'], J)
    lf['shift'], lg['shift'] = 0.25, -1.0
    f, g = _path_sum_np(lf, X)[0], _path_sum_np(lg, X)[0]
    want = dict(f=f, g=g, gf=pr.link(g) * f)
    errs = {k: kr.plane_err(got[k], want[k]) for k in ('f', 'g', 'gf')}
    print('%s real draws: bound %.2e, f %.2e, g %.2e, gf %.2e' % (name, bound, errs['f'], errs['g'], errs['gf']))
    assert max(errs.values()) <= bound
    assert np.min(np.std(got['f'], axis=0)) > 0
    dev = engine.kron_sample_paths_device(p, torch.from_numpy(np.array(X)).cuda(), n_samples=kr.MODEL_S, draws=d, jitter=J, g_offset=-1.0, f_mu=0.25)
    for k in ('f', 'g', 'gf'):
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k
    hp = dict(kron_nd.head_params(p), kern_f=p['kern_f'])
    hb, _ = _path_bound(p, 'f', J)
    h = engine.kron_head_sample_paths(hp, X, 'bernoulli', n_samples=kr.MODEL_S, draws={'f': d['f']}, jitter=J, f_mu=0.25)
    assert kr.plane_err(h['f'], f) <= hb and np.array_equal(h['f'], got['f'])
    # seeded draws made by the engine follow the kinds: the same seed gives kron_draw's arrays
    auto = engine.kron_sample_paths(p, X[:20], n_samples=3, n_features=16, rng=5, jitter=J)['draws']
    from zigp import pathwise
    rs = np.random.RandomState(5)
    for t in 'fg':
        w = pathwise.kron_draw(kmr.kinds_of(p)['fg'.index(t)], 16, kron_nd.CASES[name]['D'][0], kron_nd.CASES[name]['D'][1], p['Z' + t][0].shape[0],
                               p['Z' + t][1].shape[0], 3, rs)
        assert all(np.array_equal(auto[t][k], w[k]) for k in ('omega0', 'phase', 'a', 'eps'))


def test_path_scores_on_the_device_equal_ensemble_scores_of_the_fetched_paths(engine):
    """kron_path_scores_device with Matern kinds: its scores are ensemble_scores of the paths kron_sample_paths returns for the same draws,
    bit for bit (the protocol of tests/test_gpu_ensemble.py for the RBF model)"""
    import torch
    from test_gpu_ensemble import KEYS, _bits
    X, Y, p = kmr.fixture('d21-12')
    X = np.array(X)
    y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
    N = X.shape[0]
    X_t, Y_t = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    off = np.array([0, N // 3, N // 3, N])
    r = engine.kron_path_scores_device(p, X_t, Y_t, groups=off, n_samples=16, variogram=0.5, return_dist=True, rng=7, jitter=J, g_offset=-1.0)
    paths = engine.kron_sample_paths(p, X, n_samples=16, draws=r['draws'], jitter=J, g_offset=-1.0)
    h = engine.ensemble_scores(paths['gf'], y, groups=off, variogram=0.5, return_dist=True)
    for k in KEYS + ('variogram',):
        assert _bits(r[k].cpu().numpy(), h[k]), k
    rbf = engine.kron_sample_paths(kron_nd.problem('d21-12')[2], X, n_samples=16, draws=r['draws'], jitter=J, g_offset=-1.0)
    assert not np.array_equal(rbf['gf'], paths['gf'])


# ---- model surface ----------------------------------------------------------------------------------------------------------------------
def test_onoff_fit_with_a_matern_time_factor_checkpoint_and_predict(engine, tmp_path):
    """30 Adam steps of onoff(...) on a 6 x 5 grid with kernels=('rbf', 'matern32') -- the host loop, although device_loop=True, and the log
    says so once -- lower the cost; the checkpoint keeps the kinds and predict_onoff reproduces engine.kron_predict on the restored
    parameters bit for bit; a checkpoint without kinds (written before they existed) still predicts what it predicted."""
    import os
    from test_gpu_onofftf import _pptr
    from onofftf import onoff, predict_onoff
    from onofftf.model import init_params, engine_params, load_checkpoint, get_kernels
    from onofftf.main import KernMatern32, KernMatern52, KernSE
    Xtr, Ytr, Xte, Yte = _pptr()
    Xtr, Ytr = Xtr[:4000], Ytr[:4000]
    d = str(tmp_path) + '/'
    hist = []
    np.random.seed(0)
    onoff(Xtr, Ytr, Xte[:500], Yte[:500], d, num_iter=30, num_inducing_f=(6, 5), num_inducing_g=(6, 5), num_minibatch=1000, engine=engine,
          kmeans_seed=1, history=hist, device_loop=True, kernels=('rbf', 'matern32'))
    assert len(hist) == 30 and np.mean(hist[-5:]) < np.mean(hist[:5])
    log = open(os.path.join(d, 'modelsumm.log')).read()
    assert log.count('the host Adam loop runs') == 1 and 'matern32' in log
    pset = init_params(Xtr, (6, 5), (6, 5), init_noisevar=0.001)
    load_checkpoint(pset, os.path.join(d, 'model'))
    assert get_kernels(pset) == {'f': ('rbf', 'matern32'), 'g': ('rbf', 'matern32')}
    p = engine_params(pset)
    want = engine.kron_predict(p, Xte[:300], jitter=1e-6, g_offset=-1.0)
    ptr, pte = predict_onoff(Xtr[:200], Xte[:300], d, np.array([6, 5]), np.array([6, 5]), engine=engine)
    assert np.array_equal(pte['gfmean'][:, 0], want[0]) and np.array_equal(pte['fmean'][:, 0], want[3]) and np.array_equal(pte['pgmean'][:, 0], want[7])
    rbf = engine.kron_predict({k: v for k, v in p.items() if not k.startswith('kern_')}, Xte[:300], jitter=1e-6, g_offset=-1.0)
    assert relerr(want[3], rbf[3]) > 1e3 * TOL      # the kinds matter for this model
    # a checkpoint from before the kinds existed: the parameter arrays alone
    old = os.path.join(d, 'old')
    np.savez(old, **{k.replace('/', '__'): q.value for k, q in pset.params.items()})
    _, pold = predict_onoff(Xtr[:200], Xte[:300], old, np.array([6, 5]), np.array([6, 5]), engine=engine)
    assert np.array_equal(pold['fmean'][:, 0], rbf[3]) and np.array_equal(pold['gfmean'][:, 0], rbf[0])
    # the factor kernel objects
    Z, l = Xte[:40, 2:3], np.array([0.4])
    for cls, kind in ((KernMatern32, 'matern32'), (KernMatern52, 'matern52')):
        k = cls(l, np.array([1.3]))
        K = k.K(Z, Xte[:7, 2:3], engine=engine)
        assert relerr(K, kmr.factor_K_np(kind, Z, Xte[:7, 2:3], l, 1.3)) < 1e-12 and np.all(k.Kdiag(Z) == 1.3)
        assert np.all(np.diag(k.K(Z, engine=engine)) < 1.3)
    assert isinstance(KernMatern32(l, 1.0), KernSE)
