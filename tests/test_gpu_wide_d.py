"""End-to-end checks of the dense path at input dimensions 9 .. 64 (the run-time-D "wide" kernels): predict, ELBO, KL and gradients against
the CPU oracles with the bounds of tests/test_gpu_dense.py / test_gpu_whiten.py / test_gpu_fullcov.py, the three parametrisations,
translation invariance, inducing inputs spread over thousands of lengthscales, rbf_K, the refusals (D > 64; the device fit loops and
a Linear mean function above D = 8) and the model surface.  On the parent of this change every case ends in
ValueError('D must be in [1, 8]').

The lengthscales are set here: ell_f = ell (1 + 0.1 (d mod 5)), ell_g = 1.3 ell (1 + 0.05 (d mod 7)) -- the generator's own ramp makes
the late dimensions of a wide problem nearly flat.  Each reference is computed once per case and shared."""
import ctypes as C
import pickle

import numpy as np
import pytest

from conftest import make_problem, relerr

pytestmark = pytest.mark.gpu

# N, Mf, Mg, D, ell, chunk
CASES = [
    (1200, 96, 140, 9, 0.7, 1024),
    (1100, 130, 64, 16, 0.9, 1024),
    (1300, 64, 64, 17, 0.9, None),
    (2500, 128, 128, 24, 1.1, 1024),     # three passes, the last one short
    (1000, 140, 100, 33, 1.3, 1024),
    (900, 70, 200, 64, 1.8, None),
]
ROWS9 = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')
SCALE = 1.7


def wide_problem(N, Mf, Mg, D, ell, seed=None):
    X, Y, p = make_problem(N, Mf, D, seed=N + Mf if seed is None else seed, Mg=Mg, ell=ell)
    d = np.arange(D)
    p['ell_f'] = ell * (1 + 0.1 * (d % 5))
    p['ell_g'] = 1.3 * ell * (1 + 0.05 * (d % 7))
    return X, Y, p


def _cond(p, jitter=1e-6):
    import zigp_oracle as o
    K = o.rbf_K(p['Zf'], None, p['ell_f'], p['var_f']) + jitter * np.eye(p['Zf'].shape[0])
    return np.linalg.cond(K)


_cache = {}


def _case(case):
    if case not in _cache:
        import zigp_oracle as o
        import zigp_oracle_torch as ot
        N, Mf, Mg, D, ell, chunk = case
        X, Y, p = wide_problem(N, Mf, Mg, D, ell)
        _cache[case] = dict(X=X, Y=Y, p=p, cond=_cond(p), elbo=ot.elbo_and_grad(X, Y, p, 1e-6, scale=SCALE, chunk=1000),
                            predict={g: o.build_predict(X, p, 1e-6, g) for g in (0.0, -1.0)})
    return _cache[case]


def check_grads(tag, g, g_r, c, keys):
    """The per-block bound of tests/test_gpu_dense.py, and per DIMENSION for what has one: each column of dZ against that column's own
    largest reference entry, each dell entry against max(|ref_d|, 1e-3 block max) -- the per-dimension gradients of these cases differ by
    orders of magnitude, and a per-block check would hide a wrong dimension."""
    tol = max(1e-6, 1e-13 * c)
    for k in keys:
        a, b = np.asarray(g[k], dtype=float), np.asarray(g_r[k], dtype=float)
        a = a.reshape(b.shape) if a.size == b.size else a
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        print('  %s grad %-10s relerr %.2e (max |ref| %.3e)' % (tag, k, e, np.max(np.abs(b))))
        assert e < tol, (k, e)
        if k in ('Zf', 'Zg'):
            ec = np.max(np.abs(a - b), axis=0) / np.maximum(np.max(np.abs(b), axis=0), 1e-300)
            print('  %s grad %-10s worst column %d relerr %.2e; column maxima span %.1fx' % (
                tag, k, int(np.argmax(ec)), ec.max(), np.max(np.abs(b), axis=0).max() / np.max(np.abs(b), axis=0).min()))
            assert np.all(ec < tol), (k, int(np.argmax(ec)), float(ec.max()))
        if k in ('ell_f', 'ell_g'):
            a1, b1 = a.reshape(-1), b.reshape(-1)
            ed = np.abs(a1 - b1) / np.maximum(np.abs(b1), 1e-3 * np.max(np.abs(b1)))
            print('  %s grad %-10s worst entry %d relerr %.2e' % (tag, k, int(np.argmax(ed)), ed.max()))
            assert np.all(ed < tol), (k, int(np.argmax(ed)), float(ed.max()))


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'D%d' % c[3])
def test_predict_matches_oracle(engine, case):
    q = _case(case)
    engine.set_chunk(case[5] or 16384)
    c = q['cond']
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    for g_off in (0.0, -1.0):
        out = engine.predict(q['p'], q['X'], jitter=1e-6, g_offset=g_off)
        ref = q['predict'][g_off]
        for i, name in enumerate(ROWS9):
            e = relerr(out[i], np.asarray(ref[i]).reshape(-1))
            print('cond(Kuu)=%.2e g_offset %+.0f %s relerr=%.2e' % (c, g_off, name, e))
            assert e < tol, (name, e, c)
    engine.set_chunk(16384)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'D%d' % c[3])
def test_elbo_kl_and_gradient_match_oracle_and_repeat_bit_for_bit(engine, case):
    import zigp_oracle_torch as ot
    q = _case(case)
    engine.set_chunk(case[5] or 16384)
    engine.set_data(q['X'], q['Y'])
    ed, kl, g = engine.elbo(q['p'], jitter=1e-6, scale=SCALE)
    elbo_r, data_r, kl_r, g_r = q['elbo']
    c = q['cond']
    print('cond(Kuu)=%.2e elbo %.10e ref %.10e; data rel %.2e kl rel %.2e' % (
        c, ed - kl, elbo_r, abs(ed - SCALE * data_r) / abs(SCALE * data_r), abs(kl - kl_r) / abs(kl_r)))
    assert abs(ed - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r)
    assert abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    check_grads('D=%d' % case[3], g, g_r, c, ot.PARAM_KEYS)
    # repeatability: a second gradient call gives the same bits, and a value-only call the same KL and a data term to rounding
    ed2, kl2, g2 = engine.elbo(q['p'], jitter=1e-6, scale=SCALE)
    assert ed2 == ed and kl2 == kl and all(np.array_equal(np.asarray(g[k]), np.asarray(g2[k])) for k in g)
    ed_v, kl_v, g_v = engine.elbo(q['p'], jitter=1e-6, scale=SCALE, need_grad=False)
    ed_w, kl_w, _ = engine.elbo(q['p'], jitter=1e-6, scale=SCALE, need_grad=False)
    assert g_v is None and kl_v == kl and (ed_v, kl_v) == (ed_w, kl_w)
    assert abs(ed_v - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r)
    engine.set_chunk(16384)


MODE = (1500, 150, 90, 12, 0.8, 1024)


def test_whitened_model_at_D12(engine):
    import whiten_ref as wr
    N, Mf, Mg, D, ell, chunk = MODE
    X, Y, p = wide_problem(N, Mf, Mg, D, ell)
    p = dict(p, whiten=True)
    c = _cond(p)
    engine.set_chunk(chunk)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=SCALE)
    elbo_r, data_r, kl_r, g_r = wr.elbo_and_grad(X, Y, p, 1e-6, scale=SCALE, chunk=1000)
    assert abs(ed - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    check_grads('whiten D=12', g, g_r, c, wr.PARAM_KEYS)
    out, ref = engine.predict(p, X, jitter=1e-6), wr.build_predict(X, p, 1e-6, 0.0)
    for i, name in enumerate(ROWS9):
        assert relerr(out[i], ref[i]) < min(max(1e-9, 1e-13 * c), 1e-6), name
    engine.set_chunk(16384)


def test_full_covariance_model_at_D12(engine):
    import fullcov_ref as fr
    N, Mf, Mg, D, ell, chunk = MODE
    X, Y, p = wide_problem(N, Mf, Mg, D, ell)
    p = fr.make_lq(p, seed=N + Mf)
    c = _cond(p)
    engine.set_chunk(chunk)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=SCALE)
    elbo_r, data_r, kl_r, g_r = fr.elbo_and_grad(X, Y, p, 1e-6, scale=SCALE, chunk=1024)
    assert abs(ed - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    check_grads('q_full D=12', g, g_r, c, fr.PARAM_KEYS)
    out, ref = engine.predict(p, X, jitter=1e-6), fr.build_predict(X, p, 1e-6, 0.0)
    for i, name in enumerate(ROWS9):
        assert relerr(out[i], ref[i]) < min(max(1e-9, 1e-13 * c), 1e-6), name
    engine.set_chunk(16384)


def test_translation_invariance_at_D12(engine):
    """test_inputs_far_from_the_origin_translation_invariance at D = 12, with its bounds: inputs on a 2^-20 grid moved by +-4096 per
    dimension."""
    X, Y, p = wide_problem(1500, 150, 90, 12, 0.8)
    q = lambda a: np.round(a * 2.0 ** 20) / 2.0 ** 20
    X = q(X); p['Zf'] = q(p['Zf']); p['Zg'] = q(p['Zg'])
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    ed0, kl0, g0 = engine.elbo(p, jitter=1e-6)
    shift = 4096.0 * (1 - 2 * (np.arange(12) % 2))
    p2 = dict(p, Zf=p['Zf'] + shift, Zg=p['Zg'] + shift)
    assert np.array_equal(p2['Zf'] - shift, p['Zf'])          # exactly representable
    engine.set_data(X + shift, Y)
    ed1, kl1, g1 = engine.elbo(p2, jitter=1e-6)
    print('  elbo_data relerr %.2e, kl relerr %.2e' % (abs(ed1 - ed0) / abs(ed0), abs(kl1 - kl0) / abs(kl0)))
    assert abs(ed1 - ed0) < 1e-7 * abs(ed0) and abs(kl1 - kl0) < 1e-7 * abs(kl0)
    for k in g0:
        e = relerr(g1[k], g0[k])
        print('  grad %-10s relerr %.2e' % (k, e))
        assert e < 1e-6, (k, e)
    engine.set_chunk(16384)


def test_inducing_inputs_spread_over_thousands_of_lengthscales_at_D10(engine):
    """One coordinate of the inducing inputs and of the data stretched to +-2000 lengthscales (beyond KG_EXACT_SPREAD, where the D <= 8 path
    switches to its per-row reductions): the wide path's reductions are per-row always, and the gradients meet the ordinary bound."""
    import zigp_oracle_torch as ot
    X, Y, p = wide_problem(1200, 96, 80, 10, 0.8)
    rs = np.random.RandomState(9)
    span = 4000.0 * p['ell_f'][3]
    for k in ('Zf', 'Zg'):       # coordinate 3: a grid over 4000 lengthscales, the data scattered about the grid points (so that Kuf is not negligible)
        M = p[k].shape[0]
        p[k] = p[k].copy(); p[k][:, 3] = ((np.arange(M) + (0.5 if k == 'Zf' else 0.75)) / M - 0.5) * span
    X = X.copy(); X[:, 3] = p['Zf'][rs.randint(0, p['Zf'].shape[0], X.shape[0]), 3] + p['ell_f'][3] * rs.randn(X.shape[0])
    assert np.max(np.abs(p['Zf'][:, 3] - p['Zf'][:, 3].mean())) / p['ell_f'][3] > 1.0e3
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=1e-6)
    elbo_r, data_r, kl_r, g_r = ot.elbo_and_grad(X, Y, p, 1e-6, chunk=1000)
    c = _cond(p)
    assert abs(ed - data_r) <= 1e-7 * abs(data_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    check_grads('spread D=10', g, g_r, c, ot.PARAM_KEYS)
    engine.set_chunk(16384)


@pytest.mark.parametrize('D', [9, 64])
def test_rbf_K_wide(engine, D):
    import zigp_oracle as o
    rs = np.random.RandomState(D)
    Z, X, ell = rs.rand(37, D), rs.rand(301, D), 1.0 + rs.rand(D)
    assert relerr(engine.rbf_K(Z, X, ell, 1.7), o.rbf_K(Z, X, ell, 1.7)) < 1e-12
    assert relerr(engine.rbf_K(Z, None, ell, 1.7), o.rbf_K(Z, None, ell, 1.7)) < 1e-12


def test_refusals_leave_the_context_as_it_was(engine):
    """D = 65 is ZIGP_EARG naming the limit through every entry point that takes a dimension; the device fit loops and a Linear mean
    function are refused at D = 9; after each refusal a D = 3 call returns what it returned before, bit for bit."""
    from zigp import _lib
    from zigp.engine import _Packed
    lib, ctx = engine.lib, engine.ctx
    X3, Y3, p3 = make_problem(700, 40, 3, seed=5)
    engine.set_chunk(16384)

    def d3():
        engine.set_data(X3, Y3)
        ed, kl, g = engine.elbo(p3, jitter=1e-6)
        return (ed, kl) + tuple(np.asarray(g[k]).copy() for k in sorted(g))

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    base = d3()
    err = lambda: lib.zigp_last_error(ctx).decode()
    # D = 65
    X, Y, p = wide_problem(300, 20, 20, 64, 1.8)
    X65 = np.ascontiguousarray(np.hstack([X, X[:, :1]]))
    Yv = np.ascontiguousarray(Y.reshape(-1))
    dp = lambda a: a.ctypes.data_as(_lib.dp)
    assert lib.zigp_set_data(ctx, dp(X65), dp(Yv), 300, 65) == _lib.ZIGP_EARG and '64' in err()
    assert same(d3(), base)
    pk = _Packed(p)
    pk.struct.D = 65          # the struct's arrays are not read before the check
    ed, kl = C.c_double(0), C.c_double(0)
    assert lib.zigp_elbo(ctx, C.byref(pk.struct), 1e-6, 1.0, 0.0, 0, 10, 1, C.byref(ed), C.byref(kl), None) == _lib.ZIGP_EARG and '64' in err()
    out9 = np.zeros((9, 10))
    assert lib.zigp_predict(ctx, C.byref(pk.struct), dp(X65), 10, 1e-6, 0.0, dp(out9)) == _lib.ZIGP_EARG and '64' in err()
    Kout = np.zeros((300, 300))
    ell65 = np.ones(65)
    assert lib.zigp_rbf_K(ctx, dp(X65), 300, None, 300, 65, dp(ell65), 1.0, dp(Kout)) == _lib.ZIGP_EARG and '64' in err()
    assert same(d3(), base)
    with pytest.raises(ValueError, match='64'):
        engine.elbo(dict(p, Zf=np.zeros((20, 65)), Zg=np.zeros((20, 65)), ell_f=np.ones(65), ell_g=np.ones(65)))
    # a Linear mean function at D = 9
    a9 = np.ones(9)
    assert lib.zigp_set_mean_function(ctx, dp(a9), 9, 0.5) == _lib.ZIGP_EARG and '[1, 8]' in err()
    assert same(d3(), base)
    # the device fit loops at D = 9
    from zigp.optim import DenseDeviceFit, WhiteDeviceFit
    import dense_fit_ref as R
    X9, Y9, p9 = wide_problem(400, 16, 16, 9, 0.7)
    engine.set_data(X9, Y9)

    for cls in (DenseDeviceFit, WhiteDeviceFit):
        fit = cls(engine, R.make_pset(p9))
        x, m, v = fit.x.copy(), fit.m.copy(), fit.v.copy()
        with pytest.raises(ValueError, match='D = 9'):
            fit.steps(None, 0, 1e-6, 1.0, n_steps=2)
        assert int(lib.zigp_fit_steps_applied(ctx)) == 0 and fit.t == 0, 'a refused fit call applied a step'
        assert np.array_equal(x, fit.x) and np.array_equal(m, fit.m) and np.array_equal(v, fit.v), 'a refused fit call changed the state'
        assert same(d3(), base)


def test_model_surface_at_D12(engine):
    """OnOffSVGP with RBF(12, ARD=True): the bound equals the engine call, L-BFGS-B raises it, Adam runs on the host loop (the device loop
    stops at D = 8) and equals an explicit AdamGroups loop on the same minibatches, device_loop=True and a Linear mean raise, a Constant
    mean works, and the model survives pickling."""
    import zigp
    from onoffgpf import OnOffSVGP, OnOffLikelihood, kernels, mean_functions
    from zigp.optim import AdamGroups
    D, N, M = 12, 600, 20
    X, Y, p = wide_problem(N, M, M, D, 0.8, seed=3)

    def model(**kw):
        np.random.seed(4)
        return OnOffSVGP(X, Y, kernels.RBF(D, lengthscales=p['ell_f'].copy(), ARD=True), kernels.RBF(D, variance=5.0, lengthscales=p['ell_g'].copy(), ARD=True),
                         OnOffLikelihood(), p['Zf'].copy(), p['Zg'].copy(), **kw)

    m = model()
    ll = m.compute_log_likelihood()
    eng = zigp.reference_engine(0)
    eng.set_data(X, Y)
    from onoffgpf.OnOffSVGP import JITTER
    ed, kl, _ = eng.elbo(m._values(), jitter=JITTER, need_grad=False)
    assert ll == ed - kl
    m.optimize(maxiter=5)
    assert m.compute_log_likelihood() > ll
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.compute_log_likelihood() == m.compute_log_likelihood()
    # Adam on minibatches: the default falls to the host loop and equals an explicit loop
    a, b = model(minibatch_size=100), model(minibatch_size=100)
    assert not a._device_fit_eligible(a._pset())
    a.optimize(method='adam', maxiter=20)
    ps = b._pset()
    for q in ps.params.values():
        q.learning_rate = 0.01
    opt = AdamGroups(ps)
    for _ in range(20):
        opt.step(b._elbo(True)[1])
    for k, q in a._pset().params.items():
        assert relerr(q.value, ps.params[k].value) <= 1e-12, k
    with pytest.raises(ValueError, match='D = 12'):
        model(minibatch_size=100).optimize(method='adam', maxiter=2, device_loop=True)
    with pytest.raises(ValueError, match='Linear'):
        model(mean_function=mean_functions.Linear(np.zeros((D, 1)), 0.0))
    mc = model(mean_function=mean_functions.Constant(0.3))
    v0 = mc.compute_log_likelihood()
    assert np.isfinite(v0) and v0 != ll
    mc.optimize(maxiter=3)
    assert mc.compute_log_likelihood() > v0
