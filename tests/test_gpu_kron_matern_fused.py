"""GPU tests of Matern factors on the FUSED Kronecker kernels (zigp_set_kron_matern_fused / DenseEngine.set_kron_matern_fused; opt-in, off by
default): the _kinds kernels of csrc/zigp_kronf.hip and csrc/zigp_kronl.h against tests/kron_matern_ref.py (the oracle's literal dense order
with a kernel kind per factor) at the project's 1e-6, against the same call on the GEMM panels, and stage by stage against
tests/kronf_matern_ref.py.  Fixtures: kronf_matern_ref.fixture_kinds() -- tests/test_cpu_kron_matern.py and
tests/test_cpu_kron_matern_fused.py hold the reference's own floor on each at 1e-8 and cond(K_p + 1e-5 I) at 1e5.
The finish stage of a step with Matern factors (k_kf_kd_prepare, the second k_kf_finish, k_kf_krow_merge; k_kfl_krow_kinds behind
k_kfl_finish<3>) is held tap by tap in test_finish_stage_with_matern_factors (figures: profiles/kronf_finish_parity.log); its restatement,
kronf_matern_ref.finish, is pinned by tests/test_cpu_kronf_finish_ref.py.

On a build without the feature set_kron_matern_fused does not exist and every test here fails.  Every test prints its figures
(pytest -s; profiles/kron_matern_fused_parity.log keeps a run's)."""
import functools
import os

import numpy as np
import pytest

import kron_nd
import kron_matern_ref as kmr
import kronf_matern_ref as fm
from conftest import relerr
from test_gpu_kron_nd import _bit_identical, _check_grads, KERN_KEYS, VEC_KEYS, PRED_NAMES

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)]
TOL = 1e-6
J = kron_nd.JITTER
TABLE = fm.fixture_kinds()


@pytest.fixture
def fused(engine):
    """the engine with the switch on; off again afterwards, whatever the test did"""
    engine.set_kron_matern_fused(True)
    try:
        yield engine
    finally:
        engine.set_kron_panels(False)
        engine.set_kron_matern_fused(False)


@functools.lru_cache(maxsize=None)
def _ref_grad(name):
    X, Y, p = fm.fixture(name)
    return kmr.kron_elbo_and_grad(X, Y, p, J, scale=kron_nd.case_scale(name), g_offset=-0.5, f_mu=0.2)


def _on_panels(engine, call):
    engine.set_kron_panels(True)
    try:
        return call()
    finally:
        engine.set_kron_panels(False)


def _hook(engine, p, X, Y, **kw):
    """test_kron_fused_step follows the kinds of the CONTEXT (it does not read them from p): set the four of p, then take the step"""
    for tag, pair in zip('fg', kmr.kinds_of(p)):
        for q in range(2):
            engine.set_kron_kernel(tag, q, pair[q])
    return engine.test_kron_fused_step(p, X, Y, **kw)


def _grad_distance(a, b):
    return max([relerr(a[2][k], b[2][k]) for k in VEC_KEYS if k in a[2]] +
               [relerr(a[2][k][q], b[2][k][q]) for k in KERN_KEYS if k in a[2] for q in range(2)])


# ---- model level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(TABLE))
def test_predict_elbo_and_gradient_match_the_restatement(fused, name):
    """switch on: kron_predict (g_offset 0 and -1, an f_mu), kron_elbo value, KL and every gradient block -- the Z and lengthscale blocks
    also per input dimension -- against kron_matern_ref at 1e-6; the distance to the same call on the panels is printed"""
    X, Y, p = fm.fixture(name)
    assert fused.get_kron_matern_fused() is True
    for goff, fmu in ((0.0, None), (-1.0, 0.3)):
        out = fused.kron_predict(p, X, jitter=J, g_offset=goff, f_mu=fmu)
        ref = kmr.kron_build_predict(X, p, J, goff, fmu)
        pan = _on_panels(fused, lambda: fused.kron_predict(p, X, jitter=J, g_offset=goff, f_mu=fmu))
        errs = [relerr(out[i], ref[i]) for i in range(9)]
        print('%s f %s g %s g_offset %g: %s | fused vs panels %.1e' % (name, p['kern_f'], p['kern_g'], goff, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs)),
                                                                     max(relerr(out[i], pan[i]) for i in range(9))))
        assert max(errs) < TOL, (name, goff, errs)
    scale = kron_nd.case_scale(name)
    res = fused.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2)
    ed, kl, g = res
    e_r, d_r, kl_r, g_r = _ref_grad(name)
    pan = _on_panels(fused, lambda: fused.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2))
    print('%s elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e | fused vs panels: value %.1e kl %.1e gradients %.1e'
          % (name, ed - kl, e_r, abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r), abs(ed - pan[0]) / abs(pan[0]),
             abs(kl - pan[1]) / abs(pan[1]), _grad_distance(res, pan)))
    assert abs(ed - scale * d_r) <= TOL * abs(scale * d_r)
    assert abs(kl - kl_r) <= TOL * abs(kl_r)
    worst = _check_grads(name, kron_nd.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS + ('f_mu',), tol=TOL)
    print('%s worst gradient figure %.2e' % (name, worst))
    # bit for bit: the value-only call and the call without the KL return the gradient call's data term; a repeated call equals itself
    v = fused.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2, need_grad=False)
    assert v[0] == ed and v[1] == kl and v[2] is None
    nk = fused.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2, include_kl=False, need_grad=False)
    assert nk[0] == ed and nk[1] == 0.0
    _bit_identical(fused.kron_elbo(p, X, Y, jitter=J, scale=scale, g_offset=-0.5, f_mu=0.2), res)


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('name', ['d21-12', 'd31', 'L32'])
def test_heads_match_the_restatement(fused, name, lik):
    X, Y, p = fm.fixture(name)
    Y = (Y > 0) * 1.0 if lik == 'bernoulli' else Y
    hp = dict(kron_nd.head_params(p), kern_f=p['kern_f'])
    f_mu = 0.0 if lik == 'gaussian' else 0.2
    out = fused.kron_head_predict(hp, X, lik, jitter=J, f_mu=f_mu)
    ref = kmr.kron_head_predict(X, hp, lik, J, f_mu)
    errs = [relerr(out[i], ref[i]) for i in range(4)]
    pan = _on_panels(fused, lambda: fused.kron_head_predict(hp, X, lik, jitter=J, f_mu=f_mu))
    print('%s %s f %s predict fmean %.1e fvar %.1e pfmean %.1e pfvar %.1e | fused vs panels %.1e'
          % ((name, lik, hp['kern_f']) + tuple(errs) + (max(relerr(out[i], pan[i]) for i in range(4)),)))
    assert max(errs) < TOL
    scale = kron_nd.case_scale(name)
    res = fused.kron_head_elbo(hp, X, Y, lik, jitter=J, scale=scale, f_mu=f_mu)
    ed, kl, g = res
    e_r, d_r, kl_r, g_r = kmr.kron_head_elbo_and_grad(X, Y, hp, lik, J, scale=scale, f_mu=f_mu)
    assert abs(ed - scale * d_r) <= TOL * abs(scale * d_r) and abs(kl - kl_r) <= TOL * abs(kl_r)
    _check_grads('%s %s' % (name, lik), kron_nd.CASES[name]['D'], g, g_r, ('Zf', 'ell_f', 'var_f'),
                 ('u_fm', 'u_fs_sqrt', 'f_mu') + (('noise',) if lik == 'gaussian' else ()), tol=TOL)
    pe = _on_panels(fused, lambda: fused.kron_head_elbo(hp, X, Y, lik, jitter=J, scale=scale, f_mu=f_mu))
    print('%s %s head fused vs panels: value %.1e gradients %.1e' % (name, lik, abs(ed - pe[0]) / abs(pe[0]), _grad_distance(res, pe)))
    v = fused.kron_head_elbo(hp, X, Y, lik, jitter=J, scale=scale, f_mu=f_mu, need_grad=False)
    assert v[0] == ed and v[1] == kl


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------------
def test_rows_of_the_resident_set_equal_host_rows_and_the_stepper(fused):
    for name in ('d21-mix', 'L51'):
        X, Y, p = fm.fixture(name)
        N = X.shape[0]
        fused.set_data(X, Y)
        for lo, hi in ((0, N), (5, N - 3), (7, 7)):
            a = fused.kron_elbo(p, X[lo:hi], Y[lo:hi], jitter=J, scale=2.5)
            b = fused.kron_elbo(p, rows=(lo, hi), jitter=J, scale=2.5)
            _bit_identical(a, b)
        assert a[0] == 0.0 and a[1] != 0.0      # the empty row set: no data term, the KL as usual
        hp = dict(kron_nd.head_params(p), kern_f=p['kern_f'])
        _bit_identical(fused.kron_head_elbo(hp, X[5:N - 3], Y[5:N - 3], 'gaussian', jitter=J, scale=2.5),
                       fused.kron_head_elbo(hp, lik='gaussian', rows=(5, N - 3), jitter=J, scale=2.5))
        st = fused.kron_stepper(p)
        _bit_identical(st(p, rows=(5, N - 3), jitter=J, scale=2.5), fused.kron_elbo(p, rows=(5, N - 3), jitter=J, scale=2.5))


def test_switch_off_is_the_panels_and_the_refusals_keep_their_texts(engine):
    """off (the default): a Matern call equals the same call under set_kron_panels(True); the fused hook and both fit loops refuse with the
    texts tests/test_gpu_kron_matern.py pins.  On: set_kron_panels(True) still wins, and the C entry points name their argument."""
    from zigp import _lib
    X, Y, p = fm.fixture('d11')
    assert engine.get_kron_matern_fused() is False
    a = engine.kron_elbo(p, X, Y, jitter=J, scale=3.0)
    pa = engine.kron_predict(p, X, jitter=J, g_offset=-1.0)
    b = _on_panels(engine, lambda: engine.kron_elbo(p, X, Y, jitter=J, scale=3.0))
    _bit_identical(a, b)
    assert np.array_equal(pa, _on_panels(engine, lambda: engine.kron_predict(p, X, jitter=J, g_offset=-1.0)))
    with pytest.raises(ValueError, match='does not run on the fused Kronecker kernels'):
        _hook(engine, p, X, Y, taps=False)
    shape = dict(M0f=6, M1f=5, M0g=6, M1g=5, D0=3, D1=1)
    n = 2 * (6 * 3 + 5 * 1 + 2 * 30 + 3 + 1 + 2) + 1
    x, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    with pytest.raises(ValueError, match='Matern52 kernel on factor 1 of latent f is set; the device loop fits RBF factors only'):
        engine.kron_fit_steps(dict(shape, kern_f=('rbf', 'matern52')), x, m, v, [1e-3] * 17, [0] * 17, 0, [0, 500], 500, jitter=J)
    with pytest.raises(ValueError, match='Matern32 kernel on factor 0 of latent f is set; the device loop fits RBF factors only'):
        engine.kron_head_fit_steps(dict(shape, kern_f='matern32'), 'gaussian', x[:91], m[:91], v[:91], [1e-3] * 10, [0] * 10, [1] * 10, 0, [0], 500, jitter=J)
    lib, ctx = engine.lib, engine.ctx
    for bad in (2, -1):
        assert lib.zigp_set_kron_matern_fused(ctx, bad) == _lib.ZIGP_EARG and 'on must be 0 or 1' in lib.zigp_last_error(ctx).decode()
    assert lib.zigp_set_kron_matern_fused(None, 1) == _lib.ZIGP_EARG and lib.zigp_get_kron_matern_fused(None) == _lib.ZIGP_EARG
    assert lib.zigp_get_kron_matern_fused(ctx) == 0
    engine.set_kron_matern_fused(True)
    try:
        assert lib.zigp_get_kron_matern_fused(ctx) == 1
        f = engine.kron_elbo(p, X, Y, jitter=J, scale=3.0)
        assert f[0] != a[0] or any(not np.array_equal(x_, y_) for (_, x_), (_, y_) in zip(_flat(f), _flat(a)))      # other kernels ran
        _bit_identical(_on_panels(engine, lambda: engine.kron_elbo(p, X, Y, jitter=J, scale=3.0)), a)               # the panels still win
        r = _hook(engine, p, X, Y, jitter=J, scale=3.0, taps=False)                                   # and the hook accepts the step
        assert r['elbo_data'] == f[0]
    finally:
        engine.set_kron_matern_fused(False)
    _bit_identical(engine.kron_elbo(p, X, Y, jitter=J, scale=3.0), a)


def _flat(res):
    from test_gpu_kron_nd import _flat as f
    return f(res)


def test_all_rbf_with_the_switch_on_equals_a_fresh_context(engine):
    """every kind RBF, switch on, after Matern calls on the fused kernels: elbo, predict and both heads return the bits of a context that
    never saw the switch (the RBF kernels are launched, with the arguments they always had)"""
    from zigp.engine import DenseEngine
    X, Y, p = kron_nd.problem('d21-12')
    Xl, Yl, pl = kron_nd.problem('L32')
    hp = kron_nd.head_params(p)

    def calls(e):
        return (e.kron_elbo(p, X, Y, jitter=J, scale=2.0), e.kron_elbo(pl, Xl, Yl, jitter=J, scale=2.0),
                e.kron_predict(p, X, jitter=J, g_offset=-1.0), e.kron_predict(pl, Xl, jitter=J),
                e.kron_head_elbo(hp, X, Y, 'gaussian', jitter=J), e.kron_head_predict(hp, X, 'bernoulli', jitter=J, f_mu=0.2))

    fresh = DenseEngine(device=0)
    try:
        want = calls(fresh)
    finally:
        fresh.close()
    engine.set_kron_matern_fused(True)
    try:
        engine.kron_elbo(fm.fixture('d21-12')[2], X, Y, jitter=J)
        engine.kron_elbo(fm.fixture('L32')[2], Xl, Yl, jitter=J)
        got = calls(engine)
    finally:
        engine.set_kron_matern_fused(False)
    for i in (0, 1, 4):
        _bit_identical(got[i], want[i])
    for i in (2, 3, 5):
        assert np.array_equal(got[i], want[i])


# ---- ragged and empty tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['d11', 'L32'])
def test_ragged_tiles_and_shards(fused, name):
    """N = 1, 15, 16, 17, 33 rows against the restatement; an empty row range; two uneven shards add up to the whole batch under the bounds of
    test_gpu_kron_matern.py::test_two_shards_add_up (padding points contribute exact zeros)"""
    X, Y, p = fm.fixture(name)
    for N in (1, 15, 16, 17, 33):
        ed, kl, g = fused.kron_elbo(p, X[:N], Y[:N], jitter=J, scale=1.0)
        e_r, d_r, kl_r, g_r = kmr.kron_elbo_and_grad(X[:N], Y[:N], p, J)
        worst = _check_grads('%s N=%d' % (name, N), kron_nd.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
        out = fused.kron_predict(p, X[:N], jitter=J)
        ref = kmr.kron_build_predict(X[:N], p, J)
        print('%s N=%d: data %.1e kl %.1e worst gradient %.1e predictions %.1e' % (name, N, abs(ed - d_r) / abs(d_r), abs(kl - kl_r) / abs(kl_r), worst,
                                                                                 max(relerr(out[i], ref[i]) for i in range(9))))
        assert abs(ed - d_r) <= TOL * abs(d_r) and abs(kl - kl_r) <= TOL * abs(kl_r) and max(relerr(out[i], ref[i]) for i in range(9)) < TOL
    # an empty row range of the resident set: no data term, the KL of a call with rows, and the gradient of -KL alone
    fused.set_data(X, Y)
    full = fused.kron_elbo(p, rows=(0, 33), jitter=J, scale=1.0)
    e0, k0, g0 = fused.kron_elbo(p, rows=(9, 9), jitter=J, scale=1.0)
    assert e0 == 0.0 and k0 == full[1]
    _, _, klr, gk = kmr.kron_elbo_and_grad(X[:1], Y[:1], p, J, scale=0.0)
    assert abs(k0 - klr) <= TOL * abs(klr)
    for k_, a_ in _flat((e0, k0, g0)):
        assert np.all(np.isfinite(a_)), k_
    assert g0['noise'] == 0.0
    worst = _check_grads('%s empty range' % name, kron_nd.CASES[name]['D'], g0, gk, KERN_KEYS, tuple(k_ for k_ in VEC_KEYS if k_ != 'noise'), tol=TOL)
    print('%s empty row range: KL %.1e, worst gradient against the KL-only restatement %.1e' % (name, abs(k0 - klr) / abs(klr), worst))
    cut = 131
    ed, kl, g = fused.kron_elbo(p, X, Y, jitter=J, scale=1.0)
    a = fused.kron_elbo(p, X[:cut], Y[:cut], jitter=J, scale=1.0, include_kl=True)
    b = fused.kron_elbo(p, X[cut:], Y[cut:], jitter=J, scale=1.0, include_kl=False)
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


# ---- extremes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['d11', 'L32'])
def test_a_row_on_an_inducing_point_and_a_row_far_away(fused, name):
    """row 0 exactly on inducing points of both latents' first factor grid, row 1 1e3 lengthscales away in every column: predictions and every
    gradient finite; the far row's K tiles are exact +0 (q0 = q1 = mean = st = 0 in the forward tap, its predictive mean exactly f_mu)"""
    X, Y, p = fm.fixture(name)
    D0 = kron_nd.CASES[name]['D'][0]
    Xe = np.array(X[:20])
    Xe[0] = np.concatenate([p['Zf'][0][3], p['Zf'][1][2]])
    far = 1e3 * max(float(np.max(e)) for k in ('ell_f', 'ell_g') for e in p[k])
    Xe[1] = np.concatenate([p['Zf'][0][0] + far, p['Zf'][1][0] + far])
    assert Xe.shape[1] == D0 + kron_nd.CASES[name]['D'][1]
    out = fused.kron_predict(p, Xe, jitter=J, f_mu=0.3)
    assert np.all(np.isfinite(out))
    assert out[3][1] == 0.3 and out[5][1] == 0.0                                       # fmean = f_mu, gmean = 0: every K entry of the far row is +0
    vf, vg = float(p['var_f'][0][0] * p['var_f'][1][0]), float(p['var_g'][0][0] * p['var_g'][1][0])
    assert out[4][1] == vf and out[6][1] == vg                                         # and the variances are Knn
    ed, kl, g = fused.kron_elbo(p, Xe, Y[:20], jitter=J)
    assert np.isfinite(ed) and np.isfinite(kl)
    for k, a in _flat((ed, kl, g)):
        assert np.all(np.isfinite(a)), k
    t = _hook(fused, p, Xe, Y[:20], jitter=J)
    for h in range(2):
        part = t['lat'][h]['part']
        assert not np.any(part[:, 1]) and not np.any(np.signbit(part[:, 1])), 'the far row is not exact +0'
    e_r, d_r, kl_r, g_r = kmr.kron_elbo_and_grad(Xe, Y[:20], p, J)
    _check_grads('%s extremes' % name, kron_nd.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)


# ---- stage level ------------------------------------------------------------------------------------------------------------------------
def _stage_latent(case, kinds, large, t, Z, ell, var, M, D, X, N, cap, jitter):
    """one latent of a tapped fused step with Matern factors: the factor taps K and P, the forward tap `part` and the moment blocks Kr0 / Kr1 of
    `work` (with the other blocks, which must not have moved) against kronf_matern_ref on the tapped inputs -- the project's rule
    err_gpu <= 4 err_np + 16 eps S per element (test_gpu_kronf_stages._rule)"""
    from test_gpu_kronf_stages import _rule, _p_residual
    import kronf_ref as kr
    LD = np.longdouble
    sfx = '_kinds' + ('l' if large else '')
    for q in range(2):
        Kq = t['K'][q][:M[q], :M[q]]
        k64, kld = fm.factor_K(kinds[q], Z[q], ell[q], var[q], jitter), fm.factor_K(kinds[q], Z[q], ell[q], var[q], jitter, LD)
        S = fm.ktile(kinds[q], Z[q], ell[q], var[q], Z[q], weight=True)[1] + jitter * np.eye(M[q])
        _rule('factor' + sfx, case, 'K%d' % q, Kq, k64, kld, S)
        R = -(-M[q] // 32) * 32
        pad = np.array(t['K'][q][:R, :R])
        pad[:M[q], :M[q]] = 0
        want = np.eye(R)
        want[:M[q], :M[q]] = 0
        assert np.array_equal(pad, want), '%s: K_%d is not identity padded' % (case, q)
        _p_residual('factor' + sfx, case, q, Kq, t['P'][q][:M[q], :M[q]])
    P = [t['P'][q][:M[q], :M[q]] for q in range(2)]
    Al, S2 = t['Al'][:M[0], :M[1]], t['S2'][:M[0], :M[1]]
    args = (kinds, P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N)
    f64, S = fm.forward(*args)
    fld, _ = fm.forward(*args, dtype=LD)
    assert not np.any(t['part'][:, N:]), '%s: part rows N .. Npad' % case
    for r, k in enumerate(('q0', 'q1', 'mean', 'st')):
        _rule('forward' + sfx, case, k, t['part'][r, :N], f64[r], fld[r], S[r])
    bargs = args + (t['part'][:, :N],) + tuple(t['cot'][r, :N] for r in range(4)) + (t['zc'][0], t['zc'][1])
    b64, bld = fm.backward(*bargs), fm.backward(*bargs, dtype=LD)
    w = kr.work_split(t['work'], cap)
    for k in ('dAl', 'dS2', 'dP0', 'dP1', 'Kr0', 'Kr1'):
        r, c = b64[k][0].shape
        _rule('backward' + sfx, case, k, w[k][:r, :c], b64[k][0], bld[k][0], b64[k][1])
        assert not np.any(w[k][r:]), '%s: %s rows beyond the grid' % (case, k)
        if not k.startswith('Kr'):
            assert not np.any(w[k][:, c:]), '%s: %s columns beyond the grid' % (case, k)
            continue
        q = int(k[2])
        assert not np.any(w[k][:, c:15]), '%s: %s columns between the moments and column 15' % (case, k)
        if b64['Kd%d' % q] is None:
            assert not np.any(w[k][:, 15]), '%s: column 15 of an RBF factor' % case
        else:
            _rule('backward' + sfx, case, 'Kd%d' % q, w[k][:r, 15], b64['Kd%d' % q][0], bld['Kd%d' % q][0], b64['Kd%d' % q][1])


@pytest.mark.parametrize('name', ['d11', 'd21-21', 'd31', 'L32'])
def test_stage_taps_against_the_long_double_restatement(fused, name):
    from test_gpu_kronf_stages import _check_facts, _unpack
    X, Y, p = fm.fixture(name)
    k = kron_nd.CASES[name]
    N, D = X.shape[0], k['D']
    grids = [k['f'], k['g'] or k['f']]
    out = _hook(fused, p, X, Y, jitter=J, scale=kron_nd.case_scale(name))
    cap, nb = _check_facts(out['facts'], grids, N, 2)
    for h, tag in enumerate('fg'):
        Z, ell, var = _unpack(p, tag)
        _stage_latent('%s/%s' % (name, tag), kmr.kinds_of(p)[h], cap == (1, 7), out['lat'][h], Z, ell, var, grids[h], D, X, N, cap, J)
    # the hook's step is an ordinary step
    ed, kl, g = fused.kron_elbo(p, X, Y, jitter=J, scale=kron_nd.case_scale(name))
    assert out['elbo_data'] == ed and out['kl'] == kl
    for k in g:
        for a, b in zip(g[k], out['grads'][k]) if isinstance(g[k], list) else [(g[k], out['grads'][k])]:
            assert np.array_equal(a, b), k


@pytest.mark.parametrize('shape', ['s11', 's12', 's21', 's22p', 'Lx', 'Lr'])
def test_an_rbf_factor_inside_a_matern_instantiation_keeps_the_bits_of_the_rbf_kernels(fused, shape):
    """the exact tier of test_gpu_kronf_stages.py (small-integer inputs, K tiles exact selectors): latent g gets a Matern kind, so the step
    runs the _kinds kernels; latent f, all RBF inside them, must produce every tap the RBF instantiation produces, bit for bit"""
    import kronf_ref as kr
    from test_gpu_kronf_stages import SHAPES
    gf, gg = SHAPES[shape]
    D, N = (2, 1), 333
    e = kr.exact_problem(gf, gg or gf, D, N, 0.0, seed=5)
    inject = [L['cot'] for L in e['lat']]
    fused.set_kron_matern_fused(False)
    rbf = _hook(fused, e['p'], e['X'], e['Y'], jitter=0.0, scale=1.0, inject=inject)
    fused.set_kron_matern_fused(True)
    mat = _hook(fused, kmr.with_kinds(e['p'], 'rbf', ('matern32', 'matern52')), e['X'], e['Y'], jitter=0.0, scale=1.0, inject=inject)
    a, b = rbf['lat'][0], mat['lat'][0]
    for k in ('part', 'work', 'U', 'S2', 'T0', 'T1', 'Al', 'AlF', 'S2F', 'AlTF', 'S2TF'):
        assert np.array_equal(a[k], b[k]), (shape, k)
    for k in ('K', 'P', 'PF', 'dvec', 'Zs', 'zc'):
        for q in range(2):
            assert np.array_equal(a[k][q], b[k][q]), (shape, k, q)
    # the gradients that come from the work block alone (var_f and the noise also take sums of the point-wise kernel's own cotangents,
    # which see latent g: those are not injected)
    for k in ('Zf', 'ell_f'):
        for q in range(2):
            assert np.array_equal(rbf['grads'][k][q], mat['grads'][k][q]), (shape, k, q)
    assert np.array_equal(rbf['grads']['u_fm'], mat['grads']['u_fm']) and np.array_equal(rbf['grads']['u_fs_sqrt'], mat['grads']['u_fs_sqrt'])
    assert not np.array_equal(rbf['lat'][1]['part'], mat['lat'][1]['part']) or not np.array_equal(rbf['lat'][1]['work'], mat['lat'][1]['work'])


# ---- fit loops --------------------------------------------------------------------------------------------------------------------------
FIT_KINDS = {'d31': {'f': ('rbf', 'matern32'), 'g': ('matern52', 'rbf')}, 'L32': {'f': ('matern52', 'matern32'), 'g': ('rbf', 'matern52')}}


@pytest.mark.parametrize('name', list(FIT_KINDS))
def test_device_fit_loop_equals_host_adam_loop(fused, name):
    """zigp_kron_fit_steps with Matern factors, switch on in both runs so that the same kernels produce the gradients: 30 device steps in two
    calls, one wrap-around host batch, against the same iterations stepped from the host -- protocol and bounds of
    test_gpu_kron_nd.py::test_device_fit_loop_equals_host_adam_loop_nd (1e-12 of each block's magnitude, 1e-10 on the ELBO history)"""
    from onofftf.model import KronDeviceFit, FIT_BLOCK_NAMES, set_kernels
    from test_gpu_onofftf import _host_steps
    from test_gpu_kron_nd import _nd_pset
    X, Y, _ = kron_nd.fit_problem(name)
    X, Y = np.array(X), np.array(Y)
    N, batch, n_steps = X.shape[0], 500, 30
    psets = [_nd_pset(name), _nd_pset(name)]
    for ps in psets:
        set_kernels(ps, FIT_KINDS[name])
    rs = np.random.RandomState(2)
    rows_seq = [int(r) for r in rs.randint(0, N - batch, size=n_steps)]
    rows_seq[n_steps // 2] = -1
    wi = rs.permutation(N)[:batch]
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    jitter, scale = J, N / batch
    h_host = _host_steps(fused, psets[0], rows_seq, batch, jitter, scale, X, Y, wraps)
    fused.set_data(X, Y)
    fit = KronDeviceFit(fused, psets[1])
    ed, kl = [], []
    for a, b in ((0, 12), (12, n_steps)):
        seq = rows_seq[a:b]
        e_, k_ = fit.steps(seq, batch, jitter, scale, *(wraps if -1 in seq else (None, None)))
        ed += list(e_); kl += list(k_)
    assert fit.t == n_steps
    h_dev = np.stack([ed, kl], 1)
    eh = np.max(np.abs(h_dev - h_host) / np.abs(h_host))
    worst = max(float(np.max(np.abs(psets[1].params[k].value - psets[0].params[k].value)) / np.max(np.abs(psets[0].params[k].value)))
                for k in FIT_BLOCK_NAMES)
    u0 = _nd_pset(name)
    moved = max(float(np.max(np.abs(psets[0].params[k].value - u0.params[k].value))) for k in ('f_ind/value', 'g_ind/value'))
    print('fit %s kinds %s: %d device steps vs host AdamGroups: worst parameter block %.2e, ELBO history %.2e (u moved by up to %.3f)'
          % (name, FIT_KINDS[name], n_steps, worst, eh, moved))
    assert worst <= 1e-12 and eh <= 1e-10 and moved > 1e-2, (worst, eh, moved)


def test_head_device_fit_loop_equals_host_loop(fused):
    """zigp_kron_head_fit_steps with a Matern 3/2 time factor (d31, Gaussian): 20 steps in two calls against the host loop, under the rule of
    test_gpu_kron_nd.py::test_head_fit_one_step_and_20_steps_nd -- within max(8 d, 1e-13), d the distance of two host runs that differ
    by a seeded +-1 ulp, 8 d <= 1e-7"""
    import head_fit_ref as R
    from onofftf.heads import HeadDeviceFit
    from onofftf.model import set_kernels
    from test_gpu_kron_nd import _nd_head_problem
    X, Y, mk0 = _nd_head_problem('d31', 'gaussian')

    def mk():
        ps = mk0()
        set_kernels(ps, ('rbf', 'matern32'), ('f',))
        return ps

    seq, wi = R.rows_with_a_wrap(20)
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    a, b, dv = mk(), mk(), mk()
    ha = R.host_loop(fused, a, 'gaussian', seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps)
    hb = R.host_loop(fused, b, 'gaussian', seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps, nudge_seed=1)
    fused.set_data(X, Y)
    fit = HeadDeviceFit(fused, dv, 'gaussian')
    hist = []
    for lo, hi in ((0, 8), (8, 20)):
        part = seq[lo:hi]
        e_, k_ = fit.steps(part, R.BATCH, R.JITTER, R.SCALE, *(wraps if -1 in part else (None, None)))
        hist.append(np.stack([e_, k_], 1))
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    e_par, e_hist = R.block_distance(dv, a), R.hist_distance(np.concatenate(hist), ha)
    print('head d31 gaussian (rbf, matern32), 20 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e)'
          % (d_par, d_hist, e_par, R.bound(d_par), e_hist, R.bound(d_hist)))
    assert 8 * max(d_par, d_hist) <= 1e-7 and fit.t == 20
    assert e_par <= R.bound(d_par) and e_hist <= R.bound(d_hist)


# ---- model surface ----------------------------------------------------------------------------------------------------------------------
def test_onoff_and_fit_head_take_the_device_loop_with_fused_matern(engine, tmp_path, monkeypatch):
    """onoff(..., kernels=('rbf', 'matern32'), fused_matern=True, device_loop=True), 200 iterations on the small pptr fixture: the device loop
    runs (no host-loop line in the log), the cost falls, the engine's switch is off again afterwards, the option is not in the
    checkpoint, and predict_onoff(..., fused_matern=True) is within 1e-6 of predict_onoff without the option.  fit_head likewise."""
    import logging
    from test_gpu_onofftf import _pptr
    from onofftf import onoff, predict_onoff
    from onofftf.heads import fit_head, init_head_params
    from onofftf.svgppred import predict_svgp
    import sys
    onoff_mod, heads_mod = sys.modules['onofftf.onoff'], sys.modules['onofftf.heads']      # (the package attribute `onoff` is the function)
    reached = []

    def spy(mod, tag):
        real = mod._device_loop

        def loop(eng, *a, **kw):
            reached.append((tag, eng.get_kron_matern_fused()))      # the device loop itself, entered with the switch on
            return real(eng, *a, **kw)
        monkeypatch.setattr(mod, '_device_loop', loop)

    spy(onoff_mod, 'onoff')
    spy(heads_mod, 'head')
    Xtr, Ytr, Xte, Yte = _pptr()
    Xtr, Ytr = Xtr[:4000], Ytr[:4000]
    d = str(tmp_path) + '/'
    hist = []
    np.random.seed(0)
    onoff(Xtr, Ytr, Xte[:500], Yte[:500], d, num_iter=200, num_inducing_f=(6, 5), num_inducing_g=(6, 5), num_minibatch=1000, engine=engine,
          kmeans_seed=1, history=hist, device_loop=True, kernels=('rbf', 'matern32'), fused_matern=True)
    assert engine.get_kron_matern_fused() is False and reached == [('onoff', True)]
    assert engine.lib.zigp_kron_fit_steps_applied(engine.ctx) > 0      # the last fit call applied its device steps
    log = open(os.path.join(d, 'modelsumm.log')).read()
    assert 'the host Adam loop runs' not in log
    assert len(hist) == 200 and np.mean(hist[-5:]) < np.mean(hist[:5])
    assert not any('fused' in k for k in np.load(os.path.join(d, 'model.npz')).files)
    plain = predict_onoff(Xtr[:200], Xte[:300], d, np.array([6, 5]), np.array([6, 5]), engine=engine)
    fusedp = predict_onoff(Xtr[:200], Xte[:300], d, np.array([6, 5]), np.array([6, 5]), engine=engine, fused_matern=True)
    for a, b in zip(plain, fusedp):
        for k in ('gfmean', 'fmean', 'pgmean'):
            e = relerr(b[k], a[k])
            print('predict_onoff fused_matern vs panels %s %.1e' % (k, e))
            assert e < TOL and not np.array_equal(a[k], b[k])
    # the regression head
    logger = logging.getLogger('fused-matern-head')
    lines = []
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    logger.addHandler(handler)
    logger.setLevel(logging.DEBUG)
    try:
        pset = init_head_params(Xtr, (6, 5), 'gaussian', kmeans_seed=1)
        ck = os.path.join(d, 'head')
        h2 = []
        fit_head(pset, 'gaussian', Xtr, Ytr, 200, 1000, logger, ckpt=ck, eng=engine, history=h2, device_loop=True, kernels=('rbf', 'matern52'), fused_matern=True)
    finally:
        logger.removeHandler(handler)
    assert engine.get_kron_matern_fused() is False
    assert reached == [('onoff', True), ('head', True)]
    assert not any('the host Adam loop runs' in s for s in lines) and len(h2) == 200 and np.mean(h2[-5:]) < np.mean(h2[:5])
    pa = predict_svgp(Xtr[:200], Xte[:300], ck, np.array([6, 5]), engine=engine)
    pb = predict_svgp(Xtr[:200], Xte[:300], ck, np.array([6, 5]), engine=engine, fused_matern=True)
    for a, b in zip(pa, pb):
        for k in ('fmean', 'fvar'):
            assert relerr(b[k], a[k]) < TOL


# ---- the finish stage with Matern factors ------------------------------------------------------------------------------------------------
L77_KINDS = fm.L77_KINDS


def _finish_fixture(name):
    if name in TABLE:
        return fm.fixture(name) + (kron_nd.CASES[name]['f'], kron_nd.CASES[name]['g'] or kron_nd.CASES[name]['f'], kron_nd.CASES[name]['D'])
    if name == 'L77':
        X, Y, p = kron_nd.problem(name)
        k = kron_nd.CASES[name]
        return X, Y, kmr.with_kinds(p, *L77_KINDS), k['f'], k['g'] or k['f'], k['D']
    # a larger grid at D = (1, 1): k_kfl_krow_kinds multiplies by inv_ell[d] for d >= D, which is safe because the hyperparameter record is zero there
    X, Y, p = kron_nd.edge_problem((10, 100), (1, 1))
    return X, Y, kmr.with_kinds(p, ('matern52', 'matern32'), ('rbf', 'matern52')), (10, 100), (10, 100), (1, 1)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _finish_kinds_latent(case, kinds, large, t, Z, ell, var, s, M, D, cap, jitter, kl):
    """one latent of a tapped step with Matern factors: everything the finish stage leaves, against kronf_ref.finish / kronf_matern_ref.finish
    in long double on the stage's own tapped inputs (test_gpu_kronf_stages._rule), and the bit-for-bit identities between its runs"""
    import kronf_ref as kr
    from test_gpu_kronf_stages import _rule, _log, finish_inputs, check_G_and_krow_from_G, assert_unwritten
    from zigp import _lib
    LD = np.longdouble
    sfx = 'finish_kinds' + ('l' if large else '')
    args = finish_inputs(t, Z, s, M, cap, jitter)
    w, K = args[0], args[1:3]
    mat = [k != 'rbf' for k in kinds]
    assert_unwritten(case, t, M, D)
    assert 'krow_first_cap' in t and (large or 'krow2_cap' in t)
    cols = [slice(1, 1 + 2 * D[q]) for q in range(2)]
    k64, kld = fm.finish(kinds, *args, kl, ell, var), fm.finish(kinds, *args, kl, ell, var, dtype=LD)
    for q in range(2):
        assert np.all(np.isfinite(t['krow'][q])), '%s: a non-finite krow entry' % case
        assert not np.any(t['krow'][q][:, 1 + 2 * D[q]]), '%s: krow column 1 + 2 D' % case
        _rule(sfx, case, 'krow%d' % q, t['krow'][q], k64['krow%d' % q][0], kld['krow%d' % q][0], k64['krow%d' % q][1])
    for k in ('gu', 'gs'):       # written by the first run only
        _rule(sfx, case, k, t[k], k64[k][0], kld[k][0], k64[k][1])
    if large:
        def krow_of(q, g, ag, dt):
            mom = (fm.zz_kd(kinds[q], Z[q], ell[q], var[q], dt) + (w['Kr%d' % q][:, 15],)) if mat[q] else None
            return kr.krow_from_G(g, ag, K[q], w['Kr%d' % q], Z[q], args[13 + q], jitter, dt, _mom=mom)
        check_G_and_krow_from_G(sfx, case, t, args, kl, k64, kld, M, krow_of)
        for q in range(2):
            if not mat[q]:
                assert _bits(t['krow'][q], t['krow_first'][q]), '%s: the rows of RBF factor %d are not what stage 3 wrote' % (case, q)
            else:
                # column 0: k_kfl_krow_kinds sums G . kz over the same lanes in the same order as stage 3, but as `s0 += gj * kz` where stage 3 has
                # `tt = ... * kz; s0 += tt` with tt used again: whether either is contracted to an FMA is the compiler's choice, so the text does
                # not guarantee the bits.  Column 0 is held by the rule (krow|G above); whether the bits agree is logged.
                _log(sfx, case, 'krow%d column 0 %s stage 3\'s bits' % (q, 'keeps' if _bits(t['krow'][q][:, 0], t['krow_first'][q][:, 0]) else 'does NOT keep'))
        return
    # ---- small grids: k_kf_finish, k_kf_kd_prepare, k_kf_finish on (K', work'), k_kf_krow_merge
    want = np.array(t['work'])
    ws = kr.work_split(want, cap)
    for q in range(2):
        if mat[q]:
            ws['Kr%d' % q][:, 0] = ws['Kr%d' % q][:, 15]
    assert _bits(t['work2'], want), '%s: work2 is not work with column 0 <- column 15 in the moment blocks of the Matern factors' % case
    K2 = list(K)
    for q in range(2):
        Kd = t['Kd'][q]
        if not mat[q]:
            assert np.all(Kd == _lib.STAGE_SENTINEL), '%s: the K\' image of RBF factor %d was written' % (case, q)
            continue
        rest = np.array(Kd)
        rest[:M[q], :M[q]] = _lib.STAGE_SENTINEL
        assert np.all(rest == _lib.STAGE_SENTINEL), '%s: K\'_%d written beyond [M][M]' % (case, q)
        d64, dld = fm.zz_kd(kinds[q], Z[q], ell[q], var[q]), fm.zz_kd(kinds[q], Z[q], ell[q], var[q], LD)
        _rule(sfx, case, 'Kd%d' % q, Kd[:M[q], :M[q]], d64[0], dld[0], d64[1])
        K2[q] = Kd[:M[q], :M[q]]
    f64, fld = kr.finish(*args, kl), kr.finish(*args, kl, dtype=LD)
    w2 = kr.work_split(t['work2'], cap)
    args2 = (dict(w, Kr0=w2['Kr0'][:M[0]], Kr1=w2['Kr1'][:M[1]]), K2[0], K2[1]) + args[3:]
    g64, gld = kr.finish(*args2, kl), kr.finish(*args2, kl, dtype=LD)
    for q in range(2):
        _rule(sfx, case, 'first%d' % q, t['krow_first'][q], f64['krow%d' % q][0], fld['krow%d' % q][0], f64['krow%d' % q][1])
        _rule(sfx, case, 'second%d' % q, t['krow2'][q], g64['krow%d' % q][0], gld['krow%d' % q][0], g64['krow%d' % q][1])
        merged = np.array(t['krow_first'][q])
        if mat[q]:
            merged[:, cols[q]] = t['krow2'][q][:, cols[q]]
        assert _bits(t['krow'][q], merged), '%s: krow%d is not krow2 in columns 1 .. 2 D of a Matern factor and the first run everywhere else' % (case, q)


@pytest.mark.parametrize('name', ['d11', 'd21-21', 'd31', 'd17', 'd77', 'd21-mix2', 'L32', 'L51', 'L77', 'edgeL-D11'])
def test_finish_stage_with_matern_factors(fused, name):
    from test_gpu_kronf_stages import _check_facts, _unpack, check_assemble
    X, Y, p, gf, gg, D = _finish_fixture(name)
    N = X.shape[0]
    try:
        for kl in (True, False):
            out = _hook(fused, p, X, Y, jitter=J, scale=7.0, include_kl=kl)
            cap, nb = _check_facts(out['facts'], [gf, gg], N, 2)
            for h, tag in enumerate('fg'):
                Z, ell, var = _unpack(p, tag)
                _finish_kinds_latent('%s/%s kl=%d' % (name, tag, kl), kmr.kinds_of(p)[h], cap == (1, 7), out['lat'][h], Z, ell, var, p['u_%ss_sqrt' % tag],
                                     (gf, gg)[h], D, cap, J, kl)
            if kl and name == 'd31':
                check_assemble(name + ' matern', out, p, 'fg')
    finally:      # the hook follows the kinds of the context: leave it as the tests behind this one expect it
        for tag in 'fg':
            for q in range(2):
                fused.set_kron_kernel(tag, q, 'rbf')


@pytest.mark.parametrize('name', ['d31', 'L32'])
def test_hook_with_matern_factors_returns_the_bits_of_an_ordinary_call_and_repeats_its_taps(fused, name):
    """The tapped step of a call with Matern factors -- which also fills the scratch of the second small-grid run, the G regions and the result
    blocks with the stage sentinel -- returns the bits of the ordinary call; every tap, the Matern ones (krow_first, Kd, work2, krow2) and the
    capacity arrays included, repeats between two tapped calls; a call with taps=False and an ordinary call afterwards are unchanged."""
    from test_gpu_kronf_stages import _flat, _same, _rup
    X, Y, p = fm.fixture(name)
    kw = dict(jitter=J, scale=kron_nd.case_scale(name), f_mu=0.2, g_offset=0.1)
    try:
        ed0, kl0, g0 = fused.kron_elbo(p, X, Y, **kw)
        t1 = _hook(fused, p, X, Y, **kw)
        assert (t1['elbo_data'], t1['kl']) == (ed0, kl0) and _same(_flat(t1['grads']), _flat(g0)), 'the tapped step is not the ordinary step'
        t2 = _hook(fused, p, X, Y, **kw)
        small = 'Kd' in t1['lat'][0]
        for h, lat in enumerate(t1['lat']):
            assert 'krow_first' in lat and ('krow2' in lat and 'work2' in lat) == small and ('G' in lat) != small
            for k, v in lat.items():
                vs, ws = (v, t2['lat'][h][k]) if isinstance(v, list) else ([v], [t2['lat'][h][k]])
                if k == 'K':                   # beyond the leading R x R part the buffer is never written
                    Rs = [_rup(P.shape[0], 32) for P in lat['P']]
                    vs, ws = [a[:R, :R] for a, R in zip(vs, Rs)], [a[:R, :R] for a, R in zip(ws, Rs)]
                assert _same(vs, ws), 'tap %s of latent %d differs between two tapped calls' % (k, h)
        t3 = _hook(fused, p, X, Y, taps=False, **kw)
        assert (t3['elbo_data'], t3['kl']) == (ed0, kl0) and _same(_flat(t3['grads']), _flat(g0))
        ed1, kl1, g1 = fused.kron_elbo(p, X, Y, **kw)
        assert (ed1, kl1) == (ed0, kl0) and _same(_flat(g1), _flat(g0)), 'an ordinary call after the tapped ones changed'
    finally:
        for tag in 'fg':
            for q in range(2):
                fused.set_kron_kernel(tag, q, 'rbf')
