"""GPU parity of the Matern 3/2 and 5/2 kernels of the dense path (zigp_set_kernel; DenseEngine p['kern_f'] / p['kern_g'];
onoffgpf.kernels.Matern32 / Matern52) against tests/matern_ref.py, the CPU restatement of GPflow 0.4.0's Stationary kernels around the
reference's conditional and KL (checked by tests/test_cpu_matern.py).  Bounds are the project's own for the dense path
(tests/test_gpu_whiten.py): data term 1e-7, KL 1e-8, predict min(max(1e-9, 1e-13 cond), 1e-6), gradients max(1e-6, 1e-13 cond) per block;
cond(Kuu) -- the larger of the two latents', each with its own kernel -- and every measured error are printed."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import relerr
import matern_ref as mr
import fullcov_ref as fr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
ROWS9 = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')

SHAPES = [(1500, 50, 37, 3), (700, 137, 137, 1), (900, 64, 64, 8)]      # N, Mf, Mg, D (tests/test_cpu_matern.py checks their Kuu)
KIND_PAIRS = [('matern52', 'matern52'), ('matern32', 'rbf'), ('rbf', 'matern52')]      # the mixed pairs catch a kind applied to the wrong latent
# every shape with the diagonal parametrisation, the first shape with the two whitened ones as well
CASES = [(s, 'diag') for s in SHAPES] + [(SHAPES[0], 'white'), (SHAPES[0], 'white_full')]


def _cond(p, jitter=1e-6):
    c = []
    for h, t in enumerate('fg'):
        K = mr.kern_K_np(mr.kinds_of(p)[h], p['Z' + t], None, p['ell_' + t], p['var_' + t]) + jitter * np.eye(p['Z' + t].shape[0])
        c.append(float(np.linalg.cond(K)))
    return max(c)


def _problem(shape, mode, kinds):
    X, Y, p = mr.problem(*shape)
    if mode == 'white':
        p['whiten'] = True
    if mode == 'white_full':
        p = fr.make_lq(p, seed=3, negative=2)
    return X, Y, dict(p, kern_f=kinds[0], kern_g=kinds[1])


def _check_grads(tag, g, g_r, c, keys=None):
    worst = 0.0
    for k in (keys or mr.PARAM_KEYS):
        a, b = np.asarray(g[k], dtype=float).reshape(-1), np.asarray(g_r[k], dtype=float).reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        worst = max(worst, e)
        print('  %s grad %-10s relerr %.2e (max |ref| %.3e)' % (tag, k, e, np.max(np.abs(b))))
        assert e < max(1e-6, 1e-13 * c), (k, e)
    return worst


@pytest.mark.parametrize('kinds', KIND_PAIRS, ids=lambda k: '%s-%s' % k)
@pytest.mark.parametrize('shape,mode', CASES, ids=lambda v: v if isinstance(v, str) else 'N%d_M%d_%d_D%d' % v)
def test_elbo_gradient_and_predict_match_reference(engine, shape, mode, kinds):
    X, Y, p = _problem(shape, mode, kinds)
    N = X.shape[0]
    engine.set_chunk(1024)                                 # shape 1: two passes, the second partial
    engine.set_data(X, Y)
    scale = 1.7
    c = _cond(p)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=scale)
    ed_v, kl_v, none = engine.elbo(p, jitter=1e-6, scale=scale, need_grad=False)
    elbo_r, data_r, kl_r, g_r = mr.elbo_and_grad(X, Y, p, 1e-6, scale=scale, chunk=500)
    e_d, e_v, e_k = abs(ed - scale * data_r) / abs(scale * data_r), abs(ed_v - scale * data_r) / abs(scale * data_r), abs(kl - kl_r) / abs(kl_r)
    print('MATERN-PARITY %s %s N=%d M=%d/%d D=%d: cond(Kuu)=%.2e data rel %.2e (value-only %.2e) kl rel %.2e' % (
        '/'.join(kinds), mode, N, shape[1], shape[2], shape[3], c, e_d, e_v, e_k))
    assert none is None and kl_v == kl
    assert e_d <= 1e-7 and e_v <= 1e-7
    assert e_k <= 1e-8
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    w = _check_grads('/'.join(kinds) + ' ' + mode, g, g_r, c)
    kl2 = engine.prior_kl(p)
    assert abs(kl2.sum() - kl) <= 1e-13 * abs(kl)
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    worst_p = 0.0
    for g_off in (0.0, -1.0):
        out = engine.predict(p, X, jitter=1e-6, g_offset=g_off)
        ref = mr.build_predict(X, p, 1e-6, g_off)
        for i, name in enumerate(ROWS9):
            e = relerr(out[i], ref[i])
            worst_p = max(worst_p, e)
            assert e < tol, (name, e, c)
    print('MATERN-PARITY %s %s D=%d: worst gradient block %.2e, worst predict row %.2e (bound %.1e)' % ('/'.join(kinds), mode, shape[3], w, worst_p, tol))
    engine.set_chunk(16384)


def test_predict_device_is_bit_equal_to_predict(engine):
    import torch
    X, Y, p = _problem(SHAPES[0], 'diag', ('matern32', 'matern52'))
    engine.set_chunk(1024)
    out_d = engine.predict_device(p, torch.from_numpy(X).to('cuda:0'), jitter=1e-6)
    assert np.array_equal(out_d.cpu().numpy(), engine.predict(p, X, jitter=1e-6))
    engine.set_chunk(16384)


def test_other_call_options(engine):
    """include_kl = False, a row range that crosses a chunk boundary, select_rows with repeats, g_offset = -1 and a Constant mean, each
    against the reference, at the first shape with (Matern52, Matern32)."""
    X, Y, p = _problem(SHAPES[0], 'diag', ('matern52', 'matern32'))
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    c = _cond(p)

    def check(tag, got, ref, scale=1.0, keys=None, kl=True):
        ed, klv, g = got
        e_r, d_r, kl_r, g_r = ref
        print('MATERN-OPTIONS %s: data rel %.2e' % (tag, abs(ed - scale * d_r) / abs(scale * d_r)))
        assert abs(ed - scale * d_r) <= 1e-7 * abs(scale * d_r)
        assert (abs(klv - kl_r) <= 1e-8 * abs(kl_r)) if kl else (klv == 0.0 and kl_r == 0.0)
        _check_grads(tag, g, g_r, c, keys)

    check('include_kl=0', engine.elbo(p, include_kl=False), mr.elbo_and_grad(X, Y, p, 1e-6, include_kl=False), kl=False)
    lo, hi = 100, 1450                                     # 1350 rows at chunk 1024: two passes, [100, 1124) and [1124, 1450)
    assert engine.get_chunk_rows(50, hi - lo) == 1024
    check('rows [100, 1450)', engine.elbo(p, rows=(lo, hi), scale=2.5), mr.elbo_and_grad(X[lo:hi], Y[lo:hi], p, 1e-6, scale=2.5), scale=2.5)
    ed_v = engine.elbo(p, rows=(lo, hi), scale=2.5, need_grad=False)[0]
    d_r = mr.elbo_and_grad(X[lo:hi], Y[lo:hi], p, 1e-6, need_grad=False)[1]
    assert abs(ed_v - 2.5 * d_r) <= 1e-7 * abs(2.5 * d_r)
    idx = np.random.RandomState(4).randint(0, X.shape[0], size=1300)
    idx[10:20] = idx[0]                                    # repeats
    engine.select_rows(idx)
    check('select_rows', engine.elbo(p, scale=1.5), mr.elbo_and_grad(X[idx], Y[idx], p, 1e-6, scale=1.5), scale=1.5)
    engine.select_rows(None)
    check('g_offset=-1', engine.elbo(p, g_offset=-1.0), mr.elbo_and_grad(X, Y, p, 1e-6, g_offset=-1.0))
    q = dict(p, mean_b=0.37)
    check('Constant mean', engine.elbo(q), mr.elbo_and_grad(X, Y, q, 1e-6), keys=mr.PARAM_KEYS + ('mean_b',))
    out, ref = engine.predict(q, X[:400], g_offset=-1.0), mr.build_predict(X[:400], q, 1e-6, -1.0)
    for i in range(9):
        assert relerr(out[i], ref[i]) < min(max(1e-9, 1e-13 * c), 1e-6), ROWS9[i]
    engine.set_chunk(16384)


@pytest.mark.parametrize('kind', ['matern32', 'matern52'])
def test_kern_K(engine, kind):
    from onoffgpf import kernels
    rs = np.random.RandomState(8)
    X1, X2 = rs.randn(70, 3), rs.randn(33, 3)
    X2[:5] = X1[:5]                                        # coincident pairs
    ell, var = np.array([0.4, 1.1, 2.5]), 2.3
    for B in (X2, None):
        K = engine.kern_K(kind, X1, B, ell, var)
        ref = mr.kern_K_np(kind, X1, B, ell, var)
        e = relerr(K, ref)
        print('KERN-K %s X2 %s: relerr %.2e' % (kind, 'given' if B is not None else 'None', e))
        assert K.shape == ref.shape and e <= 1e-13
    k = (kernels.Matern32 if kind == 'matern32' else kernels.Matern52)(3, variance=var, lengthscales=ell, ARD=True)
    assert np.array_equal(k.compute_K(X1, X2), engine.kern_K(kind, X1, X2, ell, var))
    assert np.array_equal(k.compute_K_symm(X1), engine.kern_K(kind, X1, None, ell, var))
    assert np.array_equal(engine.kern_K('rbf', X1, X2, ell, var), engine.rbf_K(X1, X2, ell, var))
    assert np.array_equal(kernels.RBF(3, variance=var, lengthscales=ell, ARD=True).compute_K(X1, X2), engine.rbf_K(X1, X2, ell, var))
    with pytest.raises(ValueError, match='Matern'):
        engine.kern_K(kind, rs.randn(4, 9), None, 1.0, 1.0)
    with pytest.raises(ValueError, match="'rbf', 'matern32' and 'matern52'"):
        engine.kern_K('matern12', X1, None, ell, var)


def _fit_args(Mf, Mg, D, x, m, v, n_steps, rows, batch):
    from zigp import _lib
    s = _lib.zigp_params()
    s.Mf, s.Mg, s.D = Mf, Mg, D
    o = _lib.zigp_fit_opts()
    for b in range(_lib.DENSE_FIT_BLOCKS):
        o.lr[b], o.positive[b], o.trainable[b] = 0.01, int(b >= 4), 1
    o.ell_size_f = o.ell_size_g = D
    o.beta1, o.beta2, o.eps = 0.9, 0.999, 1e-8
    ed, kl = np.full(n_steps, 7.0), np.full(n_steps, 7.0)
    return (s, o, ed, kl), (C.byref(s), C.byref(o), x.ctypes.data, m.ctypes.data, v.ctypes.data, x.size, 0, n_steps, rows.ctypes.data, batch, 1e-6, 1.0, 1,
                            ed.ctypes.data, kl.ctypes.data)


def test_refusals_name_the_kernel_and_leave_the_context_usable(engine):
    from zigp import _lib
    from zigp.engine import _Packed
    lib, ctx = engine.lib, engine.ctx
    err = lambda: lib.zigp_last_error(ctx).decode()
    X, Y, p = mr.problem(*SHAPES[0])
    q = dict(p, kern_f='matern52', kern_g='matern32')
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    good = engine.elbo(q, jitter=1e-6)
    good_p = engine.predict(q, X[:200])

    def still_good():
        again = engine.elbo(q, jitter=1e-6)
        assert again[0] == good[0] and again[1] == good[1] and all(np.array_equal(np.asarray(again[2][k]), np.asarray(good[2][k])) for k in good[2])
        assert np.array_equal(engine.predict(q, X[:200]), good_p)

    # an unknown kind, latent 2: the setting stays what it was
    assert lib.zigp_set_kernel(ctx, 0, 3) == _lib.ZIGP_EARG and 'unknown kernel kind' in err()
    assert lib.zigp_set_kernel(ctx, 1, -1) == _lib.ZIGP_EARG
    assert lib.zigp_set_kernel(ctx, 2, _lib.KERN_MATERN32) == _lib.ZIGP_EARG and 'latent must be 0 (f) or 1 (g)' in err()
    assert lib.zigp_get_kernel(ctx, 2) == _lib.ZIGP_EARG and lib.zigp_get_kernel(ctx, -1) == _lib.ZIGP_EARG
    assert engine.get_kernel('f') == 'matern52' and engine.get_kernel('g') == 'matern32'
    with pytest.raises(ValueError, match="'rbf', 'matern32' and 'matern52'"):
        engine.elbo(dict(q, kern_g='matern12'))
    assert engine.get_kernel('g') == 'matern32', 'an unknown name raises before anything is set'
    still_good()

    # a Matern latent with D = 9, through the C-ABI (the engine refuses the same before any device work)
    from conftest import make_problem
    X9, Y9, p9 = make_problem(300, 20, 9, seed=2)
    with pytest.raises(ValueError, match="kern_g = 'matern52' and D = 9"):
        engine.elbo(dict(p9, kern_g='matern52'))
    pk = _Packed(p9)
    engine.set_data(X9, Y9)
    base9 = engine.elbo(p9, jitter=1e-6)                   # RBF at D = 9: the wide path, untouched
    for h, kind, name in ((1, _lib.KERN_MATERN52, 'Matern52 kernel on latent g'), (0, _lib.KERN_MATERN32, 'Matern32 kernel on latent f')):
        assert lib.zigp_set_kernel(ctx, h, kind) == 0
        ed, kl = C.c_double(5.0), C.c_double(5.0)
        assert lib.zigp_elbo(ctx, C.byref(pk.struct), 1e-6, 1.0, 0.0, 0, 300, 1, C.byref(ed), C.byref(kl), None) == _lib.ZIGP_EARG
        assert name in err() and 'D = 9' in err() and ed.value == 5.0 and kl.value == 5.0
        out = np.full((9, 300), 3.0)
        assert lib.zigp_predict(ctx, C.byref(pk.struct), X9.ctypes.data, 300, 1e-6, 0.0, out.ctypes.data) == _lib.ZIGP_EARG
        assert name in err() and np.all(out == 3.0)
        kl2 = np.full(2, 3.0)
        assert lib.zigp_prior_kl(ctx, C.byref(pk.struct), 1e-6, kl2.ctypes.data) == _lib.ZIGP_EARG
        assert name in err() and np.all(kl2 == 3.0)
        assert lib.zigp_set_kernel(ctx, h, _lib.KERN_RBF) == 0
        again9 = engine.elbo(p9, jitter=1e-6)
        assert again9[0] == base9[0] and all(np.array_equal(np.asarray(again9[2][k]), np.asarray(base9[2][k])) for k in base9[2])
    engine.set_data(X, Y)
    still_good()

    # both fit-loop calls with a Matern latent: nothing applied, the state unchanged
    N, Mf, Mg, D = SHAPES[0]
    n_free = (Mf + Mg) * D + 2 * (Mf + Mg) + 2 * D + 3
    rs = np.random.RandomState(1)
    inv = lambda v: np.log(np.expm1(np.asarray(v, dtype=np.float64).reshape(-1) - 1e-6))      # Log1pe(1e-6) backwards
    x0 = np.concatenate([p['Zf'].reshape(-1), p['Zg'].reshape(-1), p['u_fm'].reshape(-1), p['u_gm'].reshape(-1), inv(p['u_fs_sqrt']), inv(p['u_gs_sqrt']),
                         inv(p['ell_f']), inv(p['ell_g']), inv(p['var_f']), inv(p['var_g']), inv(p['noise'])])
    assert x0.size == n_free
    rows = np.ascontiguousarray(rs.randint(0, N, size=2 * 100), dtype=np.int64)
    for fn, head in ((lib.zigp_fit_steps, ()), (lib.zigp_fit_steps_mode, (_lib.FIT_DIAG,)), (lib.zigp_fit_steps_mode, (_lib.FIT_WHITE,))):
        for h, kind, name in ((0, _lib.KERN_MATERN52, 'Matern52 kernel on latent f'), (1, _lib.KERN_MATERN32, 'Matern32 kernel on latent g')):
            for hh in (0, 1):
                assert lib.zigp_set_kernel(ctx, hh, kind if hh == h else _lib.KERN_RBF) == 0
            x, m, v = x0.copy(), np.zeros(n_free), np.zeros(n_free)
            keep, args = _fit_args(Mf, Mg, D, x, m, v, 2, rows, 100)
            assert fn(ctx, *head, *args) == _lib.ZIGP_EARG
            assert name in err() and 'device loop' in err()
            assert lib.zigp_fit_steps_applied(ctx) == 0
            assert np.array_equal(x, x0) and not m.any() and not v.any() and np.all(keep[2] == 7.0) and np.all(keep[3] == 7.0)
    shape = dict(Mf=Mf, Mg=Mg, D=D, kern_g='matern52')
    pos, ones = [b >= 4 for b in range(11)], [1] * 11
    for call in (lambda x, m, v: engine.fit_steps(shape, x, m, v, [0.01] * 11, pos, ones, (D, D), 0, 2, rows=rows, batch=100),
                 lambda x, m, v: engine.fit_steps_mode(_lib.FIT_WHITE, shape, x, m, v, [0.01] * 11, pos, ones, (D, D), 0, 2, rows=rows, batch=100)):
        x, m, v = x0.copy(), np.zeros(n_free), np.zeros(n_free)
        with pytest.raises(ValueError, match="kern_g = 'matern52': the device fit loops fit RBF latents only"):
            call(x, m, v)
        assert np.array_equal(x, x0) and not m.any() and not v.any()
    still_good()
    # and with RBF latents the loop runs on the context the Matern calls used (the engine sets both kinds on every call)
    x, m, v = x0.copy(), np.zeros(n_free), np.zeros(n_free)
    ed, kl = engine.fit_steps(dict(Mf=Mf, Mg=Mg, D=D), x, m, v, [0.01] * 11, pos, ones, (D, D), 0, 2, rows=rows, batch=100)
    assert np.all(np.isfinite(ed)) and not np.array_equal(x, x0) and engine.get_kernel('f') == 'rbf' and engine.get_kernel('g') == 'rbf'
    still_good()
    engine.set_chunk(16384)


def _toy_model(minibatch_size=None, seed=0):
    import scipy.io as sio
    from onoffgpf import OnOffSVGP, OnOffLikelihood, kernels
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(seed)
    m = OnOffSVGP(X, Y, kernels.Matern52(1, lengthscales=2.), kernels.Matern52(1, lengthscales=2., variance=5.), OnOffLikelihood(), Z, Z.copy(),
                  minibatch_size=minibatch_size)
    m.likelihood.variance = 0.01
    return m, X, Y


def test_model_with_matern52_latents(engine, tmp_path):
    m, X, Y = _toy_model()
    p = m._values()
    assert p['kern_f'] == 'matern52' and p['kern_g'] == 'matern52'
    engine.set_data(X, Y)
    ed, kl, _ = engine.elbo(p, jitter=1e-6, need_grad=False)
    e0 = m.compute_log_likelihood()
    assert e0 == ed - kl, 'compute_log_likelihood is the engine call'
    e_r = mr.elbo_and_grad(X, Y, p, 1e-6, need_grad=False)[0]
    assert abs(e0 - e_r) <= 1e-7 * abs(e_r)
    assert abs(m.compute_prior_KL() - kl) <= 1e-13 * abs(kl)
    res = m.optimize(maxiter=20)
    e1 = m.compute_log_likelihood()
    print('toy Matern52: ELBO %.4f -> %.4f after %d L-BFGS-B iterations (%d evaluations)' % (e0, e1, res.nit, res.nfev))
    assert e1 > e0
    out = m.predict_onoffgp(X[:50])
    assert len(out) == 9 and all(np.all(np.isfinite(a)) for a in out)
    f = m.savemodel(str(tmp_path / 'm52.pickle'))
    m2 = pickle.load(open(f, 'rb'))
    assert type(m2.kernf).__name__ == 'Matern52' and m2._values()['kern_g'] == 'matern52'
    assert m2.compute_log_likelihood() == e1

    # host Adam at batch 100: the model must not take a device loop
    mb, _, _ = _toy_model(minibatch_size=100, seed=1)
    mb._adam_on_device = lambda *a, **k: pytest.fail('a Matern model took the device fit loop')
    assert not mb._device_fit_eligible(mb._pset())
    z0, l0 = mb.Zf.value.copy(), mb.kernf.lengthscales.value.copy()
    seen = []
    mb.optimize(method='adam', maxiter=30, learning_rate=0.01)
    mb.optimize(method='adam', maxiter=2, learning_rate=0.01, callback=lambda it, e: seen.append(e))
    assert len(seen) == 2 and np.all(np.isfinite(seen))
    assert not np.array_equal(mb.Zf.value, z0) and not np.array_equal(mb.kernf.lengthscales.value, l0)
    assert np.isfinite(mb.compute_log_likelihood())
    with pytest.raises(ValueError, match='kernf is a Matern52 kernel and the device loop fits RBF latents only'):
        mb.optimize(method='adam', maxiter=2, device_loop=True)
