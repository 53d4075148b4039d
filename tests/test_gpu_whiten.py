"""GPU parity of the whitened parametrisation of the dense path (zigp_set_whiten; DenseEngine p['whiten'] = True; OnOffSVGP(whiten=True))
against tests/whiten_ref.py, the CPU restatement of GPConditional(whiten=True) and the white GaussKL (pinned by
tests/test_cpu_whiten_ref.py).  Bounds are the project's own for the dense path (tests/test_gpu_dense.py): predict
min(max(1e-9, 1e-13 cond), 1e-6), data term 1e-7, KL 1e-8, gradients max(1e-6, 1e-13 cond); cond(Kuu) and every measured error are printed."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import make_problem, relerr
import whiten_ref as wr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')

# the case list of tests/test_gpu_dense.py: N, M, Mg, D, ell, chunk, u_scale
CASES = [
    (450, 9, 9, 1, 2.0, None, 0.5),
    (450, 50, 50, 1, 2.0, None, 0.01),
    (2048, 128, 128, 3, 0.3, None, 0.5),
    (3000, 200, 136, 3, 0.25, 1024, 0.5),  # ragged: M not a multiple of 128, Mf != Mg, 3 chunks with a partial last one
    (1500, 300, 300, 2, 0.2, 1024, 0.5),
    (1200, 300, 100, 2, 0.25, 1024, 0.5),
    (1200, 100, 520, 2, 0.25, 1024, 0.5),
    (1500, 96, 140, 4, 0.5, 1024, 0.5),
    (1400, 150, 90, 5, 0.6, 1024, 0.5),
    (1100, 130, 64, 6, 0.7, 1024, 0.5),
    (1000, 64, 64, 7, 0.8, None, 0.5),
    (1300, 150, 100, 8, 0.9, 1024, 0.5),
]
ROWS9 = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')


def _cond(p, jitter=1e-6):
    import zigp_oracle as o
    K = o.rbf_K(p['Zf'], None, p['ell_f'], p['var_f']) + jitter * np.eye(p['Zf'].shape[0])
    return np.linalg.cond(K)


def _problem(N, M, Mg, D, ell, us):
    X, Y, p = make_problem(N, M, D, seed=N + M, Mg=Mg, ell=ell, u_scale=us)
    if D == 1:
        X = X * 10.0
        p['Zf'] *= 10.0
        p['Zg'] *= 10.0
    p['whiten'] = True
    return X, Y, p


def _check_grads(tag, g, g_r, c, keys=None):
    for k in (keys or wr.PARAM_KEYS):
        a, b = np.asarray(g[k], dtype=float).reshape(-1), np.asarray(g_r[k], dtype=float).reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        print('  %s grad %-10s relerr %.2e (max |ref| %.3e)' % (tag, k, e, np.max(np.abs(b))))
        assert e < max(1e-6, 1e-13 * c), (k, e)


@pytest.mark.parametrize('N,M,Mg,D,ell,chunk,us', CASES)
def test_predict_matches_reference(engine, N, M, Mg, D, ell, chunk, us):
    X, Y, p = _problem(N, M, Mg, D, ell, us)
    engine.set_chunk(chunk or 16384)
    c = _cond(p)
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    for g_off in (0.0, -1.0):
        out = engine.predict(p, X, jitter=1e-6, g_offset=g_off)
        ref = wr.build_predict(X, p, 1e-6, g_off)
        for i, name in enumerate(ROWS9):
            e = relerr(out[i], ref[i])
            print('cond(Kuu)=%.2e g_offset %+.0f %s relerr=%.2e' % (c, g_off, name, e))
            assert e < tol, (name, e, c)
    engine.set_chunk(16384)


@pytest.mark.parametrize('N,M,Mg,D,ell,chunk,us', CASES)
def test_elbo_kl_and_gradient_match_reference(engine, N, M, Mg, D, ell, chunk, us):
    X, Y, p = _problem(N, M, Mg, D, ell, us)
    engine.set_chunk(chunk or 16384)
    engine.set_data(X, Y)
    scale = 1.7
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=scale, g_offset=0.0)
    elbo_r, data_r, kl_r, g_r = wr.elbo_and_grad(X, Y, p, 1e-6, scale=scale, chunk=1000)
    c = _cond(p)
    print('cond(Kuu)=%.2e elbo %.10e ref %.10e; data rel %.2e kl rel %.2e' % (
        c, ed - kl, elbo_r, abs(ed - scale * data_r) / abs(scale * data_r), abs(kl - kl_r) / abs(kl_r)))
    assert abs(ed - scale * data_r) <= 1e-7 * abs(scale * data_r)
    assert abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    _check_grads('M=%d/%d D=%d' % (M, Mg, D), g, g_r, c)
    engine.set_chunk(16384)


def test_value_only_no_kl_g_offset_and_prior_kl(engine):
    X, Y, p = make_problem(5000, 150, 3, seed=6, Mg=70)
    p['whiten'] = True
    engine.set_chunk(1024)                                  # five passes, the last one partial
    engine.set_data(X, Y)
    c = _cond(p)
    e_r, d_r, kl_r, g_r = wr.elbo_and_grad(X, Y, p, 1e-6, g_offset=-1.0, chunk=1000)
    ed, kl, g = engine.elbo(p, g_offset=-1.0)
    ed_v, kl_v, g_v = engine.elbo(p, g_offset=-1.0, need_grad=False)
    print('cond %.2e value-only data rel %.2e, gradient-step data rel %.2e, kl rel %.2e' % (
        c, abs(ed_v - d_r) / abs(d_r), abs(ed - d_r) / abs(d_r), abs(kl - kl_r) / abs(kl_r)))
    assert g_v is None
    assert abs(ed_v - d_r) <= 1e-7 * abs(d_r) and abs(ed - d_r) <= 1e-7 * abs(d_r)
    assert abs(kl - kl_r) <= 1e-8 * abs(kl_r) and kl_v == kl
    _check_grads('g_offset=-1', g, g_r, c)
    # without the KL: the value is the data term alone, du and ds lose their KL parts, nothing else moves
    ed_n, kl_n, g_n = engine.elbo(p, g_offset=-1.0, include_kl=False)
    _, _, _, g_rn = wr.elbo_and_grad(X, Y, p, 1e-6, g_offset=-1.0, chunk=1000, include_kl=False)
    assert kl_n == 0.0 and ed_n == ed
    _check_grads('include_kl=0', g_n, g_rn, c)
    for k in ('Zf', 'Zg', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise'):      # the white KL does not depend on Kuu
        assert np.array_equal(np.asarray(g_n[k]), np.asarray(g[k])), k
    ed_vn, kl_vn, _ = engine.elbo(p, g_offset=-1.0, include_kl=False, need_grad=False)
    assert kl_vn == 0.0 and ed_vn == ed_v
    # prior_kl: the two latents' white KLs
    import torch
    want = [float(wr.gauss_kl_white_diag(torch.as_tensor(p['u_%sm' % t]), torch.as_tensor(p['u_%ss_sqrt' % t]))) for t in 'fg']
    got = engine.prior_kl(p)
    assert np.allclose(got, want, rtol=1e-12, atol=0) and abs(got.sum() - kl) <= 1e-14 * abs(kl)
    # stream overlap off: the same kernels in another order of independent work
    engine.set_overlap(False)
    off = (engine.elbo(p, g_offset=-1.0), engine.elbo(p, g_offset=-1.0, need_grad=False), engine.predict(p, X))
    engine.set_overlap(True)
    assert off[0][0] == ed and off[1][0] == ed_v and np.array_equal(off[2], engine.predict(p, X))
    for k in g:
        assert np.array_equal(np.asarray(off[0][2][k]), np.asarray(g[k])), k
    engine.set_chunk(16384)


def test_predict_device_is_bit_equal_to_predict(engine):
    import torch
    X, Y, p = make_problem(3001, 70, 3, seed=12, Mg=45, ell=0.4)
    p['whiten'] = True
    engine.set_chunk(1024)                                  # three passes, the last one partial
    Xd = torch.from_numpy(X).to('cuda:0')
    for g_off in (0.0, -1.0):
        out_d = engine.predict_device(p, Xd, jitter=1e-6, g_offset=g_off)
        out_h = engine.predict(p, X, jitter=1e-6, g_offset=g_off)
        assert out_d.is_cuda and tuple(out_d.shape) == (9, 3001) and np.array_equal(out_d.cpu().numpy(), out_h)
        ref = wr.build_predict(X, p, 1e-6, g_off)
        tol = min(max(1e-9, 1e-13 * _cond(p)), 1e-6)
        for i in range(9):
            assert relerr(out_h[i], ref[i]) < tol, i
    engine.set_chunk(16384)


def test_M2048_and_the_chunk_rule_fallback(engine):
    """M = 2048 / 1100 (16 and 9 row blocks) against the reference on 2500 rows, then 80 000 rows -- beyond the one-pass bound of the chunk
    rule, three passes of 27648 -- against ten passes of 8192 (the bounds of the unwhitened test of the same shape)."""
    engine.set_chunk(0)
    assert engine.get_chunk_rows(2048, 80000) == 27648
    X, Y, p = make_problem(80000, 2048, 3, seed=77, Mg=1100, ell=0.1)
    p['whiten'] = True
    c = _cond(p)
    n = 2500
    engine.set_data(X[:n], Y[:n])
    ed, kl, g = engine.elbo(p, jitter=1e-6)
    e_r, d_r, kl_r, g_r = wr.elbo_and_grad(X[:n], Y[:n], p, 1e-6, chunk=1250)
    print('M=2048: cond(Kuu)=%.2e data rel %.2e kl rel %.2e' % (c, abs(ed - d_r) / abs(d_r), abs(kl - kl_r) / abs(kl_r)))
    assert abs(ed - d_r) <= 1e-7 * abs(d_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('M=2048', g, g_r, c)
    out = engine.predict(p, X[:n], jitter=1e-6)
    ref = wr.build_predict(X[:n], p, 1e-6)
    for i in range(9):
        e = relerr(out[i], ref[i])
        print('  M=2048 predict %s relerr %.2e' % (ROWS9[i], e))
        assert e < min(max(1e-9, 1e-13 * c), 1e-6), i
    engine.set_data(X, Y)
    ed_a, kl_a, g_a = engine.elbo(p, jitter=1e-6)
    engine.set_chunk(8192)
    ed_b, kl_b, g_b = engine.elbo(p, jitter=1e-6)
    assert abs(ed_a - ed_b) <= 1e-10 * abs(ed_a) and kl_a == kl_b
    for k in g_a:
        assert relerr(g_a[k], g_b[k]) <= 1e-7, k
    engine.set_chunk(16384)


def test_linear_mean_function(engine):
    X, Y, p = make_problem(3000, 96, 3, seed=21, ell=0.35)
    p = dict(p, mean_b=0.37, mean_a=np.array([0.5, -0.25, 0.125]), whiten=True)
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    c = _cond(p)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=1.7)
    e_r, d_r, kl_r, g_r = wr.elbo_and_grad(X, Y, p, 1e-6, scale=1.7)
    assert abs(ed - 1.7 * d_r) <= 1e-7 * abs(1.7 * d_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('linear mean', g, g_r, c, keys=wr.PARAM_KEYS + ('mean_a', 'mean_b'))
    out = engine.predict(p, X[:500], jitter=1e-6)
    ref = wr.build_predict(X[:500], p, 1e-6)
    for i in range(9):
        assert relerr(out[i], ref[i]) < min(max(1e-9, 1e-13 * c), 1e-6), i
    engine.set_chunk(16384)


def test_select_rows(engine):
    X, Y, p = make_problem(5000, 70, 3, seed=12)
    p['whiten'] = True
    engine.set_chunk(2048)
    engine.set_data(X, Y)
    idx = np.random.RandomState(3).randint(5000, size=1700)
    engine.select_rows(idx)
    a = engine.elbo(p, jitter=1e-6, scale=5000 / 1700.0)
    engine.select_rows(None)
    engine.set_data(X[idx], Y[idx])
    b = engine.elbo(p, jitter=1e-6, scale=5000 / 1700.0)
    assert a[0] == b[0] and a[1] == b[1]
    for k in a[2]:
        assert np.array_equal(np.asarray(a[2][k]), np.asarray(b[2][k])), k
    e_r, d_r, kl_r, g_r = wr.elbo_and_grad(X[idx], Y[idx], p, 1e-6, scale=5000 / 1700.0)
    assert abs(a[0] - 5000 / 1700.0 * d_r) <= 1e-7 * abs(5000 / 1700.0 * d_r)
    _check_grads('select_rows', a[2], g_r, _cond(p))
    engine.set_chunk(16384)


def test_row_ranges_sum_to_the_whole_range_and_calls_are_bit_stable(engine):
    """Two row ranges, the KL on the first only, against the whole-range call: value to 1e-14, gradients to 1e-10 relative; a second identical
    call is bit-identical.  The split lies on a pass boundary (2 + 2 passes of 1024 rows against 4), so the two sides differ in the order of
    a handful of additions only: O(eps) in the value, in C1 and in K gm; the reverse M x M stage amplifies that by at most cond(Kuu), and
    the case is chosen with cond(Kuu) <= 1e5 for BOTH latents (asserted), i.e. <= 1e-16 x 1e5 = 1e-11 in the gradients."""
    import zigp_oracle as o
    X, Y, p = make_problem(4096, 128, 3, seed=11, ell=0.12)
    p['whiten'] = True
    c = max(_cond(p), np.linalg.cond(o.rbf_K(p['Zg'], None, p['ell_g'], p['var_g']) + 1e-6 * np.eye(128)))
    assert c <= 1e5, c
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p)
    again = engine.elbo(p)
    assert again[0] == ed and again[1] == kl
    for k in g:
        assert np.array_equal(np.asarray(again[2][k]), np.asarray(g[k])), k
    parts = [engine.elbo(p, rows=(0, 2048), include_kl=True), engine.elbo(p, rows=(2048, 4096), include_kl=False)]
    ev = abs(sum(q[0] for q in parts) - ed) / abs(ed)
    print('cond(Kuu)=%.2e row ranges: value rel %.2e' % (c, ev))
    assert ev <= 1e-14
    assert parts[0][1] == kl and parts[1][1] == 0.0
    for k in g:
        s = np.asarray(parts[0][2][k]) + np.asarray(parts[1][2][k])
        e = np.max(np.abs(s - np.asarray(g[k]))) / max(np.max(np.abs(np.asarray(g[k]))), 1e-300)
        print('  row ranges grad %-10s rel %.2e' % (k, e))
        assert e <= 1e-10, (k, e)
    engine.set_chunk(16384)


def test_mode_isolation_on_a_shared_engine(engine):
    """A whitened call leaves nothing behind: unwhitened calls before and after it return the same bits (value-only, gradient step,
    predict, prior_kl), and the whitened results differ from them."""
    X, Y, p = make_problem(3000, 200, 3, seed=3, Mg=136)
    pw = dict(p, whiten=True)
    engine.set_chunk(1024)
    engine.set_data(X, Y)

    def run(q):
        return engine.elbo(q), engine.elbo(q, need_grad=False), engine.predict(q, X[:1500]), engine.prior_kl(q)

    before = run(p)
    white = run(pw)
    assert engine.get_whiten()
    after = run(p)
    assert not engine.get_whiten()
    assert white[0][0] != before[0][0] and white[0][1] != before[0][1]
    assert before[0][0] == after[0][0] and before[0][1] == after[0][1] and before[1][0] == after[1][0]
    for k in before[0][2]:
        assert np.array_equal(np.asarray(before[0][2][k]), np.asarray(after[0][2][k])), k
    assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    engine.set_chunk(16384)


def test_fit_steps_refuses_whitening(engine):
    """zigp_fit_steps with the flag on: ZIGP_EARG and a message that names whitening -- through the C-ABI and through DenseEngine.fit_steps."""
    from zigp import _lib
    X, Y, p = make_problem(2048, 16, 2, seed=1)
    engine.set_data(X, Y)
    n_free = 2 * 16 * 2 + 4 * 16 + 2 + 2 + 3
    x, m, v = np.zeros(n_free), np.zeros(n_free), np.zeros(n_free)
    s = _lib.zigp_params()
    s.Mf, s.Mg, s.D = 16, 16, 2
    o = _lib.zigp_fit_opts()
    for b in range(_lib.DENSE_FIT_BLOCKS):
        o.lr[b], o.positive[b], o.trainable[b] = 0.01, 0, 1
    o.ell_size_f = o.ell_size_g = 2
    o.beta1, o.beta2, o.eps = 0.9, 0.999, 1e-8
    ed, kl = np.zeros(1), np.zeros(1)
    engine.set_whiten(True)
    try:
        rc = engine.lib.zigp_fit_steps(engine.ctx, C.byref(s), C.byref(o), x.ctypes.data, m.ctypes.data, v.ctypes.data, n_free, 0, 1, None, 0, 1e-6,
                                       1.0, 1, ed.ctypes.data, kl.ctypes.data)
        msg = engine.lib.zigp_last_error(engine.ctx).decode()
        assert rc == _lib.ZIGP_EARG and 'whiten' in msg.lower(), (rc, msg)
        assert engine.lib.zigp_fit_steps_applied(engine.ctx) == 0 and not x.any()
    finally:
        engine.set_whiten(False)
    with pytest.raises(ValueError, match='(?i)whiten'):
        engine.fit_steps(dict(Mf=16, Mg=16, D=2, whiten=True), x, m, v, [0.01] * 11, [0] * 11, [1] * 11, (2, 2), 0, 1)
    engine.set_whiten(False)
    assert engine.lib.zigp_set_whiten(engine.ctx, 2) == _lib.ZIGP_EARG and engine.lib.zigp_get_whiten(engine.ctx) == 0
    assert engine.lib.zigp_get_whiten(None) == _lib.ZIGP_EARG


def _toy_model(whiten, num_inducing=10, seed=0):
    """zero-inflated-gpflow.ipynb:52-135 with the whiten switch."""
    import scipy.io as sio
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    kf = onoffgpf.kernels.RBF(1)
    kf.lengthscales = 2.
    kf.variance = 1.
    kg = onoffgpf.kernels.RBF(1)
    kg.lengthscales = 2.
    kg.variance = 5.
    Zf = np.delete(np.linspace(min(X), max(X), num_inducing, endpoint=False), 0).transpose().reshape(-1, 1)
    np.random.seed(seed)
    m = OnOffSVGP(X, Y, kernf=kf, kerng=kg, likelihood=OnOffLikelihood(), Zf=Zf, Zg=Zf.copy(), whiten=whiten)
    m.likelihood.variance = 0.01
    m.likelihood.variance.fixed = False
    return m, X, Y


def test_model_surface(tmp_path):
    m, X, Y = _toy_model(True)
    assert m.whiten is True and m._values()['whiten'] is True and not m._device_fit_eligible(m._pset())
    p = m._values()
    e_r, d_r, kl_r, _ = wr.elbo_and_grad(X, Y, p, 1e-6, need_grad=False)
    e0 = m.compute_log_likelihood()
    print('toy whitened ELBO at init %.10e (reference %.10e), KL %.6e' % (e0, e_r, kl_r))
    assert abs(e0 - e_r) <= 1e-7 * abs(e_r)
    assert abs(m.compute_prior_KL() - kl_r) <= 1e-8 * abs(kl_r)
    m0, _, _ = _toy_model(False)
    assert m0.whiten is False and 'whiten' not in m0._values()
    assert abs(m0.compute_log_likelihood() - e0) > 1e-6 * abs(e0)       # the same numbers mean another model unwhitened
    res = m.optimize(maxiter=30)
    e1 = m.compute_log_likelihood()
    print('toy whitened ELBO after %d L-BFGS-B iterations: %.6f' % (res.nit, e1))
    assert e1 > e0
    p = m._values()
    out = m.predict_onoffgp(X)
    ref = wr.build_predict(X, p, 1e-6)
    c = _cond(p)
    assert len(out) == 9 and all(a.shape == (X.shape[0], 1) for a in out)
    for i in range(9):
        e = relerr(out[i].reshape(-1), ref[i])
        print('  fitted: cond %.2e predict %s relerr %.2e' % (c, ROWS9[i], e))
        assert e < min(max(1e-9, 1e-13 * c), 1e-6), i
    e_fit = wr.elbo_and_grad(X, Y, p, 1e-6, need_grad=False)[0]
    assert abs(e1 - e_fit) <= 1e-7 * abs(e_fit)
    # host Adam follows the switch as well (the device loop is not eligible)
    m.optimize(method='adam', maxiter=3, learning_rate=1e-3)
    # pickle round trip keeps the mode
    f = m.savemodel(str(tmp_path / 'm.pickle'))
    m2 = pickle.load(open(f, 'rb'))
    assert m2.whiten is True
    assert abs(m2.compute_log_likelihood() - m.compute_log_likelihood()) <= 1e-12 * abs(e1)
