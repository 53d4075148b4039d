"""GPU parity of the full-covariance q(u) on the whitened dense model (zigp_set_q_full; DenseEngine p['q_diag'] = False) against
tests/fullcov_ref.py, the CPU restatement of GPConditional(whiten=True) with a 3-d q_sqrt and the white GaussKL's 3-d branch (pinned by
tests/test_cpu_fullcov_ref.py).  Bounds are those of tests/test_gpu_whiten.py: predict min(max(1e-9, 1e-13 cond), 1e-6), data term 1e-7,
KL 1e-8, gradients -- every block, the (M, M) ones included -- max(1e-6, 1e-13 cond) relative to the block's largest entry; cond(Kuu)
and every measured error are printed.  Problems: conftest.make_problem with Lq = diag(s) + (0.1 / sqrt(M)) tril(randn, -1)
(fullcov_ref.make_lq); the variance stays >= sigma^2 - sum A^2 >= 0 for any Lq, so no case is excluded or skipped."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem, relerr
import fullcov_ref as fr

pytestmark = pytest.mark.gpu

# N, Mf, Mg, D, ell, chunk, negative diagonal entries, garbage above the diagonal
CASES = [
    (100, 16, 16, 3, 0.3, None, 0, False),        # one row block, heavy padding
    (2048, 128, 128, 3, 0.3, None, 0, False),     # exact block
    (1500, 300, 150, 2, 0.2, None, 5, False),     # Mf != Mg: 3 and 2 row blocks, N not a multiple of 1024; negative diagonal entries
    (1300, 150, 150, 8, 0.9, None, 0, True),      # D = 8; garbage in the strict upper triangle
    (2048, 1100, 1100, 3, 0.1, None, 0, False),   # 9 row blocks, tail re-deal
    (2500, 128, 128, 3, 0.3, 1024, 0, False),     # three passes with a short last one: C1 split across passes, second chunk_plan
]
IDS = ['N%d-M%d-%d-D%d%s' % (c[0], c[1], c[2], c[3], '-chunk%d' % c[5] if c[5] else '') for c in CASES]
ROWS9 = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')
SCALE = 1.7
_cache = {}


def _cond(p, jitter=1e-6):
    import zigp_oracle as o
    K = o.rbf_K(p['Zf'], None, p['ell_f'], p['var_f']) + jitter * np.eye(p['Zf'].shape[0])
    return np.linalg.cond(K)


def _case(case):
    """problem and reference results of a case, computed once and shared (never modified)"""
    if case not in _cache:
        N, M, Mg, D, ell, chunk, neg, garbage = case
        X, Y, p = make_problem(N, M, D, seed=N + M, Mg=Mg, ell=ell)
        p = fr.make_lq(p, seed=N + M, negative=neg, garbage=garbage)
        _cache[case] = dict(X=X, Y=Y, p=p, cond=_cond(p), elbo=fr.elbo_and_grad(X, Y, p, 1e-6, scale=SCALE, chunk=1024),
                            predict={g: fr.build_predict(X, p, 1e-6, g) for g in (0.0, -1.0)})
    return _cache[case]


def _check_grads(tag, g, g_r, c, keys=None):
    for k in (keys or fr.PARAM_KEYS):
        a, b = np.asarray(g[k], dtype=float), np.asarray(g_r[k], dtype=float)
        if k in ('u_fs_sqrt', 'u_gs_sqrt'):
            assert a.shape == (b.shape[0], b.shape[0]), (k, a.shape)
            assert np.all(np.triu(a, 1) == 0.0), k                           # exactly zero above the diagonal
        a, b = a.reshape(-1), b.reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        print('  %s grad %-10s relerr %.2e (max |ref| %.3e)' % (tag, k, e, np.max(np.abs(b))))
        assert e < max(1e-6, 1e-13 * c), (k, e)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_predict_matches_reference(engine, case):
    q = _case(case)
    X, p, c = q['X'], q['p'], q['cond']
    engine.set_chunk(case[5] or 16384)
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    for g_off in (0.0, -1.0):
        out = engine.predict(p, X, jitter=1e-6, g_offset=g_off)
        ref = q['predict'][g_off]
        for i, name in enumerate(ROWS9):
            e = relerr(out[i], ref[i])
            print('cond(Kuu)=%.2e g_offset %+.0f %s relerr=%.2e' % (c, g_off, name, e))
            assert e < tol, (name, e, c)
    engine.set_chunk(16384)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_elbo_kl_and_gradient_match_reference(engine, case):
    q = _case(case)
    X, Y, p, c = q['X'], q['Y'], q['p'], q['cond']
    engine.set_chunk(case[5] or 16384)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=SCALE)
    ed_v, kl_v, g_v = engine.elbo(p, jitter=1e-6, scale=SCALE, need_grad=False)
    again = engine.elbo(p, jitter=1e-6, scale=SCALE)
    elbo_r, data_r, kl_r, g_r = q['elbo']
    print('cond(Kuu)=%.2e elbo %.10e ref %.10e; data rel %.2e (value-only %.2e) kl rel %.2e; value-only vs gradient call %.2e' % (
        c, ed - kl, elbo_r, abs(ed - SCALE * data_r) / abs(SCALE * data_r), abs(ed_v - SCALE * data_r) / abs(SCALE * data_r),
        abs(kl - kl_r) / abs(kl_r), abs((ed_v - kl_v) - (ed - kl)) / abs(ed - kl)))
    assert abs(ed - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r) and abs(ed_v - SCALE * data_r) <= 1e-7 * abs(SCALE * data_r)
    assert abs(kl - kl_r) <= 1e-8 * abs(kl_r) and kl_v == kl and g_v is None
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    assert abs((ed_v - kl_v) - (ed - kl)) <= 1e-12 * abs(ed - kl)            # W-form (value-only) against R-form (gradient step) variance
    _check_grads('M=%d/%d D=%d' % (case[1], case[2], case[3]), g, g_r, c)
    assert again[0] == ed and again[1] == kl                                 # fixed-order reductions: two identical calls, identical bits
    for k in g:
        assert np.array_equal(np.asarray(again[2][k]), np.asarray(g[k])), k
    engine.set_chunk(16384)


def test_options(engine):
    """include_kl 0 / 1, scale != 1, g_offset = -1, a row range, select_rows with repeats, predict against predict_device -- at
    (1500, 300, 150, 2) with 1024-row passes (two passes, the second short)."""
    import torch
    q = _case(CASES[2])
    X, Y, p, c = q['X'], q['Y'], q['p'], q['cond']
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    for include_kl in (True, False):
        ed, kl, g = engine.elbo(p, jitter=1e-6, scale=0.6, g_offset=-1.0, include_kl=include_kl)
        ed_v, kl_v, _ = engine.elbo(p, jitter=1e-6, scale=0.6, g_offset=-1.0, include_kl=include_kl, need_grad=False)
        e_r, d_r, kl_r, g_r = fr.elbo_and_grad(X, Y, p, 1e-6, scale=0.6, g_offset=-1.0, chunk=1024, include_kl=include_kl)
        assert abs(ed - 0.6 * d_r) <= 1e-7 * abs(0.6 * d_r) and abs(ed_v - ed) <= 1e-12 * abs(ed)
        assert (abs(kl - kl_r) <= 1e-8 * abs(kl_r) and kl_v == kl) if include_kl else (kl == 0.0 and kl_v == 0.0)
        _check_grads('include_kl=%d' % include_kl, g, g_r, c)
    got = engine.prior_kl(p)
    want = [float(fr.gauss_kl_white_full(torch.as_tensor(p['u_%sm' % t]), torch.as_tensor(p['u_%ss_sqrt' % t]))) for t in 'fg']
    assert np.allclose(got, want, rtol=1e-8, atol=0)
    # a row range that starts and ends inside a pass
    r0, r1 = 317, 1403
    ed, kl, g = engine.elbo(p, jitter=1e-6, rows=(r0, r1))
    e_r, d_r, kl_r, g_r = fr.elbo_and_grad(X[r0:r1], Y[r0:r1], p, 1e-6, chunk=1024)
    assert abs(ed - d_r) <= 1e-7 * abs(d_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('rows', g, g_r, c)
    ed0, kl0, g0 = engine.elbo(p, jitter=1e-6, rows=(5, 5))                 # no rows: the KL and its gradient alone
    _, _, _, g_k = fr.elbo_and_grad(X[:0], Y[:0], p, 1e-6)
    assert ed0 == 0.0 and abs(kl0 - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('no rows', g0, g_k, c, keys=('u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt'))
    # a gathered batch with repeated rows
    idx = np.random.RandomState(3).randint(X.shape[0], size=700)
    assert np.unique(idx).size < idx.size
    engine.select_rows(idx)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=X.shape[0] / 700.0)
    engine.select_rows(None)
    e_r, d_r, kl_r, g_r = fr.elbo_and_grad(X[idx], Y[idx], p, 1e-6, scale=X.shape[0] / 700.0, chunk=1024)
    assert abs(ed - X.shape[0] / 700.0 * d_r) <= 1e-7 * abs(X.shape[0] / 700.0 * d_r)
    _check_grads('select_rows', g, g_r, c)
    # predict_device: the bits of predict
    Xd = torch.from_numpy(X).to('cuda:0')
    for g_off in (0.0, -1.0):
        out_d = engine.predict_device(p, Xd, jitter=1e-6, g_offset=g_off)
        assert np.array_equal(out_d.cpu().numpy(), engine.predict(p, X, jitter=1e-6, g_offset=g_off))
    engine.set_chunk(16384)


def test_linear_mean_function(engine):
    q = _case(CASES[1])
    X, Y, c = q['X'], q['Y'], q['cond']
    p = dict(q['p'], mean_b=0.37, mean_a=np.array([0.5, -0.25, 0.125]))
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=1e-6, scale=SCALE)
    e_r, d_r, kl_r, g_r = fr.elbo_and_grad(X, Y, p, 1e-6, scale=SCALE, chunk=1024)
    assert abs(ed - SCALE * d_r) <= 1e-7 * abs(SCALE * d_r) and abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('linear mean', g, g_r, c, keys=fr.PARAM_KEYS + ('mean_a', 'mean_b'))
    out = engine.predict(p, X[:500], jitter=1e-6)
    ref = fr.build_predict(X[:500], p, 1e-6)
    for i in range(9):
        assert relerr(out[i], ref[i]) < min(max(1e-9, 1e-13 * c), 1e-6), i


def test_diagonal_factor_agrees_with_the_diagonal_whitened_mode(engine):
    """Lq = diag(s): ELBO, KL, predict and every shared gradient block agree with the diagonal whitened mode of the same engine within the
    bounds above; diag(dLq) is its ds; the off-diagonal of dLq (not zero: 2 C1 diag(s)) is the reference's."""
    X, Y, p = make_problem(1500, 300, 2, seed=1800, Mg=150, ell=0.2)
    pw = dict(p, whiten=True)
    pf = dict(pw, q_diag=False, u_fs_sqrt=np.diag(p['u_fs_sqrt'].reshape(-1)), u_gs_sqrt=np.diag(p['u_gs_sqrt'].reshape(-1))[:, :, None])
    c = _cond(p)
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    ed_w, kl_w, g_w = engine.elbo(pw, jitter=1e-6, scale=SCALE)
    ed_f, kl_f, g_f = engine.elbo(pf, jitter=1e-6, scale=SCALE)
    print('diag: data rel %.2e kl rel %.2e' % (abs(ed_f - ed_w) / abs(ed_w), abs(kl_f - kl_w) / abs(kl_w)))
    assert abs(ed_f - ed_w) <= 1e-7 * abs(ed_w) and abs(kl_f - kl_w) <= 1e-8 * abs(kl_w)
    g_d = dict(g_f, u_fs_sqrt=np.diagonal(g_f['u_fs_sqrt']), u_gs_sqrt=np.diagonal(g_f['u_gs_sqrt']))
    for k in fr.PARAM_KEYS:
        e = relerr(np.asarray(g_d[k]).reshape(-1), np.asarray(g_w[k]).reshape(-1))
        print('  diag grad %-10s rel %.2e' % (k, e))
        assert e < max(1e-6, 1e-13 * c), (k, e)
    _, _, _, g_r = fr.elbo_and_grad(X, Y, pf, 1e-6, scale=SCALE, chunk=1024)
    _check_grads('diag vs ref', g_f, g_r, c, keys=('u_fs_sqrt', 'u_gs_sqrt'))
    for k in ('u_fs_sqrt', 'u_gs_sqrt'):
        a, b = np.tril(g_f[k], -1), np.tril(np.asarray(g_r[k]).reshape(g_f[k].shape), -1)
        assert np.max(np.abs(b)) > 0 and relerr(a, b) < max(1e-6, 1e-13 * c), k
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    out_w, out_f = engine.predict(pw, X, jitter=1e-6), engine.predict(pf, X, jitter=1e-6)
    for i in range(9):
        assert relerr(out_f[i], out_w[i]) < tol, ROWS9[i]
    assert np.allclose(engine.prior_kl(pf), engine.prior_kl(pw), rtol=1e-8, atol=0)
    engine.set_chunk(16384)


def test_mode_isolation_on_a_shared_engine(engine):
    """A full-covariance call leaves nothing behind: a diagonal whitened call and an unwhitened call return the same bits before and after
    it (value-only, gradient step, predict, prior_kl)."""
    X, Y, p = make_problem(3000, 200, 3, seed=3, Mg=136)
    pw = dict(p, whiten=True)
    pf = fr.make_lq(p, seed=3)
    engine.set_chunk(1024)
    engine.set_data(X, Y)

    def run(q):
        return engine.elbo(q), engine.elbo(q, need_grad=False), engine.predict(q, X[:1500]), engine.prior_kl(q)

    before = [run(p), run(pw)]
    full = run(pf)
    assert engine.get_q_full() and engine.get_whiten()
    after = [run(p), run(pw)]
    assert not engine.get_q_full()
    for b, a in zip(before, after):
        assert full[0][0] != b[0][0] and full[0][1] != b[0][1]
        assert b[0][0] == a[0][0] and b[0][1] == a[0][1] and b[1][0] == a[1][0]
        for k in b[0][2]:
            assert np.array_equal(np.asarray(b[0][2][k]), np.asarray(a[0][2][k])), k
        assert np.array_equal(b[2], a[2]) and np.array_equal(b[3], a[3])
    engine.set_chunk(16384)


def test_refusals(engine):
    """ZIGP_EARG with a message naming the cause, through the C-ABI and through DenseEngine: the mode on with whitening off, zigp_fit_steps
    with the mode on (nothing applied, state untouched), a zero diagonal entry, zigp_set_q_full(ctx, 2), a NULL context."""
    from zigp import _lib
    from zigp.engine import _Packed
    lib, ctx = engine.lib, engine.ctx
    X, Y, p = make_problem(2048, 16, 2, seed=1)
    pf = fr.make_lq(p, seed=1)
    engine.set_data(X, Y)
    assert lib.zigp_set_q_full(ctx, 2) == _lib.ZIGP_EARG and lib.zigp_get_q_full(ctx) == 0
    assert lib.zigp_set_q_full(None, 1) == _lib.ZIGP_EARG and lib.zigp_get_q_full(None) == _lib.ZIGP_EARG
    pk = _Packed(pf)
    ed, kl, kl2, out9 = C.c_double(0), C.c_double(0), np.zeros(2), np.zeros((9, 4))
    try:
        # the mode on, whitening off: every entry point that follows the mode refuses
        engine.set_whiten(False)
        engine.set_q_full(True)
        calls = {'zigp_elbo': lambda: lib.zigp_elbo(ctx, C.byref(pk.struct), 1e-6, 1.0, 0.0, 0, 2048, 1, C.byref(ed), C.byref(kl), None),
                 'zigp_predict': lambda: lib.zigp_predict(ctx, C.byref(pk.struct), X.ctypes.data, 4, 1e-6, 0.0, out9.ctypes.data),
                 'zigp_prior_kl': lambda: lib.zigp_prior_kl(ctx, C.byref(pk.struct), 1e-6, kl2.ctypes.data)}
        for name, call in calls.items():
            rc = call()
            msg = lib.zigp_last_error(ctx).decode()
            assert rc == _lib.ZIGP_EARG and 'whiten' in msg.lower() and 'q_full' in msg, (name, rc, msg)
        assert ed.value == 0.0 and not kl2.any() and not out9.any()
        # zigp_fit_steps with the mode on
        engine.set_whiten(True)
        n_free = 2 * 16 * 2 + 4 * 16 + 2 + 2 + 3
        x, m, v = np.full(n_free, 0.25), np.zeros(n_free), np.zeros(n_free)
        s = _lib.zigp_params()
        s.Mf, s.Mg, s.D = 16, 16, 2
        o = _lib.zigp_fit_opts()
        for b in range(_lib.DENSE_FIT_BLOCKS):
            o.lr[b], o.positive[b], o.trainable[b] = 0.01, 0, 1
        o.ell_size_f = o.ell_size_g = 2
        o.beta1, o.beta2, o.eps = 0.9, 0.999, 1e-8
        h1, h2 = np.zeros(1), np.zeros(1)
        rc = lib.zigp_fit_steps(ctx, C.byref(s), C.byref(o), x.ctypes.data, m.ctypes.data, v.ctypes.data, n_free, 0, 1, None, 0, 1e-6, 1.0, 1,
                                h1.ctypes.data, h2.ctypes.data)
        msg = lib.zigp_last_error(ctx).decode()
        assert rc == _lib.ZIGP_EARG and 'q_diag' in msg and 'q_full' in msg, (rc, msg)
        assert lib.zigp_fit_steps_applied(ctx) == 0 and np.all(x == 0.25) and not m.any() and not v.any()
        # a zero diagonal entry (a negative one is legal)
        bad = dict(pf, u_gs_sqrt=pf['u_gs_sqrt'].copy())
        bad['u_gs_sqrt'][7, 7] = 0.0
        pkz = _Packed(pf)
        pkz.struct.u_gs_sqrt = bad['u_gs_sqrt'].ctypes.data
        rc = lib.zigp_elbo(ctx, C.byref(pkz.struct), 1e-6, 1.0, 0.0, 0, 2048, 1, C.byref(ed), C.byref(kl), None)
        msg = lib.zigp_last_error(ctx).decode()
        assert rc == _lib.ZIGP_EARG and 'zero' in msg and 'u_gs_sqrt' in msg, (rc, msg)
    finally:
        engine.set_q_full(False)
        engine.set_whiten(False)
    # through DenseEngine
    with pytest.raises(ValueError, match='(?i)whiten'):
        engine.elbo(dict(pf, whiten=False))
    with pytest.raises(ValueError, match='(?i)whiten'):
        engine.predict(dict(pf, whiten=False), X[:4])
    with pytest.raises(ValueError, match='zero diagonal'):
        engine.elbo(bad)
    with pytest.raises(ValueError, match='u_fs_sqrt'):
        engine.elbo(dict(pf, u_fs_sqrt=np.ones(16)))
    with pytest.raises(ValueError, match='q_diag'):
        engine.fit_steps(dict(Mf=16, Mg=16, D=2, whiten=True, q_diag=False), x, m, v, [0.01] * 11, [0] * 11, [1] * 11, (2, 2), 0, 1)
    assert np.all(x == 0.25)
    # and a legal call still works afterwards, negative diagonal included
    neg = fr.make_lq(p, seed=1, negative=3)
    ed1, kl1, _ = engine.elbo(neg, jitter=1e-6, need_grad=False)
    e_r, d_r, kl_r, _ = fr.elbo_and_grad(X, Y, neg, 1e-6, need_grad=False)
    assert abs(ed1 - d_r) <= 1e-7 * abs(d_r) and abs(kl1 - kl_r) <= 1e-8 * abs(kl_r)
    # engines that do not ask for the mode do not carry it
    engine.elbo(p, need_grad=False)
    assert not engine.get_q_full() and not engine.get_whiten()
