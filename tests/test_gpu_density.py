"""GPU tests of the predictive density (include/zigp.h "predictive density"; csrc/zigp_density.hip): the rows kernel against the 50-digit
sum of tests/density_ref.py under the project's rule for point-wise kernels (err_gpu <= 4 err_np + 16 eps S, tests/test_gpu_kron_stages.py;
tests/test_cpu_density.py keeps NumPy alone under 4 eps S), the exact tiers, the dense path end to end, the Kronecker rows, the model
surface and every refusal.  The largest err_gpu / (eps S) per likelihood is printed (profiles/density_parity.log)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import scipy.io as sio

from conftest import make_problem
import density_ref as R
import fullcov_ref as fr
import kron_nd as K

pytestmark = pytest.mark.gpu
EPS = R.EPS
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
SENT = -7.25


def _rule_check(tag, got, truth, err_np, S):
    err = R.err_to(truth, got)
    print('%s: %d rows, err_gpu / (eps S) max %.3f (NumPy %.3f)' % (tag, len(S), (err / (EPS * S)).max(), (err_np / (EPS * S)).max()))
    bad = np.nonzero(err > 4 * err_np + 16 * EPS * S)[0]
    assert bad.size == 0, (tag, bad[:5], err[bad[:5]] / (EPS * S[bad[:5]]))


# ---- 1. the rows kernel against the 50-digit sum ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n,full', [(20, True), (1, False), (64, False), (256, False)], ids=['n20-grid', 'n1', 'n64', 'n256'])
def test_onoff_rows_against_the_50_digit_sum(engine, n, full):
    rows, rule, truth, err_np, S = R.onoff_case(n, full)
    out, total = engine.density_rows('onoff', *rows, R.NOISE, rule=rule)
    assert out.shape == (3, len(S)) and np.all(np.isfinite(out))
    _rule_check('onoff n_quad %d' % n, out[0], truth, err_np, S)
    if n == 64:      # the default rule is this one
        assert np.array_equal(engine.density_rows('onoff', *rows, R.NOISE)[0], out)


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_head_rows_against_the_50_digit_closed_form(engine, lik):
    (fm, fv, y), truth, err_np, S = R.head_case(lik)
    out, total = engine.density_rows(lik, fm, fv, None, None, y, R.NOISE)
    _rule_check(lik, out[0], truth, err_np, S)
    ref = R.head_np(lik, fm, fv, y, R.NOISE)
    if lik == 'gaussian':      # ymean = fm, yvar = fv + noise: bit for bit
        assert np.array_equal(out[1], fm) and np.array_equal(out[2], fv + R.NOISE)
    else:                      # ymean = p under the rule's link term; yvar = p (1 - p) composed from the p that was returned, bit for bit
        assert np.all(np.abs(out[1] - ref[1]) <= 16 * EPS * (ref[1] + 0.5 * R.C1))
        assert np.array_equal(out[2], out[1] * (1.0 - out[1]))


# ---- 2. exact tiers --------------------------------------------------------------------------------------------------------------
def _rows(N, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randn(N) * 2, rs.rand(N) * 0.5, rs.randn(N) * 2, rs.rand(N) * 3, np.where(rs.rand(N) < 0.5, 0.0, rs.randn(N))


@pytest.mark.parametrize('N', [1, 63, 64, 65, 1000])
def test_rows_beyond_N_stay_untouched_and_the_sum_is_stable(engine, N):
    fm, fv, gm, gv, y = _rows(1024, seed=N)
    x, w = R.rule(20)
    full = engine.density_rows('onoff', fm, fv, gm, gv, y, R.NOISE, rule=(x, w))[0]
    buf = np.full(3 * 1024, SENT)
    out, total = engine.density_rows('onoff', fm[:N], fv[:N], gm[:N], gv[:N], y[:N], R.NOISE, rule=(x, w), out=buf)
    assert np.all(buf[3 * N:] == SENT) and np.array_equal(out, full[:, :N])
    out2, total2 = engine.density_rows('onoff', fm[:N], fv[:N], gm[:N], gv[:N], y[:N], R.NOISE, rule=(x, w))
    assert total2 == total and np.array_equal(out2, out)
    assert abs(total - np.sum(out[0])) <= N * EPS * np.sum(np.abs(out[0]))
    # the sum alone (out3 = NULL) is the same sum
    tot = np.zeros(1)
    rc = engine.lib.zigp_density_rows(engine.ctx, 0, *[a.ctypes.data for a in (fm, fv, gm, gv, y)], N, R.NOISE, x.ctypes.data, w.ctypes.data,
                                      x.size, None, tot.ctypes.data)
    assert rc == 0 and tot[0] == total


def test_device_rows_beyond_N_stay_untouched(engine):
    """the kernel's own bound: a (3, N) device block inside a larger sentinel buffer, N not a multiple of the block"""
    import torch
    X, Y, p = make_problem(1000, 24, 3, seed=5)
    Xd, Yd = torch.as_tensor(X, device='cuda:0'), torch.as_tensor(Y, device='cuda:0')
    for N in (1, 65, 1000):
        buf = torch.full((3 * N + 512,), SENT, dtype=torch.float64, device='cuda:0')
        out, total = engine.predict_density_device(p, Xd[:N].contiguous(), Yd[:N].contiguous(), n_quad=20, out=buf[:3 * N].view(3, N))
        assert bool(torch.all(buf[3 * N:] == SENT)) and bool(torch.all(buf[:3 * N] != SENT))


def test_negative_zero_variances_count_as_zero(engine):
    fm, fv, gm, gv, y = _rows(300, seed=2)
    z, neg = np.zeros(300), np.full(300, -1e-18)
    for a, b in (((fm, z, gm, gv, y), (fm, neg, gm, gv, y)), ((fm, fv, gm, z, y), (fm, fv, gm, neg, y)), ((fm, z, gm, z, y), (fm, neg, gm, neg, y))):
        ra, rb = engine.density_rows('onoff', *a, R.NOISE, n_quad=20), engine.density_rows('onoff', *b, R.NOISE, n_quad=20)
        assert np.array_equal(ra[0][0], rb[0][0]) and ra[1] == rb[1]


def test_empty_call(engine):
    e = np.zeros(0)
    out, total = engine.density_rows('onoff', e, e, e, e, e, R.NOISE)
    assert out.shape == (3, 0) and total == 0.0


# ---- 3. dense end to end ---------------------------------------------------------------------------------------------------------
def _dense_problem(mode):
    N = 1350
    if mode == 'wide':
        X, Y, p = make_problem(N, 48, 9, seed=11, Mg=40, ell=1.2)
    else:
        X, Y, p = make_problem(N, 48, 3, seed=11, Mg=40, ell=0.4)
    if mode == 'white':
        p['whiten'] = True
    if mode == 'white_full':
        p = fr.make_lq(p, seed=3, negative=2)
    if mode == 'matern':
        p = dict(p, kern_f='matern52')
    if mode == 'constant':
        p = dict(p, mean_b=0.37)
    return X, Y, p


@pytest.mark.parametrize('mode', ['diag', 'white', 'white_full', 'wide', 'matern', 'goff', 'constant'])
def test_predict_density_is_density_rows_of_predict(engine, mode):
    """N = 1350 rows through chunks of 1024 (the rows cross a chunk boundary): logp and the sum are bit-equal to density_rows on
    engine.predict's rows; ymean and yvar are gfmean and (gfvar + gfmeanu) + noise of those rows, bit for bit, and density_rows -- which
    recomputes the three moments from the four rows -- returns the same bits."""
    X, Y, p = _dense_problem(mode)
    goff = -1.0 if mode == 'goff' else 0.0
    engine.set_chunk(1024)
    try:
        rows = engine.predict(p, X, jitter=1e-6, g_offset=goff)
        out, total = engine.predict_density(p, X, Y, jitter=1e-6, g_offset=goff, n_quad=20)
        ref, ref_total = engine.density_rows('onoff', rows[3], rows[4], rows[5], rows[6], Y, p['noise'], n_quad=20)
        assert out.shape == (3, X.shape[0])
        assert np.array_equal(out[0], ref[0]) and total == ref_total
        assert np.array_equal(out[1], rows[0]) and np.array_equal(out[2], (rows[1] + rows[2]) + p['noise'])
        assert np.array_equal(out[1], ref[1]) and np.array_equal(out[2], ref[2])
        none, total_only = engine.predict_density(p, X, Y, jitter=1e-6, g_offset=goff, n_quad=20, rows_out=False)
        assert none is None and total_only == total
        assert np.array_equal(engine.predict(p, X, jitter=1e-6, g_offset=goff), rows)
    finally:
        engine.set_chunk(16384)


def test_predict_density_device_is_bit_equal_to_the_host_call(engine):
    import torch
    X, Y, p = _dense_problem('diag')
    engine.set_chunk(1024)
    try:
        out, total = engine.predict_density(p, X, Y, n_quad=64)
        out_d, total_d = engine.predict_density_device(p, torch.as_tensor(X, device='cuda:0'), torch.as_tensor(Y, device='cuda:0'), n_quad=64)
        assert out_d.is_cuda and tuple(out_d.shape) == (3, X.shape[0])
        assert np.array_equal(out_d.cpu().numpy(), out) and total_d == total
        with pytest.raises(ValueError):
            engine.predict_density_device(p, torch.as_tensor(X), torch.as_tensor(Y, device='cuda:0'))
        # a host pointer handed to the C call is refused, not dereferenced on the device
        from zigp.engine import _Packed
        pk, x, w, tot = _Packed(p), *R.rule(20), np.zeros(1)
        rc = engine.lib.zigp_predict_density_device(engine.ctx, C.byref(pk.struct), C.c_void_p(X.ctypes.data), C.c_void_p(Y.ctypes.data), 10, 1e-6, 0.0,
                                                    x.ctypes.data, w.ctypes.data, x.size, None, tot.ctypes.data)
        assert rc == -1 and b'device memory' in engine.lib.zigp_last_error(engine.ctx)
    finally:
        engine.set_chunk(16384)


def test_predict_density_against_numpy_on_the_oracle_rows(engine):
    """logp of the dense call against logp_np on the ORACLE's predict rows: the rule, plus the predict tolerance of tests/test_gpu_dense.py
    (max(1e-9, 1e-13 cond) of each row's largest entry) carried through the density's derivatives (central differences)."""
    import zigp_oracle as o
    X, Y, p = _dense_problem('diag')
    cond = max(np.linalg.cond(o.rbf_K(p['Z' + t], None, p['ell_' + t], p['var_' + t]) + 1e-6 * np.eye(p['Z' + t].shape[0])) for t in 'fg')
    tol = max(1e-9, 1e-13 * cond)
    ref = [np.asarray(r).reshape(-1) for r in o.build_predict(X, p, 1e-6, 0.0)]
    x, w = R.rule(20)
    y = Y.reshape(-1)
    args = [ref[3], ref[4], ref[5], ref[6]]
    lp = R.logp_np(*args, y, p['noise'], x, w)
    S = R.scales(*args, y, p['noise'], x, w)
    carry = np.zeros_like(lp)
    for k in range(4):
        d = tol * np.max(np.abs(args[k]))
        hi, lo = list(args), list(args)
        hi[k], lo[k] = args[k] + d, args[k] - d
        carry += np.maximum(np.abs(R.logp_np(*hi, y, p['noise'], x, w) - lp), np.abs(R.logp_np(*lo, y, p['noise'], x, w) - lp))
    engine.set_chunk(1024)
    try:
        out, total = engine.predict_density(p, X, Y, n_quad=20)
    finally:
        engine.set_chunk(16384)
    err = np.abs(out[0] - lp)
    print('dense vs oracle rows: cond %.2e, max err / (16 eps S + carry) %.3f' % (cond, np.max(err / (16 * EPS * S + carry))))
    assert np.all(err <= 16 * EPS * S + carry)
    assert np.all(np.abs(out[1] - ref[0]) <= tol * np.max(np.abs(ref[0])))
    assert np.all(np.abs(out[2] - (ref[1] + ref[2] + p['noise'])) <= tol * np.max(np.abs(ref[1] + ref[2] + p['noise'])) * 2)


# ---- 4. Kronecker ----------------------------------------------------------------------------------------------------------------
def test_kron_rows(engine):
    """rows of kron_predict on the small 2-D fixture, fed to density_rows, against logp_np on the same rows under the rule (err_np taken
    against the 50-digit sum of those rows)"""
    X, Y, p = K.problem('d11')
    rows = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
    x, w = R.rule(20)
    y = Y.reshape(-1)
    noise = float(np.squeeze(p['noise']))
    args = (rows[3], rows[4], rows[5], rows[6], y)
    out, total = engine.density_rows('onoff', *args, noise, rule=(x, w))
    truth = R.logp_mp(*args, noise, x, w)
    _rule_check('kron onoff', out[0], truth, R.err_to(truth, R.logp_np(*args, noise, x, w)), R.scales(*args, noise, x, w))
    assert np.all(np.abs(out[1] - rows[0]) <= 8 * EPS * np.abs(rows[0]))
    assert np.all(np.abs(out[2] - ((rows[1] + rows[2]) + noise)) <= 8 * EPS * np.abs((rows[1] + rows[2]) + noise))


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_kron_head_rows(engine, lik):
    X, Y, p = K.problem('d11')
    y = ((Y > 0) * 1.0 if lik == 'bernoulli' else Y).reshape(-1)
    hp = K.head_params(p)
    noise = float(np.squeeze(p['noise']))
    rows = engine.kron_head_predict(hp, X, lik, jitter=K.JITTER, f_mu=0.2 if lik == 'bernoulli' else 0.0)
    out, total = engine.density_rows(lik, rows[0], rows[1], None, None, y, noise)
    truth = R.head_mp(lik, rows[0], rows[1], y, noise)
    _rule_check('kron ' + lik, out[0], truth, R.err_to(truth, R.head_np(lik, rows[0], rows[1], y, noise)[0]), R.head_scales(lik, rows[0], rows[1], y, noise))
    if lik == 'bernoulli':     # the probability IS pfmean: same link, same rows
        assert np.array_equal(out[1], rows[2])
    else:
        assert np.array_equal(out[1], rows[2]) and np.array_equal(out[2], rows[3])


# ---- 5. model --------------------------------------------------------------------------------------------------------------------
def test_model_predict_y_and_predict_density(tmp_path):
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    from onoffgpf.OnOffSVGP import JITTER
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(0)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=2.), onoffgpf.kernels.RBF(1, lengthscales=2., variance=5.), OnOffLikelihood(), Z, Z.copy())
    m.likelihood.variance = 0.01
    before = m.predict_onoffgp(X)
    N = X.shape[0]
    ymean, yvar = m.predict_y(X)
    lp = m.predict_density(X, Y)
    assert ymean.shape == yvar.shape == lp.shape == (N, 1) and np.all(np.isfinite(lp))
    out, total = m._engine.predict_density(m._values(), X, Y, jitter=JITTER, n_quad=64)
    rows = m._engine.predict(m._values(), X, jitter=JITTER)
    assert np.array_equal(lp[:, 0], out[0]) and np.array_equal(ymean[:, 0], out[1]) and np.array_equal(yvar[:, 0], out[2])
    assert np.array_equal(ymean[:, 0], rows[0]) and np.array_equal(yvar[:, 0], (rows[1] + rows[2]) + 0.01)
    assert not np.array_equal(m.predict_density(X, Y, n_quad=20), lp)
    f = m.savemodel(str(tmp_path / 'm.pickle'))
    m2 = pickle.load(open(f, 'rb'))
    assert np.array_equal(m2.predict_density(X, Y), lp)
    y2 = m2.predict_y(X)
    assert np.array_equal(y2[0], ymean) and np.array_equal(y2[1], yvar)
    for a, b in zip(m.predict_onoffgp(X), before):      # untouched
        assert np.array_equal(a, b)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_everything_as_it_was(engine):
    from zigp.engine import _Packed
    import torch
    lib, ctx = engine.lib, engine.ctx
    X, Y, p = make_problem(700, 24, 3, seed=9)
    engine.set_data(X, Y)
    elbo0, pred0 = engine.elbo(p, need_grad=False), engine.predict(p, X)
    dens0 = engine.predict_density(p, X, Y, n_quad=20)
    pk = _Packed(p)
    fm, fv, gm, gv, y = (np.ascontiguousarray(a) for a in _rows(700, seed=4))
    x, w = R.rule(20)
    x257, w257 = np.zeros(257), np.full(257, 1.0 / 257)
    out3, tot = np.full(3 * 700, SENT), np.full(1, SENT)
    Xd, Yd = torch.as_tensor(X, device='cuda:0'), torch.as_tensor(Y, device='cuda:0')
    out3d = torch.full((3, 700), SENT, dtype=torch.float64, device='cuda:0')
    P = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    D = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731

    def rows_call(lik=0, r=(fm, fv, gm, gv, y), N=700, noise=0.01, xs=x, ws=w, nq=20, o=out3, t=tot):
        return lib.zigp_density_rows(ctx, lik, *[P(a) for a in r], N, noise, P(xs), P(ws), nq, P(o), P(t))

    def dense_call(N=700, Xn=X, Yn=Y, xs=x, ws=w, nq=20, o=out3, t=tot, pp=pk):
        return lib.zigp_predict_density(ctx, C.byref(pp.struct), P(Xn), P(Yn), N, 1e-6, 0.0, P(xs), P(ws), nq, P(o), P(t))

    def device_call(N=700, Xn=Xd, Yn=Yd, xs=x, ws=w, nq=20, o=out3d, t=tot, pp=pk):
        return lib.zigp_predict_density_device(ctx, C.byref(pp.struct), D(Xn), D(Yn), N, 1e-6, 0.0, P(xs), P(ws), nq, D(o), P(t))

    def bad_w(v):
        b = w.copy()
        b[7] = v
        return b

    bad_noise = _Packed(dict(p, noise=-0.01))
    for call in (rows_call, dense_call, device_call):
        cases = [(dict(N=-1), 'N'), (dict(nq=0), 'n_quad'), (dict(nq=257, xs=x257, ws=w257), 'n_quad'), (dict(ws=bad_w(0.0)), 'weights'),
                 (dict(ws=bad_w(-0.1)), 'weights'), (dict(ws=bad_w(np.inf)), 'weights'), (dict(ws=bad_w(np.nan)), 'weights'),
                 (dict(xs=None), 'nodes'), (dict(ws=None), 'weights'), (dict(t=None), 'sum')]
        if call is rows_call:
            cases += [(dict(lik=3), 'lik'), (dict(lik=-1), 'lik'), (dict(noise=0.0), 'noise'), (dict(noise=-1.0), 'noise'), (dict(lik=1, noise=0.0), 'noise'),
                      (dict(r=(None, fv, gm, gv, y)), 'fm'), (dict(r=(fm, fv, None, gv, y)), 'gm'), (dict(r=(fm, fv, gm, gv, None)), 'y'),
                      (dict(lik=1, r=(fm, None, None, None, y)), 'fv')]
        else:
            cases += [(dict(Xn=None), 'Xnew'), (dict(Yn=None), 'Ynew'), (dict(pp=bad_noise), 'variances')]
        for kw, word in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            assert word in lib.zigp_last_error(ctx).decode(), (call.__name__, kw, lib.zigp_last_error(ctx))
            assert np.all(out3 == SENT) and tot[0] == SENT and bool(torch.all(out3d == SENT)), (call.__name__, kw)
    from zigp import _lib
    for name in ('zigp_density_rows', 'zigp_predict_density', 'zigp_predict_density_device'):      # a NULL context
        args = [1 if t in (C.c_int32, C.c_int64) else 1.0 if t is C.c_double else None for t in _lib.SIGNATURES[name][1]]
        args[-2], args[-1] = (D(out3d) if name.endswith('device') else P(out3)), P(tot)
        assert getattr(lib, name)(*args) == -1 and np.all(out3 == SENT) and tot[0] == SENT and bool(torch.all(out3d == SENT))
    # N = 0 is fine: sum 0, the rows untouched
    assert rows_call(N=0) == 0 and tot[0] == 0.0 and np.all(out3 == SENT)
    tot[0] = SENT
    assert dense_call(N=0) == 0 and tot[0] == 0.0
    # the context works as before
    again = engine.elbo(p, need_grad=False)
    assert again[0] == elbo0[0] and again[1] == elbo0[1] and np.array_equal(engine.predict(p, X), pred0)
    dens = engine.predict_density(p, X, Y, n_quad=20)
    assert np.array_equal(dens[0], dens0[0]) and dens[1] == dens0[1]
    with pytest.raises(ValueError, match='n_quad'):
        engine.density_rows('onoff', fm, fv, gm, gv, y, 0.01, rule=(x257, w257))
    with pytest.raises(ValueError, match='weights'):
        engine.predict_density(p, X, Y, rule=(x, bad_w(0.0)))
