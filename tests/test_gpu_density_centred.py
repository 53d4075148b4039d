"""GPU tests of the mode-centred predictive density (include/zigp.h "centred"; k_density_rows<ZIGP_LIK_ONOFF, true> in csrc/zigp_density.hip), in three
tiers, each against tests/density_centred_ref.py:
  sum       at the kernel's OWN returned (zhat, tau) the finite sum is the definition: err_gpu <= 4 err_np + 16 eps S against the
            50-digit sum on the same float64 inputs (the project's rule for point-wise kernels, tests/test_gpu_density.py);
  centre    zhat and tau against centre_np, in units of tau: at most max(8 d, 1e-12), d the distance between centre_np and the same
            search with a seeded +-1 ulp on every link value (what rounding alone does to the search; the device-fit tests' idiom);
  integral  on the stress grid, |logp - integral| <= 2 x the reference's own error on that row + 64 eps S (a centre shifted by a
            fraction of tau moves the quadrature error at second order only).
Then the exact tier (dense end to end, device entry, repeat calls, NULL centre2, rows past N) and the model surface.  The largest
ratios are printed (profiles/density_centred_parity.log)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.io as sio

from conftest import make_problem
import density_ref as R
import density_centred_ref as Q

pytestmark = pytest.mark.gpu
EPS = R.EPS
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
SENT = -7.25


def _sum_tier(tag, rows, ru, out, centre2):
    """the rule, at the kernel's own centre; one 50-digit evaluation"""
    z, t = centre2
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(z)) and np.all(t > 0) and np.all(t <= Q.TAU_MAX)
    truth = Q.logp_centred_mp(rows, z, t, ru)
    err_np = R.err_to(truth, Q.logp_centred_np(rows, z, t, ru))
    S = Q.scales_centred(rows, z, t, ru)
    err = R.err_to(truth, out[0])
    print('%s: %d rows, err_gpu / (eps S) max %.3f (NumPy %.3f)' % (tag, len(S), (err / (EPS * S)).max(), (err_np / (EPS * S)).max()))
    bad = np.nonzero(err > 4 * err_np + 16 * EPS * S)[0]
    assert bad.size == 0, (tag, bad[:5], err[bad[:5]] / (EPS * S[bad[:5]]))


# ---- 1. sum tier -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n', [('grid', 20), ('subset', 1), ('subset', 64), ('subset', 256), ('stress', 64)],
                         ids=['n20-grid', 'n1', 'n64', 'n256', 'n64-stress'])
def test_sum_at_the_kernels_own_centre(engine, kind, n):
    rows, ru = Q.case_rows(kind), Q.rule(n)
    out, total, c2 = engine.density_rows('onoff', *rows, Q.NOISE, rule=ru, centre='mode', return_centre=True)
    assert out.shape == (3, len(rows[0])) and c2.shape == (2, len(rows[0]))
    _sum_tier('centred %s n_quad %d' % (kind, n), rows, ru, out, c2)
    if n == 64 and kind == 'subset':      # the default rule is this one
        assert np.array_equal(engine.density_rows('onoff', *rows, Q.NOISE, centre='mode')[0], out)


def _rows(N, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randn(N) * 2, rs.rand(N) * 0.5, rs.randn(N) * 2, rs.rand(N) * 3, np.where(rs.rand(N) < 0.5, 0.0, rs.randn(N))


def test_sum_across_the_block_boundary(engine):
    """N = 1, 255, 256, 257: each call's rows, centres and sum; the 257-row call carries the 50-digit check, the shorter calls are its
    prefixes bit for bit (a row's result does not depend on its neighbours), nothing is written past N, and the sum is the stable one;
    then the 257 rows at 256 nodes under both centres"""
    rows, ru = _rows(257, seed=7), Q.rule(20)
    out, total, c2 = engine.density_rows('onoff', *rows, Q.NOISE, rule=ru, centre='mode', return_centre=True)
    _sum_tier('centred block boundary', rows, ru, out, c2)
    P = lambda a: a.ctypes.data     # noqa: E731
    for N in (1, 255, 256):
        buf, cbuf, tot = np.full(3 * 257, SENT), np.full(2 * 257, SENT), np.full(1, SENT)
        rc = engine.lib.zigp_density_rows_centred(engine.ctx, *[P(np.ascontiguousarray(a[:N])) for a in rows], N, Q.NOISE, P(ru[0]), P(ru[1]),
                                                  ru[0].size, P(buf), P(tot), P(cbuf))
        assert rc == 0
        assert np.all(buf[3 * N:] == SENT) and np.all(cbuf[2 * N:] == SENT)
        assert np.array_equal(buf[:3 * N].reshape(3, N), out[:, :N]) and np.array_equal(cbuf[:2 * N].reshape(2, N), c2[:, :N])
        o2, t2 = engine.density_rows('onoff', *[a[:N] for a in rows], Q.NOISE, rule=ru, centre='mode')
        assert t2 == tot[0] and np.array_equal(o2, out[:, :N])
        assert abs(tot[0] - np.sum(out[0, :N])) <= N * EPS * np.sum(np.abs(out[0, :N]))
    # N = 257 at n_quad = 256: the one shape at which a full three-column table lies beside two block partials in the layout of scratch2
    # that both centres share.  Each centre against its 50-digit sum; the centre='mean' call that follows the centre='mode' call is what
    # an engine that never ran a centred call gives, bit for bit.
    ru = Q.rule(256)
    assert ru[0].size == 256
    out, total, c2 = engine.density_rows('onoff', *rows, Q.NOISE, rule=ru, centre='mode', return_centre=True)
    mean, mean_total = engine.density_rows('onoff', *rows, Q.NOISE, rule=ru)
    _sum_tier('centred block boundary n_quad 256', rows, ru, out, c2)
    truth = R.logp_mp(*rows, Q.NOISE, *ru)
    err, err_np, S = R.err_to(truth, mean[0]), R.err_to(truth, R.logp_np(*rows, Q.NOISE, *ru)), R.scales(*rows, Q.NOISE, *ru)
    print('gm-centred block boundary n_quad 256: %d rows, err_gpu / (eps S) max %.3f (NumPy %.3f)' % (len(S), (err / (EPS * S)).max(), (err_np / (EPS * S)).max()))
    bad = np.nonzero(err > 4 * err_np + 16 * EPS * S)[0]
    assert bad.size == 0, (bad[:5], err[bad[:5]] / (EPS * S[bad[:5]]))
    assert abs(mean_total - np.sum(mean[0])) <= 257 * EPS * np.sum(np.abs(mean[0]))
    import zigp
    fresh = zigp.DenseEngine(0)
    try:
        fresh_mean, fresh_total = fresh.density_rows('onoff', *rows, Q.NOISE, rule=ru)
    finally:
        fresh.close()
    assert np.array_equal(mean, fresh_mean) and mean_total == fresh_total


# ---- 2. centre tier --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['grid', 'stress'])
def test_centre_against_the_reference_search(engine, kind):
    rows, z, t = Q.centre_case(kind)
    z1, t1 = Q.centre_np(*rows, Q.NOISE, link=Q.ulp_link(1))
    d = max(np.max(np.abs(z1 - z) / t), np.max(np.abs(t1 - t) / t))
    _, _, c2 = engine.density_rows('onoff', *rows, Q.NOISE, n_quad=1, centre='mode', return_centre=True)
    dz, dt = np.abs(c2[0] - z) / t, np.abs(c2[1] - t) / t
    dist = max(dz.max(), dt.max())
    print('centre %s: %d rows, d (seeded +-1 ulp on the link) %.3e, GPU to centre_np %.3e (zhat %.3e, tau %.3e) in units of tau; bar %.3e'
          % (kind, len(z), d, dist, dz.max(), dt.max(), max(8 * d, 1e-12)))
    assert dist <= max(8 * d, 1e-12), (int(np.argmax(np.maximum(dz, dt))), dist, d)


def test_degenerate_rows_have_the_exact_centre(engine):
    """gv = 0 and gv = -1e-18: zhat = 0, tau = 1 exactly, and the same bits as one another"""
    fm, fv, gm, gv, y = _rows(300, seed=2)
    res = [engine.density_rows('onoff', fm, fv, gm, g0, y, Q.NOISE, n_quad=20, centre='mode', return_centre=True)
           for g0 in (np.zeros(300), np.full(300, -1e-18))]
    for out, total, c2 in res:
        assert np.all(c2[0] == 0.0) and np.all(c2[1] == 1.0) and np.all(np.isfinite(out))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ---- 3. integral tier ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [20, 32, 64])
def test_stress_rows_against_the_integral(engine, n):
    rows, z, t = Q.centre_case('stress')
    truth, ru = Q.stress_integral(), Q.rule(n)
    e_ref = R.err_to(truth, Q.logp_centred_np(rows, z, t, ru))
    S = Q.scales_centred(rows, z, t, ru)
    out, total = engine.density_rows('onoff', *rows, Q.NOISE, rule=ru, centre='mode')
    e_gpu = R.err_to(truth, out[0])
    e_mean = R.err_to(truth, engine.density_rows('onoff', *rows, Q.NOISE, rule=ru)[0][0])
    print('integral n_quad %d: GPU centred max %.3e (reference %.3e), largest e_gpu / (2 e_ref + 64 eps S) %.3f; GPU gm-centred max %.3e'
          % (n, e_gpu.max(), e_ref.max(), np.max(e_gpu / (2 * e_ref + 64 * EPS * S)), e_mean.max()))
    bad = np.nonzero(e_gpu > 2 * e_ref + 64 * EPS * S)[0]
    assert bad.size == 0, (bad[:5], e_gpu[bad[:5]], e_ref[bad[:5]])


# ---- 4. exact tier ---------------------------------------------------------------------------------------------------------------
def test_dense_end_to_end_is_bit_consistent(engine):
    """N = 1350 rows through chunks of 1024: predict_density(centre='mode') is density_rows(centre='mode') of predict's rows, bit for bit
    in all three rows, the centre and the sum; ymean and yvar are those of centre='mean'; a second call gives the same bits; the device
    entry equals the host entry; centre2 = NULL changes nothing; the device call writes nothing past N."""
    import torch
    X, Y, p = make_problem(1350, 48, 3, seed=11, Mg=40, ell=0.4)
    N = X.shape[0]
    engine.set_chunk(1024)
    try:
        rows = engine.predict(p, X, jitter=1e-6)
        out, total, c2 = engine.predict_density(p, X, Y, n_quad=20, centre='mode', return_centre=True)
        ref, ref_total, ref_c2 = engine.density_rows('onoff', rows[3], rows[4], rows[5], rows[6], Y, p['noise'], n_quad=20, centre='mode',
                                                     return_centre=True)
        assert out.shape == (3, N) and c2.shape == (2, N)
        assert np.array_equal(out, ref) and total == ref_total and np.array_equal(c2, ref_c2)
        mean, mean_total = engine.predict_density(p, X, Y, n_quad=20)
        assert np.array_equal(out[1], mean[1]) and np.array_equal(out[2], mean[2])
        assert np.array_equal(out[1], rows[0]) and np.array_equal(out[2], (rows[1] + rows[2]) + p['noise'])
        assert not np.array_equal(out[0], mean[0])
        out2, total2 = engine.predict_density(p, X, Y, n_quad=20, centre='mode')          # centre2 = NULL, and a second call
        assert np.array_equal(out2, out) and total2 == total
        none, total_only = engine.predict_density(p, X, Y, n_quad=20, centre='mode', rows_out=False)
        assert none is None and total_only == total
        Xd, Yd = torch.as_tensor(X, device='cuda:0'), torch.as_tensor(Y, device='cuda:0')
        out_d, total_d, c2_d = engine.predict_density_device(p, Xd, Yd, n_quad=20, centre='mode', return_centre=True)
        assert out_d.is_cuda and c2_d.is_cuda and tuple(out_d.shape) == (3, N) and tuple(c2_d.shape) == (2, N)
        assert np.array_equal(out_d.cpu().numpy(), out) and total_d == total and np.array_equal(c2_d.cpu().numpy(), c2)
        out_d2, total_d2 = engine.predict_density_device(p, Xd, Yd, n_quad=20, centre='mode')
        assert np.array_equal(out_d2.cpu().numpy(), out) and total_d2 == total
        # the kernel's own bound: (3, n) and (2, n) device blocks inside larger sentinel buffers, n not a multiple of the block
        from zigp.engine import _Packed
        pk, (x, w), tot = _Packed(p), Q.rule(20), np.zeros(1)
        for n in (1, 257, 1000):
            buf = torch.full((3 * n + 512,), SENT, dtype=torch.float64, device='cuda:0')
            cbuf = torch.full((2 * n + 512,), SENT, dtype=torch.float64, device='cuda:0')
            rc = engine.lib.zigp_predict_density_centred_device(engine.ctx, C.byref(pk.struct), C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), n,
                                                                1e-6, 0.0, x.ctypes.data, w.ctypes.data, x.size, C.c_void_p(buf.data_ptr()),
                                                                tot.ctypes.data, C.c_void_p(cbuf.data_ptr()))
            assert rc == 0
            assert bool(torch.all(buf[3 * n:] == SENT)) and bool(torch.all(cbuf[2 * n:] == SENT))
            assert bool(torch.all(buf[:3 * n] != SENT)) and bool(torch.all(cbuf[:2 * n] != SENT))
        # a host pointer handed to the device call is refused, not dereferenced
        hc = np.zeros(20)
        rc = engine.lib.zigp_predict_density_centred_device(engine.ctx, C.byref(pk.struct), C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), 10,
                                                            1e-6, 0.0, x.ctypes.data, w.ctypes.data, x.size, None, tot.ctypes.data,
                                                            C.c_void_p(hc.ctypes.data))
        assert rc == -1 and b'device memory' in engine.lib.zigp_last_error(engine.ctx)
        # the old path is what it was
        again, again_total = engine.predict_density(p, X, Y, n_quad=20)
        assert np.array_equal(again, mean) and again_total == mean_total
    finally:
        engine.set_chunk(16384)


def test_refusals_match_the_uncentred_calls(engine):
    fm, fv, gm, gv, y = (np.ascontiguousarray(a) for a in _rows(100, seed=4))
    x, w = Q.rule(20)
    out3, tot, c2 = np.full(300, SENT), np.full(1, SENT), np.full(200, SENT)
    P = lambda a: None if a is None else a.ctypes.data     # noqa: E731

    def call(r=(fm, fv, gm, gv, y), N=100, noise=0.01, xs=x, ws=w, nq=20, t=tot):
        return engine.lib.zigp_density_rows_centred(engine.ctx, *[P(a) for a in r], N, noise, P(xs), P(ws), nq, P(out3), P(t), P(c2))
    bad = w.copy()
    bad[3] = 0.0
    for kw, word in [(dict(N=-1), 'N'), (dict(nq=0), 'n_quad'), (dict(nq=257, xs=np.zeros(257), ws=np.full(257, 1 / 257)), 'n_quad'),
                     (dict(ws=bad), 'weights'), (dict(xs=None), 'nodes'), (dict(t=None), 'sum'), (dict(noise=0.0), 'noise'),
                     (dict(r=(fm, fv, None, gv, y)), 'gm')]:
        assert call(**kw) == -1, kw
        assert word in engine.lib.zigp_last_error(engine.ctx).decode(), kw
        assert np.all(out3 == SENT) and tot[0] == SENT and np.all(c2 == SENT), kw
    assert call(N=0) == 0 and tot[0] == 0.0 and np.all(out3 == SENT) and np.all(c2 == SENT)
    with pytest.raises(ValueError, match='n_quad'):
        engine.density_rows('onoff', fm, fv, gm, gv, y, 0.01, rule=(np.zeros(257), np.full(257, 1 / 257)), centre='mode')


# ---- 5. model --------------------------------------------------------------------------------------------------------------------
def test_model_surface_mode_and_mean_agree_on_the_toy_rows():
    """OnOffSVGP.predict_density at 64 nodes, centre='mode' against centre='mean', on the toy fixture.  Each sum has a bar to the integral:
    the rule's rounding term 16 eps S (S of its own reference) plus twice its reference's own distance from integral_mp; the two agree
    within the sum of the two bars.  integral_mp is taken on every 75th row (6 rows: mpmath.quad is slow); the largest difference over
    all rows is printed."""
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    from onoffgpf.OnOffSVGP import JITTER
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(0)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=2.), onoffgpf.kernels.RBF(1, lengthscales=2., variance=5.), OnOffLikelihood(), Z, Z.copy())
    m.likelihood.variance = 0.01
    lp_mean = m.predict_density(X, Y, n_quad=64, centre='mean')
    lp_mode = m.predict_density(X, Y, n_quad=64, centre='mode')
    assert lp_mode.shape == lp_mean.shape == (X.shape[0], 1) and np.all(np.isfinite(lp_mode))
    assert np.array_equal(lp_mean, m.predict_density(X, Y))
    out, total, c2 = m._engine.predict_density(m._values(), X, Y, jitter=JITTER, n_quad=64, centre='mode', return_centre=True)
    assert np.array_equal(lp_mode[:, 0], out[0])
    pr = m._engine.predict(m._values(), X, jitter=JITTER)
    idx = np.arange(0, X.shape[0], 75)
    rows = tuple(np.ascontiguousarray(a[idx]) for a in (pr[3], pr[4], pr[5], pr[6], Y.reshape(-1)))
    ru = Q.rule(64)
    z, t = Q.centre_np(*rows, 0.01)
    truth = Q.integral_mp(rows, z, t, noise=0.01)
    bar_mode = 16 * EPS * Q.scales_centred(rows, z, t, ru, noise=0.01) + 2 * R.err_to(truth, Q.logp_centred_np(rows, z, t, ru, noise=0.01))
    bar_mean = 16 * EPS * R.scales(*rows, 0.01, *ru) + 2 * R.err_to(truth, R.logp_np(*rows, 0.01, *ru))
    diff = np.abs(lp_mode[:, 0] - lp_mean[:, 0])
    print('model surface: |mode - mean| max %.3e over %d rows; on the %d checked rows max %.3e against bars %.3e + %.3e (smallest sum)'
          % (diff.max(), diff.size, idx.size, diff[idx].max(), bar_mode.min(), bar_mean.min()))
    assert np.all(diff[idx] <= bar_mode + bar_mean)
