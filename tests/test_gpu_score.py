"""GPU tests of the predictive scores (include/zigp.h "predictive scores"; csrc/zigp_score.hip): the CDF pair, the quantiles and the CRPS
against the 50-digit sums of tests/score_ref.py under the project's rule (err_gpu <= 4 err_np + 16 eps S; tests/test_cpu_score.py keeps
NumPy alone under 8 eps S), against the NumPy sums at the rule sizes that exercise the lane mapping, the exact tiers (row counts, sentinels,
position, repeat), the consistency of the three quantities, the Gaussian head, every refusal, the dense path end to end, the Kronecker
rows and the model surface.  The largest error per quantity and rule size is printed in units of eps S (profiles/score_parity.log)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.io as sio

from conftest import make_problem
import density_ref as R
import fullcov_ref as fr
import kron_nd as K
import score_ref as S

pytestmark = pytest.mark.gpu
EPS = R.EPS
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
SENT = -7.25
LEVELS = S.LEVELS + (0.05,)          # the five levels, plus an unsorted duplicate


def _bar(tag, got, truth, err_np, scale):
    """err_gpu <= 4 err_np + 16 eps S against the 50-digit value; where S = 0 (the tail underflows) the result is an exact 0"""
    err = S.err_to(truth, got)
    ok = scale > 0
    print('%s: %d rows, err_gpu / (eps S) max %.3f (NumPy %.3f)' % (tag, len(scale), (err[ok] / (EPS * scale[ok])).max(), (err_np[ok] / (EPS * scale[ok])).max()))
    bad = np.nonzero(err > 4 * err_np + 16 * EPS * scale)[0]
    assert bad.size == 0, (tag, bad[:5], err[bad[:5]], scale[bad[:5]])
    assert np.all(np.asarray(got)[~ok] == 0.0), tag


def _quantile_bar(tag, rows4, rule, n, which, p, t):
    """the residual in probability of the GPU's t against 4 x the bisection's plus 16 (eps S_F(t) + ulp(t) pdf(t))"""
    res = S.quantile_residual(*rows4, S.NOISE, *rule, p, t)
    unit = S.quantile_scale(*rows4, S.NOISE, *rule, p, t)
    res_np = S.quantile_case(n, which, p)[1]
    print('%s p = %.10g: residual / (eps S_F + ulp pdf) max %.3f (bisection %.3f)' % (tag, p, (res / unit).max(), (res_np / unit).max()))
    bad = np.nonzero(res > 4 * res_np + 16 * unit)[0]
    assert bad.size == 0, (tag, p, bad[:5], res[bad[:5]], unit[bad[:5]])


# ---- 1. against the 50-digit sums ------------------------------------------------------------------------------------------------
def test_cdf_pair_on_the_full_grid_against_the_50_digit_sums(engine):
    rows, rule, truth, err_np, scale = S.cdf_case(20, 'grid')
    r = engine.score_rows('onoff', *rows, S.NOISE, rule=rule, crps=False)
    assert r['crps'] is None and r['crps_sum'] is None and r['quantiles'] is None and r['cdf'].shape == r['sf'].shape == (675,)
    _bar('CDF F  n_quad 20 grid', r['cdf'], truth[0], err_np[0], scale[0])
    _bar('CDF SF n_quad 20 grid', r['sf'], truth[1], err_np[1], scale[1])


@pytest.mark.parametrize('n,which', [(20, 'subset'), (64, 'fifth')], ids=['n20-subset', 'n64-fifth'])
def test_all_three_against_the_50_digit_sums(engine, n, which):
    rows, rule, truth, err_np, scale = S.cdf_case(n, which)
    r = engine.score_rows('onoff', *rows, S.NOISE, rule=rule, levels=LEVELS)
    tag = 'n_quad %d %s' % (n, which)
    _bar('CDF F  ' + tag, r['cdf'], truth[0], err_np[0], scale[0])
    _bar('CDF SF ' + tag, r['sf'], truth[1], err_np[1], scale[1])
    _, _, t_c, err_c, S_C = S.crps_case(n, which)
    _bar('CRPS   ' + tag, r['crps'], t_c, err_c, S_C)
    assert abs(r['crps_sum'] - np.sum(r['crps'])) <= len(S_C) * EPS * np.sum(np.abs(r['crps']))
    q = r['quantiles']
    assert q.shape == (len(LEVELS), len(S_C)) and np.all(np.isfinite(q))
    for l, p in enumerate(S.LEVELS):
        _quantile_bar('quantile ' + tag, rows[:4], rule, n, which, p, q[l])
    assert np.array_equal(q[5], q[1])          # the duplicate level: the same bits
    if n == 64:      # the default rule is this one
        d = engine.score_rows('onoff', *rows, S.NOISE, levels=LEVELS)
        assert all(np.array_equal(d[k], r[k]) for k in ('cdf', 'sf', 'quantiles', 'crps')) and d['crps_sum'] == r['crps_sum']


# ---- 2. against the NumPy sums, at the rule sizes that exercise the lane mapping and the tail of the table -------------------------
@pytest.mark.parametrize('n', [1, 7, 32, 33, 63, 64, 65, 200, 256, -20])
def test_rule_sizes_against_numpy(engine, n, monkeypatch):
    """|gpu - np| <= 5 err_floor + 16 eps S, err_floor = the 8 eps S that tests/test_cpu_score.py asserts for NumPy alone; the quantile in
    probability, by NumPy's own sum at the GPU's t, in units of eps S_F + ulp pdf.  32 / 33 is where a row goes from half a wave to a whole
    one; -20 is 20 nodes with a whole wave per row (ZIGP_SCORE_WAVE_PER_ROW=1, the other arm of tools/score_time.py)."""
    if n < 0:
        monkeypatch.setenv('ZIGP_SCORE_WAVE_PER_ROW', '1')
        n = -n
    rows = tuple(np.ascontiguousarray(c[:16]) for c in R.subset())
    x, w = S._rule(n)
    r = engine.score_rows('onoff', *rows, S.NOISE, rule=(x, w), levels=S.LEVELS)
    F, SF = S.cdf_np(*rows, S.NOISE, x, w)
    SFl, SFu = S.cdf_scales(*rows, S.NOISE, x, w)
    S_C = S.crps_scale(*rows, S.NOISE, x, w)
    bar = 5 * S.FLOOR + 16
    for tag, got, ref, scale in (('F', r['cdf'], F, SFl), ('SF', r['sf'], SF, SFu), ('CRPS', r['crps'], S.crps_np(*rows, S.NOISE, x, w), S_C)):
        ok = scale > 0
        print('n_quad %3d %-4s: |gpu - np| / (eps S) max %.3f' % (n, tag, (np.abs(got - ref)[ok] / (EPS * scale[ok])).max()))
        assert np.all(np.abs(got - ref) <= bar * EPS * scale), (n, tag)
    for l, p in enumerate(S.LEVELS):
        t = r['quantiles'][l]
        G = S.cdf_np(*rows[:4], t, S.NOISE, x, w)
        res = np.abs(G[0] - p) if p <= 0.5 else np.abs(G[1] - (1.0 - p))
        unit = S.quantile_scale(*rows[:4], S.NOISE, x, w, p, t)
        print('n_quad %3d quantile p = %.10g: residual / (eps S_F + ulp pdf) max %.3f' % (n, p, (res / unit).max()))
        assert np.all(res <= bar * unit), (n, p)


# ---- 3. row counts and buffers ---------------------------------------------------------------------------------------------------
def _rows(N, seed=0):
    rs = np.random.RandomState(seed)
    return tuple(np.ascontiguousarray(a) for a in (rs.randn(N) * 2, rs.rand(N) * 0.5, rs.randn(N) * 2, rs.rand(N) * 3,
                                                   np.where(rs.rand(N) < 0.5, 0.0, rs.randn(N))))


def _raw(engine, lik, rows, N, rule, levels, pad=64):
    """the C call on sentinel-backed buffers: (cdf2, quant, crps) views of the first entries, the sum, and the three whole buffers"""
    x, w = rule
    lv = np.ascontiguousarray(levels, dtype=np.float64)
    L = lv.size
    bufs = [np.full(2 * N + pad, SENT), np.full(L * N + pad, SENT), np.full(N + pad, SENT)]
    tot = np.full(1, SENT)
    P = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    rc = engine.lib.zigp_score_rows(engine.ctx, lik, *[P(a) for a in rows], N, S.NOISE, P(x), P(w), x.size, P(lv), L, *[P(b) for b in bufs], P(tot))
    assert rc == 0, engine.lib.zigp_last_error(engine.ctx)
    assert np.all(bufs[0][2 * N:] == SENT) and np.all(bufs[1][L * N:] == SENT) and np.all(bufs[2][N:] == SENT)
    return bufs[0][:2 * N].reshape(2, N), bufs[1][:L * N].reshape(L, N), bufs[2][:N], tot[0]


@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_row_counts_sentinels_position_and_repeat(engine, N):
    """OnOff at 20 nodes (half a wave per row, eight rows per block) and at 64 (a whole wave, four rows per block) and the Gaussian head
    (256 rows per block): nothing is written behind an output, a row has the same bits at every position and every N, and a second call
    repeats every bit, the sum included"""
    levels = (0.05, 0.5, 0.95)
    full = _rows(1024, seed=11)
    for lik, rule in ((0, R.rule(20)), (0, R.rule(64)), (1, R.rule(20))):
        pick = (lambda c: c) if lik == 0 else (lambda c: (c[0], c[1] + 0.01, None, None, c[4]))
        whole = _raw(engine, lik, pick(full), 1024, rule, levels)
        head = tuple(np.ascontiguousarray(c[:N]) for c in full)
        a = _raw(engine, lik, pick(head), N, rule, levels)
        b = _raw(engine, lik, pick(head), N, rule, levels)
        for u, v, wh in zip(a[:3], b[:3], whole[:3]):
            assert np.array_equal(u, v) and np.array_equal(u, wh[..., :N]) and np.all(u != SENT)
        assert a[3] == b[3] and abs(a[3] - np.sum(a[2])) <= N * EPS * np.sum(np.abs(a[2]))
        rev = tuple(np.ascontiguousarray(c[::-1]) for c in head)          # the same rows at other positions
        r = _raw(engine, lik, pick(rev), N, rule, levels)
        for u, v in zip(a[:3], r[:3]):
            assert np.array_equal(u, v[..., ::-1])


def test_empty_call_and_partial_requests(engine):
    e = np.zeros(0)
    r = engine.score_rows('onoff', e, e, e, e, e, S.NOISE, levels=(0.5,))
    assert r['crps_sum'] == 0.0 and r['cdf'].shape == (0,) and r['quantiles'].shape == (1, 0)
    rows = _rows(100, seed=3)
    allr = engine.score_rows('onoff', *rows, S.NOISE, n_quad=20, levels=(0.25, 0.75))
    q = engine.score_rows('onoff', *rows[:4], None, S.NOISE, n_quad=20, levels=(0.25, 0.75))          # no y: the quantiles alone
    assert q['cdf'] is None and q['sf'] is None and q['crps'] is None and q['crps_sum'] is None and np.array_equal(q['quantiles'], allr['quantiles'])
    c = engine.score_rows('onoff', *rows, S.NOISE, n_quad=20, crps=False)
    assert c['crps'] is None and c['quantiles'] is None and np.array_equal(c['cdf'], allr['cdf']) and np.array_equal(c['sf'], allr['sf'])
    s = engine.score_rows('onoff', *rows, S.NOISE, n_quad=20, cdf=False)
    assert s['cdf'] is None and np.array_equal(s['crps'], allr['crps']) and s['crps_sum'] == allr['crps_sum']


def test_negative_zero_variances_count_as_zero(engine):
    fm, fv, gm, gv, y = _rows(300, seed=2)
    z, neg = np.zeros(300), np.full(300, -1e-18)
    for a, b in (((fm, z, gm, gv, y), (fm, neg, gm, gv, y)), ((fm, fv, gm, z, y), (fm, fv, gm, neg, y)), ((fm, z, gm, z, y), (fm, neg, gm, neg, y))):
        ra, rb = (engine.score_rows('onoff', *r, S.NOISE, n_quad=20, levels=(0.05, 0.5)) for r in (a, b))
        assert all(np.array_equal(ra[k], rb[k]) for k in ('cdf', 'sf', 'quantiles', 'crps')) and ra['crps_sum'] == rb['crps_sum']


# ---- 4. consistency --------------------------------------------------------------------------------------------------------------
def test_the_three_quantities_are_consistent(engine):
    rows = _rows(500, seed=7)
    x, w = R.rule(64)
    levels = (1e-9, 1e-3, 0.05, 0.5, 0.95, 1.0 - 1e-3, 1.0 - 1e-9)
    r = engine.score_rows('onoff', *rows, S.NOISE, rule=(x, w), levels=levels)
    SFl, SFu = S.cdf_scales(*rows, S.NOISE, x, w)
    total = np.sum(w)
    assert np.all(np.abs((r['cdf'] + r['sf']) - total) <= (S.FLOOR + 16) * EPS * (SFl + SFu) + 4 * EPS)          # F + SF = sum w = 1, within the summed bounds
    assert np.all(r['crps'] > 0)
    q = r['quantiles']
    assert np.all(np.diff(q, axis=0) >= 0)
    for l, p in enumerate(levels):          # inside the stated bracket, up to the rounding of its own ends
        lo, hi = S.bracket(*rows[:4], S.NOISE, x, w, p)
        slack = 64 * EPS * (np.abs(lo) + np.abs(hi) + 1.0)
        assert np.all((q[l] >= lo - slack) & (q[l] <= hi + slack)), p


# ---- 5. the Gaussian head --------------------------------------------------------------------------------------------------------
def test_gaussian_head_against_the_50_digit_closed_forms(engine):
    fm, fv, y = R.head_grid('gaussian')
    r = engine.score_rows('gaussian', fm, fv, None, None, y, S.NOISE, levels=S.LEVELS)
    truth = S.head_mp(fm, fv, y, S.NOISE)
    ref = S.head_np(fm, fv, y, S.NOISE, S.LEVELS)
    scale = S.head_scales(fm, fv, y, S.NOISE)
    for k, (tag, key) in enumerate((('F', 'cdf'), ('SF', 'sf'), ('CRPS', 'crps'))):
        _bar('gaussian head ' + tag, r[key], truth[k], S.err_to(truth[k], ref[k]), scale[k])
    for l, p in enumerate(S.LEVELS):
        res, unit = S.head_quantile_residual(fm, fv, S.NOISE, p, r['quantiles'][l])
        res_np, _ = S.head_quantile_residual(fm, fv, S.NOISE, p, ref[3][l])
        print('gaussian head quantile p = %.10g: residual / (eps S_F + ulp pdf) max %.3f (NumPy %.3f)' % (p, (res / unit).max(), (res_np / unit).max()))
        assert np.all(res <= 4 * res_np + 16 * unit), p


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_results_as_they_were(engine):
    rows = _rows(200, seed=4)
    x, w = R.rule(20)
    levels = (0.05, 0.5, 0.95)

    def legal():
        return engine.score_rows('onoff', *rows, S.NOISE, rule=(x, w), levels=levels)

    def same(a, b):
        return all(np.array_equal(a[k], b[k]) for k in ('cdf', 'sf', 'quantiles', 'crps')) and a['crps_sum'] == b['crps_sum']
    before = legal()
    with pytest.raises(ValueError, match='Bernoulli.*Brier'):
        engine.score_rows('bernoulli', rows[0], rows[1], None, None, rows[4], S.NOISE)
    assert same(legal(), before)
    for bad in (0.0, 1.0, np.nan, -0.1, np.inf):
        with pytest.raises(ValueError, match='levels'):
            engine.score_rows('onoff', *rows, S.NOISE, rule=(x, w), levels=(0.5, bad))
        assert same(legal(), before)
    with pytest.raises(ValueError, match='levels'):
        engine.score_rows('onoff', *rows, S.NOISE, rule=(x, w), levels=np.linspace(0.1, 0.9, 17))
    # the C call itself: 17 levels, a NULL y with crps asked for, n_levels = 0 with levels given -- outputs untouched
    P = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    lv17, lv3 = np.linspace(0.1, 0.9, 17), np.array(levels)
    bufs = [np.full(2 * 200, SENT), np.full(17 * 200, SENT), np.full(200, SENT), np.full(1, SENT)]

    def call(r=rows, lv=lv3, L=3, out=(0, 1, 2, 3), lik=0, nq=20):
        o = [P(bufs[k]) if k in out else None for k in range(4)]
        return engine.lib.zigp_score_rows(engine.ctx, lik, *[P(a) for a in r], 200, S.NOISE, P(x), P(w), nq, P(lv), L, *o)
    cases = [(dict(lv=lv17, L=17), 'n_levels'), (dict(r=rows[:4] + (None,), out=(1, 2)), 'y'), (dict(r=rows[:4] + (None,), out=(0, 1)), 'y'),
             (dict(r=rows[:4] + (None,), out=(1, 3)), 'y'), (dict(L=0), 'n_levels'), (dict(lv=None), 'levels'), (dict(out=(0, 2, 3)), 'quant'),
             (dict(lik=2), 'Bernoulli'), (dict(lik=3), 'lik'), (dict(nq=0), 'n_quad'), (dict(r=(None,) + rows[1:]), 'fm')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in engine.lib.zigp_last_error(engine.ctx).decode(), (kw, engine.lib.zigp_last_error(engine.ctx))
        assert all(np.all(b == SENT) for b in bufs), kw
        assert same(legal(), before)
    assert call() == 0 and np.array_equal(bufs[2], before['crps']) and bufs[3][0] == before['crps_sum']


# ---- 7. through predict ----------------------------------------------------------------------------------------------------------
def _dense_problem(mode):
    N = 300
    if mode == 'wide':
        X, Y, p = make_problem(N, 20, 9, seed=11, ell=1.2)
    else:
        X, Y, p = make_problem(N, 20, 3, seed=11, ell=0.4)
    if mode == 'white':
        p['whiten'] = True
    if mode == 'white_full':
        p = fr.make_lq(p, seed=3, negative=2)
    if mode == 'matern':
        p = dict(p, kern_f='matern52')
    if mode == 'constant':
        p = dict(p, mean_b=0.37)
    return X, Y, p


@pytest.mark.parametrize('mode', ['diag', 'white', 'white_full', 'matern', 'constant', 'wide'])
def test_predict_scores_is_score_rows_of_predict_on_host_and_device(engine, mode):
    import torch
    X, Y, p = _dense_problem(mode)
    levels = (0.05, 0.5, 0.95)
    rows = engine.predict(p, X, jitter=1e-6)
    ref = engine.score_rows('onoff', rows[3], rows[4], rows[5], rows[6], Y, p['noise'], n_quad=20, levels=levels)
    out = engine.predict_scores(p, X, Y, jitter=1e-6, n_quad=20, levels=levels)
    dev = engine.predict_scores_device(p, torch.as_tensor(X, device='cuda:0'), torch.as_tensor(Y, device='cuda:0'), jitter=1e-6, n_quad=20, levels=levels)
    for k in ('cdf', 'sf', 'quantiles', 'crps'):
        assert np.array_equal(out[k], ref[k]), (mode, k)
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), out[k]), (mode, k)
    assert out['crps_sum'] == ref['crps_sum'] == dev['crps_sum']
    assert np.array_equal(engine.predict(p, X, jitter=1e-6), rows)
    if mode == 'diag':
        qd = engine.predict_scores_device(p, torch.as_tensor(X, device='cuda:0'), None, n_quad=20, levels=levels)          # no Ynew: the quantiles alone
        assert qd['cdf'] is None and qd['crps'] is None and np.array_equal(qd['quantiles'].cpu().numpy(), out['quantiles'])
        with pytest.raises(ValueError):
            engine.predict_scores_device(p, torch.as_tensor(X), torch.as_tensor(Y, device='cuda:0'))
        from zigp.engine import _Packed
        pk, (x, w), tot = _Packed(p), R.rule(20), np.zeros(1)
        rc = engine.lib.zigp_predict_scores_device(engine.ctx, C.byref(pk.struct), C.c_void_p(X.ctypes.data), C.c_void_p(Y.ctypes.data), 10, 1e-6, 0.0,
                                                   x.ctypes.data, w.ctypes.data, x.size, None, 0, None, None, None, tot.ctypes.data)
        assert rc == -1 and b'device memory' in engine.lib.zigp_last_error(engine.ctx)


def test_kron_rows_and_the_gaussian_kron_head(engine):
    """rows of kron_predict and of a Gaussian kron_head_predict, fed to score_rows, against NumPy on the same rows (the bar of
    test_rule_sizes_against_numpy)"""
    X, Y, p = K.problem('d11')
    y = Y.reshape(-1)
    noise = float(np.squeeze(p['noise']))
    x, w = R.rule(20)
    bar = 5 * S.FLOOR + 16
    rows = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
    args = (rows[3], rows[4], rows[5], rows[6], y)
    r = engine.score_rows('onoff', *args, noise, rule=(x, w), levels=(0.05, 0.5, 0.95))
    F, SF = S.cdf_np(*args, noise, x, w)
    SFl, SFu = S.cdf_scales(*args, noise, x, w)
    assert np.all(np.abs(r['cdf'] - F) <= bar * EPS * SFl) and np.all(np.abs(r['sf'] - SF) <= bar * EPS * SFu)
    assert np.all(np.abs(r['crps'] - S.crps_np(*args, noise, x, w)) <= bar * EPS * S.crps_scale(*args, noise, x, w))
    for l, pl in enumerate((0.05, 0.5, 0.95)):
        t = r['quantiles'][l]
        G = S.cdf_np(*args[:4], t, noise, x, w)
        res = np.abs(G[0] - pl) if pl <= 0.5 else np.abs(G[1] - (1.0 - pl))
        assert np.all(res <= bar * (EPS * S.cdf_scales(*args[:4], t, noise, x, w)[0 if pl <= 0.5 else 1] + np.spacing(np.abs(t)) * S.pdf_np(*args[:4], t, noise, x, w)))
    h = engine.kron_head_predict(K.head_params(p), X, 'gaussian', jitter=K.JITTER, f_mu=0.0)
    g = engine.score_rows('gaussian', h[0], h[1], None, None, y, noise, levels=(0.05, 0.5, 0.95))
    ref, scale = S.head_np(h[0], h[1], y, noise, (0.05, 0.5, 0.95)), S.head_scales(h[0], h[1], y, noise)
    for k, key in enumerate(('cdf', 'sf', 'crps')):
        assert np.all(np.abs(g[key] - ref[k]) <= bar * EPS * scale[k]), key
    assert np.all(np.abs(g['quantiles'] - ref[3]) <= bar * EPS * (np.abs(h[0]) + np.sqrt(h[1] + noise) * np.abs(ref[3] - h[0]) / np.sqrt(h[1] + noise) + np.abs(ref[3])))


# ---- 8. model --------------------------------------------------------------------------------------------------------------------
def test_model_quantiles_round_trip_through_the_cdf_and_crps_is_the_engines(engine):
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    from onoffgpf.OnOffSVGP import JITTER
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(0)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=2.), onoffgpf.kernels.RBF(1, lengthscales=2., variance=5.), OnOffLikelihood(), Z, Z.copy())
    m.likelihood.variance = 0.01
    m.optimize(maxiter=5)
    N = X.shape[0]
    levels = (0.05, 0.5, 0.95)
    q = m.predict_quantiles(X, levels)
    assert q.shape == (N, 3) and np.all(np.diff(q, axis=1) >= 0)
    rows = m._engine.predict(m._values(), X, jitter=JITTER)
    noise = float(m.likelihood.variance.value.reshape(-1)[0])
    x, w = R.rule(64)
    bar = 5 * S.FLOOR + 16
    for l, p in enumerate(levels):          # F(quantile) = level, within the quantile bar
        t = np.ascontiguousarray(q[:, l])
        F, SF = m.predict_cdf(X, t)
        assert F.shape == SF.shape == (N, 1)
        res = np.abs(F[:, 0] - p) if p <= 0.5 else np.abs(SF[:, 0] - (1.0 - p))
        unit = EPS * S.cdf_scales(rows[3], rows[4], rows[5], rows[6], t, noise, x, w)[0 if p <= 0.5 else 1] \
            + np.spacing(np.abs(t)) * S.pdf_np(rows[3], rows[4], rows[5], rows[6], t, noise, x, w)
        assert np.all(res <= bar * unit), p
    c = m.predict_crps(X, Y)
    e = m._engine.predict_scores(m._values(), X, Y, jitter=JITTER, n_quad=64)
    assert c.shape == (N, 1) and np.array_equal(c[:, 0], e['crps']) and np.all(c > 0)
    assert np.array_equal(m.predict_cdf(X, Y)[0][:, 0], e['cdf'])
