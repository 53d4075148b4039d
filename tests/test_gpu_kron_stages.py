"""Stage-level parity of the Kronecker path's point-wise and per-point panel kernels (csrc/zigp_kron.hip): ONE launch of
k_kron_pointwise / k_kron_head_pointwise / k_kron_kbuild / k_kron_colsum / k_kron_da / k_kron_kgrad on caller-supplied operands
(DenseEngine.test_kron_pointwise / test_kron_panel_*, include/zigp_diag.h), against the host references of tests/stage_ref.py.

The point-wise outputs follow the rule of the dense point-wise stage, err_gpu <= 4 err_np + 16 eps S per point against a 50-digit evaluation;
evaluation points, the dq cotangents, the masked points and the device-hyperparameter variants are compared bit for bit; the panel kernels
are bit-equal to numpy on integer operands and within the bound of their restatement on random ones.  Every test prints STAGE-LOG lines
(profiles/kron_stage_parity.log keeps a run's)."""
import functools

import numpy as np
import pytest

import stage_ref as sr
from test_gpu_kron import make_kron_problem
from test_gpu_stages import GRID, _assert_exact_premise, _compare, _rule, sr_sentinel

pytestmark = pytest.mark.gpu

T = sr.KPW_THREADS
PT_KEYS = ('gm_f', 'gv_f', 'dq0_f', 'dq1_f', 'gm_g', 'gv_g', 'dq0_g', 'dq1_g')
LIKS = ('onoff', 'gaussian', 'bernoulli')
HEAD_FM = [-40, -8, -3, -1, -1e-3, 0, 1e-3, 1, 3, 8, 40]
HEAD_FV = [1e-10, 1e-3, 0.1, 1, 10, 1e3, 1e6]


def _run(engine, lik, mode, both=True, **kw):
    """One launch; with both, the launch that reads Knn, the noise and (heads) f_offset from the device hyperparameter block as well, which
    must return the same bits in every output buffer, untouched ones included (no step launches the heads' predict kernel on the block)."""
    out = engine.test_kron_pointwise(lik, mode, dev_hyp=False, **kw)
    if both and not (lik != 'onoff' and mode == 'predict'):
        dev = engine.test_kron_pointwise(lik, mode, dev_hyp=True, **kw)
        for k in out:
            assert np.array_equal(out[k], dev[k]), 'kron pointwise %s/%s: %s differs between the by-value launch and the device block' % (lik, mode, k)
        print('STAGE-LOG %-12s %-34s bit-equal to the by-value launch (%d buffers)' % ('kron-pw/hyp', '%s/%s device block' % (lik, mode), len(out)))
    return out


def _block_sums(vals, n_blocks, zero=0.0):
    """sums per block of T points of the first len(vals) points (object arrays: mpf sums)"""
    v = list(vals) + [zero] * (n_blocks * T - len(vals))
    if isinstance(zero, float):
        return np.asarray(v, dtype=np.float64).reshape(n_blocks, T).sum(1)
    return np.array([sum(v[b * T:(b + 1) * T], zero) for b in range(n_blocks)], dtype=object)


# =====================================================================================================================================
# (a) the head likelihoods over a grid
# =====================================================================================================================================
@pytest.mark.parametrize('lik,noise', [('bernoulli', 1.0), ('gaussian', 1e-4), ('gaussian', 1e-2), ('gaussian', 1.0)])
def test_head_arithmetic_over_the_grid(engine, lik, noise):
    """fm x fv x y (231 points per launch) against the 50-digit evaluation, err_gpu <= 4 err_np + 16 eps S per point and output, nothing
    excluded.  The planes make the evaluation point exact whatever the compiler contracts (q0 = q1 = 0, Knn = 1, st = target - 1,
    f_offset = 0); the doubles really evaluated are read back from predict rows 0 / 1 and both references are fed those.  ve and d noise
    leave the kernel only as sums over a block of 256 points, so every block holds ONE grid point 256 times: the block's sum is that
    point's value (times 256), and the rule applies per point."""
    ys = [0, 1, 0.5] if lik == 'bernoulli' else [0, 0.7, -3]
    g = np.array(np.meshgrid(HEAD_FM, HEAD_FV, ys, indexing='ij'), dtype=np.float64).reshape(3, -1)
    n = g.shape[1]
    assert n == 231
    rep = lambda a: np.repeat(a, T)
    part = np.stack([np.zeros(n * T), np.zeros(n * T), rep(g[0]), rep(g[1] - 1.0)])
    Y = rep(g[2])
    stage = 'kron-head/%s noise=%g' % (lik, noise)
    pr = _run(engine, lik, 'predict', part_f=part, N=n * T, noise=noise)['out']
    fm_all, fv_all = sr.kron_pw_inputs(part, 1.0, 0.0)
    _compare(stage, 'predict rows 0, 1 (evaluation point)', pr[:2], np.stack([fm_all, fv_all]), None, True, columns_only=True)
    fm, fv, y = pr[0, ::T].copy(), pr[1, ::T].copy(), g[2]
    truth, ref, S = sr.head_mp(lik, fm, fv, y, noise), sr.head_np(lik, fm, fv, y, noise), sr.head_scales(lik, fm, fv, y, noise)
    for row, k in ((2, 'pm'), (3, 'pv')):
        assert np.array_equal(pr[row], rep(pr[row, ::T])), 'the 256 copies of a point differ'
        _rule(stage, 'predict ' + k, pr[row, ::T], ref[k], truth[k], S[k])
    gr = _run(engine, lik, 'grad', part_f=part, Y=Y, noise=noise)
    for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv')):
        assert np.array_equal(gr[k], rep(gr[k][::T])), 'the 256 copies of a point differ'
        _rule(stage, name, gr[k][::T], ref[name], truth[name], S[name])
    va = _run(engine, lik, 'value', part_f=part, Y=Y, noise=noise)
    for mode, acc in (('value', va['acc']), ('grad', gr['acc'])):
        for col, key in ((0, 've'), (1, 'dnoise'), (2, 'dfv'), (4, 'dfm')):
            _rule(stage, '%s acc[%d] = 256 x %s' % (mode, col, key), acc[:, col], ref[key], truth[key], S[key], float(T))
        assert not acc[:, 3].any(), 'acc[:, 3] of a head launch is not exactly 0'
    assert np.array_equal(va['acc'], gr['acc'])


# =====================================================================================================================================
# (b) pointwise_eval as instantiated inside k_kron_pointwise
# =====================================================================================================================================
def test_onoff_wrapper_over_the_dense_grid(engine):
    """The dense test's GRID (gm x gv x fm x fv x y, 4620 points) at noise 1e-2 through k_kron_pointwise: predict rows 0, 1, 2, 7, 8, the four
    cotangents and the block sums of ve and d noise follow the rule.  The evaluation points are the dense test's doubles (1 - 0 + (target
    - 1)), so the 50-digit truth is shared with it through stage_ref's cache."""
    noise = 1e-2
    g = np.array(np.meshgrid(GRID['gm'], GRID['gv'], GRID['fm'], GRID['fv'], GRID['y'], indexing='ij'), dtype=np.float64).reshape(5, -1)
    n = g.shape[1]
    assert n == 4620
    Nc = sr.round_up(n, T)
    nb = Nc // T
    pad = lambda a: np.concatenate([a, np.zeros(Nc - n)])
    z = np.zeros(Nc)
    pf, pg = np.stack([z, z, pad(g[2]), pad(g[3] - 1.0)]), np.stack([z, z, pad(g[0]), pad(g[1] - 1.0)])
    Y = g[4].copy()
    stage = 'kron-pw/grid noise=%g' % noise
    pr = _run(engine, 'onoff', 'predict', part_f=pf, part_g=pg, N=n, noise=noise)['out']
    (fm, fv), (gm, gv) = sr.kron_pw_inputs(pf, 1.0, 0.0), sr.kron_pw_inputs(pg, 1.0, 0.0)
    for row, a in ((3, fm), (4, fv), (5, gm), (6, gv)):
        _compare(stage, 'predict row %d (evaluation point)' % row, pr[row][None, :], a[None, :n], None, True, columns_only=True)
    fm, fv, gm, gv = pr[3].copy(), pr[4].copy(), pr[5].copy(), pr[6].copy()
    truth = sr.pointwise_mp_cached(fm, fv, gm, gv, Y, noise)
    ref, S = sr.pointwise_np(fm, fv, gm, gv, Y, noise), sr.pointwise_scales(fm, fv, gm, gv, Y, noise)
    assert all(t > 0 for t in truth['e2']) and all(t > 0 for t in truth['ev']), 'a grid point reaches a clipping branch (the clipped value is exactly 0)'
    for row, k in ((0, 'gfmean'), (1, 'gfvar'), (2, 'gfmeanu'), (7, 'e1'), (8, 'ev')):
        _rule(stage, 'predict ' + k, pr[row], ref[k], truth[k], S[k])
    gr = _run(engine, 'onoff', 'grad', part_f=pf, part_g=pg, Y=Y, noise=noise)
    for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv'), ('gm_g', 'dgm'), ('gv_g', 'dgv')):
        _rule(stage, name, gr[k][:n], ref[name], truth[name], S[name])
    va = _run(engine, 'onoff', 'value', part_f=pf, part_g=pg, Y=Y, noise=noise)
    zero = 0 * truth['ve'][0]
    for mode, acc in (('value', va['acc']), ('grad', gr['acc'])):
        for col, key in ((0, 've'), (1, 'dnoise')):
            _rule(stage, '%s acc[%d] = summed %s' % (mode, col, key), acc[:, col], _block_sums(ref[key], nb), _block_sums(truth[key], nb, zero),
                  _block_sums(S[key], nb))
    assert np.array_equal(va['acc'][:, :2], gr['acc'][:, :2])


# =====================================================================================================================================
# (c) evaluation point, offsets, cancellation; the dq cotangents
# =====================================================================================================================================
def _labels(rs, lik, n):
    if lik == 'bernoulli':
        return (rs.rand(n) < 0.5) * 1.0
    return np.where(rs.rand(n) < 0.4, 0.0, rs.randn(n))


@pytest.mark.parametrize('lik', LIKS)
def test_evaluation_point_offsets_and_dq_are_exact(engine, lik):
    """Dyadic operands (stage_ref.kron_dyadic_case): Knn - q0 q1 + st and mean + offset are exact in every association, with or without
    fma, also where terms of size 32 cancel to 2^-20, so the predict rows that carry the evaluation point are bit-equal to numpy; in
    gradient mode dq0 = -(gv) q1 and dq1 = -(gv) q0 bit for bit, formed from the returned gv.  g_offset = -1, f_offset = 0.25, scale = 2.5."""
    c = sr.kron_dyadic_case()
    pf, pg = c['part_f'], c['part_g']
    Nc = pf.shape[1]
    N = Nc - 3
    two = lik == 'onoff'
    kw = dict(part_f=pf, part_g=pg if two else None, var_f=c['var_f'], var_g=c['var_g'], noise=c['noise'], g_offset=c['g_offset'],
              f_offset=c['f_offset'], scale=c['scale'])
    stage = 'kron-pw/dyadic %s' % lik
    knn_f, knn_g = c['var_f'][0] * c['var_f'][1], c['var_g'][0] * c['var_g'][1]
    fm, fv = sr.kron_pw_inputs(pf, knn_f, c['f_offset'])
    gm, gv = sr.kron_pw_inputs(pg, knn_g, c['g_offset'])
    assert fv[0] == 2.0 ** -20 and fv[1] == 2.0 ** -20 and gv[0] == 2.0 ** -20
    pr = _run(engine, lik, 'predict', N=N, **kw)['out']
    want = np.stack([fm, fv, gm, gv])[:, :N] if two else np.stack([fm, fv])[:, :N]
    _compare(stage, 'evaluation point rows', pr[3:7] if two else pr[:2], want, None, True, columns_only=True)
    Y = _labels(np.random.RandomState(5), lik, N)
    gr = _run(engine, lik, 'grad', Y=Y, **kw)
    for tag, part in (('f', pf), ('g', pg))[:2 if two else 1]:
        g_ = gr['gv_' + tag]
        assert np.all(np.isfinite(g_)) and g_[:N].any()
        _compare(stage, 'dq0_%s = -(gv) q1' % tag, gr['dq0_' + tag][None, :], (-g_ * part[1])[None, :], None, True, columns_only=True)
        _compare(stage, 'dq1_%s = -(gv) q0' % tag, gr['dq1_' + tag][None, :], (-g_ * part[0])[None, :], None, True, columns_only=True)
    print('STAGE-LOG %-12s %-34s bit-equal (evaluation point rows, dq0, dq1)' % ('kron-pw', 'dyadic %s' % lik))


# =====================================================================================================================================
# (d) masking and accumulators
# =====================================================================================================================================
MASK_NC, MASK_NMAX = 1024, 1000


@functools.lru_cache(maxsize=None)
def _mask_case(lik):
    """Operands of the masking tests and their references over the MASK_NMAX points any of the cases validates, computed once.  Every
    column of part, the padding included, holds random finite non-zero values of the size a step leaves there (the panel path's padding
    columns are the kernel at x = 0: plausible means and variances, not zeros)."""
    rs = np.random.RandomState({'onoff': 11, 'gaussian': 12, 'bernoulli': 13}[lik])
    Nc = MASK_NC
    var_f, var_g, noise, g_offset, f_offset, scale = (1.5, 2.0), (0.75, 1.25), 0.05, -1.0, 0.25, 2.5

    def planes(knn):
        q0, q1 = 0.05 + rs.rand(Nc), 0.05 + 0.9 * knn * rs.rand(Nc)
        return np.stack([q0, q1, rs.randn(Nc), 0.05 + rs.rand(Nc)])

    pf, pg = planes(3.0), planes(0.9375)
    assert np.all(pf != 0) and np.all(pg != 0) and np.all(np.isfinite(pf)) and np.all(np.isfinite(pg))
    Y = _labels(rs, lik, MASK_NMAX)
    n = MASK_NMAX
    fm, fv = (a[:n] for a in sr.kron_pw_inputs(pf, var_f[0] * var_f[1], f_offset))
    gm, gv = (a[:n] for a in sr.kron_pw_inputs(pg, var_g[0] * var_g[1], g_offset))
    kw = dict(part_f=pf, part_g=pg if lik == 'onoff' else None, var_f=var_f, var_g=var_g, noise=noise, g_offset=g_offset, f_offset=f_offset, scale=scale)
    return dict(kw=kw, Y=Y, pts=(fm, fv, gm, gv), refs={})


def _mask_refs(case, lik, pts):
    """references at the evaluation points the GPU reported (shared by the cases of one likelihood as long as those are the same doubles)"""
    key = tuple(a.tobytes() for a in pts)
    if key not in case['refs']:
        fm, fv, gm, gv = pts
        Y, noise = case['Y'][:len(fm)], case['kw']['noise']
        if lik == 'onoff':
            case['refs'][key] = (sr.pointwise_mp(fm, fv, gm, gv, Y, noise), sr.pointwise_np(fm, fv, gm, gv, Y, noise), sr.pointwise_scales(fm, fv, gm, gv, Y, noise))
        else:
            case['refs'][key] = (sr.head_mp(lik, fm, fv, Y, noise), sr.head_np(lik, fm, fv, Y, noise), sr.head_scales(lik, fm, fv, Y, noise))
    return case['refs'][key]


@pytest.mark.parametrize('N', [1, 255, 256, 257, 1000])
@pytest.mark.parametrize('lik', LIKS)
def test_masked_points_and_accumulators(engine, lik, N):
    """N valid points of Nc = 1024 (one point; a block boundary and either side of it; inside the last block): gm, gv, dq0, dq1 are exactly 0
    at n >= N -- the panel path's reductions over ALL Nc columns (E K^T, K0 diag(gm) K1^T) rely on it, their K panels are not zero there --,
    every accumulator of a fully masked block is exactly 0, the accumulators of the live blocks follow the rule against block-summed
    truth and S, predict writes nothing at or beyond column N, and the value-only launch writes none of the per-point buffers."""
    case = _mask_case(lik)
    kw, Nc, two = case['kw'], MASK_NC, lik == 'onoff'
    sent = sr_sentinel()
    nb = Nc // T
    stage = 'kron-pw/mask %s N=%d' % (lik, N)
    Y = case['Y'][:N]
    pr = _run(engine, lik, 'predict', N=N, ld_out=Nc, **kw)['out']
    assert np.all(pr[:, N:] == sent), '%s: predict wrote at or beyond column N' % stage
    assert not np.any(pr[:, :N] == sent), '%s: predict left a valid column unwritten' % stage
    rows = (3, 4, 5, 6) if two else (0, 1)
    # the evaluation points the kernel used (its own doubles: the compiler may contract Knn - q0 q1), a few ulp from the numpy statement
    pts = tuple(pr[r, :MASK_NMAX].copy() for r in rows)
    for a, b in zip(pts, case['pts']):
        assert np.all(np.abs(a[:N] - b[:N]) <= 8 * sr.EPS * (np.abs(b[:N]) + 4.0)), '%s: the evaluation point is not Knn - q0 q1 + st' % stage
    # references are evaluated once, at the points of the N = 1000 case; a smaller N must report the same doubles for its points
    full = tuple(_run(engine, lik, 'predict', both=False, N=MASK_NMAX, **kw)['out'][r].copy() for r in rows)
    for a, b in zip(pts, full):
        assert np.array_equal(a[:N], b[:N])
    if not two:
        full = full + (np.zeros(MASK_NMAX), np.zeros(MASK_NMAX))
    truth, ref, S = _mask_refs(case, lik, full)
    names = dict(gm_f='dfm', gv_f='dfv', gm_g='dgm', gv_g='dgv')
    va = _run(engine, lik, 'value', Y=Y, **kw)
    for k in PT_KEYS:
        assert np.all(va[k] == sent), '%s: the value-only launch wrote %s' % (stage, k)
    gr = _run(engine, lik, 'grad', Y=Y, **kw)
    for k in PT_KEYS:
        if not two and k.endswith('_g'):
            assert np.all(gr[k] == sent), '%s: a head launch wrote %s' % (stage, k)
            continue
        assert np.all(np.isfinite(gr[k])), '%s: %s is not finite' % (stage, k)
        assert not gr[k][N:].any(), '%s: %s is not exactly 0 at a masked point' % (stage, k)
        if k in names:
            _rule(stage, names[k], gr[k][:N], ref[names[k]][:N], truth[names[k]][:N], S[names[k]][:N], kw['scale'])
    cols = [(0, 've'), (1, 'dnoise'), (2, 'dfv'), (4, 'dfm')] + ([(3, 'dgv')] if two else [])
    zero = 0 * truth['ve'][0]
    live = np.arange(nb) * T < N
    for mode, acc in (('value', va['acc']), ('grad', gr['acc'])):
        assert np.all(np.isfinite(acc))
        assert not acc[~live].any(), '%s: a fully masked block has a non-zero accumulator' % stage
        if not two:
            assert not acc[:, 3].any(), '%s: acc[:, 3] of a head launch is not exactly 0' % stage
        for col, key in cols:
            _rule(stage, '%s acc[%d] = block sums of %s' % (mode, col, key), acc[live, col], _block_sums(ref[key][:N], nb)[live],
                  _block_sums(truth[key][:N], nb, zero)[live], _block_sums(S[key][:N], nb)[live], kw['scale'])
    assert np.array_equal(va['acc'], gr['acc'])


# =====================================================================================================================================
# (f) tie to the real calls
# =====================================================================================================================================
@pytest.mark.parametrize('N', [300, 257])
@pytest.mark.parametrize('panels', [False, True], ids=['fused', 'panels'])
@pytest.mark.parametrize('lik', LIKS)
def test_real_calls_follow_the_rule_at_their_own_points(engine, lik, panels, N):
    """The real predict call's moment rows follow the rule at the evaluation points the same call reports (rows 3 - 6; heads 0 - 1), and the
    data term of a value-only ELBO with scale 3 is 3 sum ve at those points within the rule's bound summed over the rows (both calls run
    the same forward launch), on the fused kernels and on the panel path."""
    X, Y, p = make_kron_problem(N, 6, 5, seed=N)
    Y = Y.reshape(-1)
    jitter, scale, noise = 1e-5, 3.0, p['noise']
    stage = 'kron-real/%s %s N=%d' % (lik, 'panels' if panels else 'fused', N)
    engine.set_kron_panels(panels)
    try:
        if lik == 'onoff':
            out = engine.kron_predict(p, X, jitter=jitter, g_offset=-1.0, f_mu=0.25)
            ed, _, _ = engine.kron_elbo(p, X, Y, jitter=jitter, scale=scale, g_offset=-1.0, include_kl=False, need_grad=False, f_mu=0.25)
        else:
            ph = {k: p[k] for k in ('Zf', 'ell_f', 'var_f', 'u_fm', 'u_fs_sqrt', 'noise')}
            if lik == 'bernoulli':
                Y = (Y > 0) * 1.0
            out = engine.kron_head_predict(ph, X, lik, jitter=jitter, f_mu=0.25)
            ed, _, _ = engine.kron_head_elbo(ph, X, Y, lik, jitter=jitter, scale=scale, f_mu=0.25, include_kl=False, need_grad=False)
    finally:
        engine.set_kron_panels(False)
    if lik == 'onoff':
        fm, fv, gm, gv = (out[r].copy() for r in (3, 4, 5, 6))
        truth, ref, S = sr.pointwise_mp(fm, fv, gm, gv, Y, noise), sr.pointwise_np(fm, fv, gm, gv, Y, noise), sr.pointwise_scales(fm, fv, gm, gv, Y, noise)
        rows = ((0, 'gfmean'), (1, 'gfvar'), (2, 'gfmeanu'), (7, 'e1'), (8, 'ev'))
    else:
        fm, fv = out[0].copy(), out[1].copy()
        truth, ref, S = sr.head_mp(lik, fm, fv, Y, noise), sr.head_np(lik, fm, fv, Y, noise), sr.head_scales(lik, fm, fv, Y, noise)
        rows = ((2, 'pm'), (3, 'pv'))
    for row, k in rows:
        _rule(stage, 'predict ' + k, out[row], ref[k], truth[k], S[k])
    t_sum = sum(truth['ve'], 0 * truth['ve'][0])
    bound = scale * float(np.sum(4 * sr.mp_err(ref['ve'], truth['ve']) + 16 * sr.EPS * S['ve']))
    err = float(abs(ed - scale * t_sum))
    print('STAGE-LOG %-12s %-34s |data term - 3 sum ve| / bound = %.4g' % ('kron-real', stage[10:], err / bound))
    assert err <= bound, '%s: data term %.17g, 3 sum ve %.17g, error %.3g > %.3g' % (stage, ed, float(scale * t_sum), err, bound)


# =====================================================================================================================================
# (g) the panel path's per-point kernels
# =====================================================================================================================================
PANEL_M, PANEL_D, PANEL_N, PANEL_NC = (5, 16, 33), (1, 3, 8), (1, 257, 1000), 1024


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('M0,M1', [(5, 16), (16, 33), (33, 5)])
def test_panel_colsum(engine, M0, M1, kind):
    o = sr.kron_panel_operands(kind, M0, 1, 1, PANEL_NC, seed=M0, M1=M1)
    a = (o['K'], o['A'], o['K1'], o['A1'], o['B'], o['Asq'], o['C'])
    got = engine.test_kron_panel_colsum(*a)
    stage = 'kron-colsum/%s %dx%d' % (kind, M0, M1)
    if kind == 'int':
        ref, bnd = sr.kron_colsum(*a)
        _assert_exact_premise(bnd / sr.gamma(np.array([M0, M1, M0, M0])[:, None] + 2) + 1)
        _compare(stage, 'part', got, ref, None, True, columns_only=True)
    else:
        ref, bnd = sr.kron_colsum(*a, dtype=np.longdouble)
        _compare(stage, 'part', got, np.asarray(ref, dtype=np.float64), bnd * (1 + 2.0 ** -11), False, columns_only=True)


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('M', PANEL_M)
def test_panel_da(engine, M, kind):
    o = sr.kron_panel_operands(kind, M, 1, 1, PANEL_NC, seed=10 + M)
    a = (o['A'], o['C'], o['K'], o['gv'], o['dq'])
    dA, E = engine.test_kron_panel_da(*a)
    stage = 'kron-da/%s M=%d' % (kind, M)
    (rA, bA), (rE, bE) = sr.kron_da(*a, dtype=np.float64 if kind == 'int' else np.longdouble)
    for name, got, ref, bnd in (('dA', dA, rA, bA), ('E', E, rE, bE)):
        if kind == 'int':
            _compare(stage, name, got, ref, None, True)
        else:
            _compare(stage, name, got, np.asarray(ref, dtype=np.float64), bnd * (1 + 2.0 ** -11), False)


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('D', PANEL_D)
@pytest.mark.parametrize('M', PANEL_M)
def test_panel_kgrad(engine, M, D, kind):
    """Every N of the issue per (M, D): accumulation onto non-zero initial krow, col0 = 2 and ldx = D + 3, and the columns n >= N of every
    operand hold the stage sentinel's double: a read of one of them wrecks the sums."""
    sent = sr_sentinel()
    for N in PANEL_N:
        o = sr.kron_panel_operands(kind, M, D, N, PANEL_NC, seed=100 * M + 10 * D + N % 7)
        ops = {k: o[k].copy() for k in ('B', 'A', 'PdA', 'K', 'gm', 'dq')}
        for a in ops.values():
            a[..., N:] = sent
        args = (ops['B'], ops['A'], ops['PdA'], ops['K'], ops['gm'], ops['dq'], o['X'], o['col0'], o['Z'])
        got = engine.test_kron_panel_kgrad(*args, krow=o['krow0'])
        stage = 'kron-kgrad/%s M=%d D=%d N=%d' % (kind, M, D, N)
        assert np.array_equal(got[:, 1 + 2 * D], o['krow0'][:, 1 + 2 * D]), '%s: the last column of krow was touched' % stage
        if kind == 'int':
            ref, bnd = sr.kron_kgrad(*args, krow0=o['krow0'])
            _assert_exact_premise(bnd / sr.gamma(N + 9) + 1)
            _compare(stage, 'krow', got, ref, None, True)
        else:
            ref, bnd = sr.kron_kgrad(*args, krow0=o['krow0'], dtype=np.longdouble)
            _compare(stage, 'krow', got, np.asarray(ref, dtype=np.float64), bnd * (1 + 2.0 ** -11), False)
    if kind == 'int':
        print('STAGE-LOG %-12s %-34s bit-equal for N in %s' % ('kron-kgrad', 'int M=%d D=%d' % (M, D), list(PANEL_N)))


@pytest.mark.parametrize('D', PANEL_D)
@pytest.mark.parametrize('M', PANEL_M)
def test_panel_kbuild(engine, M, D):
    """Rows m >= M are exactly 0; the padding columns n >= N hold the kernel at x = 0 (bit-equal to the launch's value for a row of zeros: NOT
    zero, which is why the point-wise kernel has to leave exact zeros at masked points); valid entries are held to the bar of
    test_kuf_panel_kernel_golden_kernse_np_and_ulp against an 80-bit evaluation: (4 + 8 y) eps K + 5e-324, y = -log(K / var)."""
    eps = np.finfo(np.float64).eps
    L = np.longdouble
    col0, Nc = 2, PANEL_NC
    for N in PANEL_N:
        rng = np.random.RandomState(1000 * M + 10 * D + N % 5)
        X = rng.randn(N, col0 + D + 1) * rng.choice([0.3, 3.0, 30.0], size=(N, 1))
        Z, ell, var = rng.randn(M, D), 0.5 + rng.rand(D), 1.7
        K = engine.test_kron_panel_kbuild(X, col0, Z, ell, var, Nc)
        stage = 'kron-kbuild M=%d D=%d N=%d' % (M, D, N)
        assert K.shape == (128, Nc) and np.all(np.isfinite(K))
        assert not K[M:].any(), '%s: a row m >= M is not exactly 0' % stage
        ref, y = sr.kron_kbuild(X, col0, Z, ell, var, Nc, dtype=L)
        tol = (4.0 + 8.0 * y) * eps * ref + L(5e-324)
        err = np.abs(K[:M].astype(L) - ref)
        ref64, _ = sr.kron_kbuild(X, col0, Z, ell, var, Nc)
        r, r64 = float(np.max(err / tol)), float(np.max(np.abs(ref64.astype(L) - ref) / tol))
        print('STAGE-LOG %-12s %-34s max error / tolerance = %.4g (numpy formula: %.4g)' % ('kron-kbuild', stage[12:], r, r64))
        assert r <= 1.0, '%s: error / ((4 + 8 y) eps K) = %.3g' % (stage, r)
        at0 = engine.test_kron_panel_kbuild(np.zeros((1, col0 + D + 1)), col0, Z, ell, var, 256)[:, 0]
        assert at0[:M].all(), 'the kernel at x = 0 underflowed: the padding would not be told from zero'
        assert np.array_equal(K[:, N:], np.repeat(at0[:, None], Nc - N, 1)), '%s: a padding column is not the kernel at x = 0' % stage


def test_kron_stage_entry_points_validate_and_leave_the_context_usable(engine):
    from zigp import _lib
    lib = engine.lib
    assert lib.zigp_test_kron_pointwise(None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_pointwise(engine.ctx, None) == _lib.ZIGP_EARG
    part = np.ones((4, 256))
    with pytest.raises(ValueError):
        engine.test_kron_pointwise('onoff', 'predict', part, None, N=10)                  # OnOff without part_g
    with pytest.raises(ValueError):
        engine.test_kron_pointwise('gaussian', 'predict', part, N=10, dev_hyp=True)       # no such launch
    with pytest.raises(ValueError):
        engine.test_kron_pointwise('gaussian', 'predict', np.ones((4, 100)), N=10)        # Nc not a multiple of 256
    with pytest.raises(ValueError):
        engine.test_kron_pointwise('gaussian', 'predict', part, N=257)                    # N > Nc
    with pytest.raises(ValueError):
        engine.test_kron_pointwise('gaussian', 'value', part, N=10)                       # the ELBO modes need Y
    with pytest.raises(ValueError):
        engine.test_kron_panel_kbuild(np.zeros((4, 2)), 1, np.zeros((3, 2)), 1.0, 1.0, 256)   # col0 + D > ldx
    assert lib.zigp_test_kron_kbuild(None, 1, 256, 1, 0, 1, 1, None, None, None, 1.0, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_colsum(engine.ctx, 0, 1, 256, *([None] * 8)) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_da(engine.ctx, 1, 100, *([None] * 7)) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_kgrad(engine.ctx, 1, 9, 1, 256, 9, 0, *([None] * 9)) == _lib.ZIGP_EARG
    X, Y, p = make_kron_problem(200, 6, 5, seed=1)
    a = engine.kron_elbo(p, X, Y, jitter=1e-5, need_grad=False)
    engine.test_kron_pointwise('bernoulli', 'grad', part, Y=np.ones(10))
    engine.test_kron_panel_colsum(*([np.ones((2, 256))] * 7))
    b = engine.kron_elbo(p, X, Y, jitter=1e-5, need_grad=False)
    assert a[:2] == b[:2]
