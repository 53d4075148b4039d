"""Stage-level parity of the dense heads' point-wise kernel, k_pointwise_head (csrc/zigp_kernels.h): ONE launch on caller-supplied
partial-row planes of f (zigp_test_pointwise_head, include/zigp_diag.h; DenseEngine.test_pointwise(head=...)).

(a) The head arithmetic over a grid, against a 50-digit evaluation: err_gpu <= 4 err_np + 16 eps S per point and output, with the weights
    S and the references of the Kronecker heads' test (tests/stage_ref.py head_np / head_mp / head_scales; tests/test_gpu_kron_stages.py):
    fm x fv x y x noise with |z| up to 40, fv from 1e-12 to 1e6, the labels 1.0, 0.0 and 2.0 (which counts as off).
(b) On dyadic operands, bit for bit against the float64 restatement: the plane sums in the kernel's order (plane-row counts 4, 8 and 12:
    a wave adds one, two and three rows), the masked points for N = 1, 63, 64, 65 and 1000 valid points of 1024, the accumulators after
    two launches, and the zeros written for the placeholder latent -- in the value-only, the gradient and the predict form.
Every comparison prints a STAGE-LOG line (profiles/dense_head_parity.log keeps a run's)."""
import ctypes as C

import numpy as np
import pytest

import stage_ref as sr
import dense_head_ref as hr
from test_gpu_stages import _rule

pytestmark = pytest.mark.gpu

T = 64          # points per block of the kernel (PW_PTS)
HEAD_FM = [-40, -8, -3, -1, -1e-3, 0, 1e-3, 1, 3, 8, 40]
HEAD_FV = [1e-12, 1e-10, 1e-3, 0.1, 1, 10, 1e3, 1e6]
LOG2PI_HALF = -0.5 * 1.8378770664093454836


@pytest.mark.parametrize('lik,noise', [('bernoulli', 1.0), ('gaussian', 1e-4), ('gaussian', 1e-2), ('gaussian', 1.0)])
def test_head_arithmetic_over_the_grid(engine, lik, noise):
    """264 grid points per launch.  The planes make the evaluation point one addition (plane 0 = fm, plane 1 = 0, plane 2 = fv - 1,
    var_f = 1); the doubles really evaluated are read back from predict rows 0 / 1 -- bit-equal to the numpy replica in both variance
    forms -- and both references are fed those.  ve and d noise leave the kernel only as sums over a block of 64 points, so every block
    holds ONE grid point 64 times: the block's sum is 64 x that point's value and the rule applies per point."""
    ys = [1.0, 0.0, 2.0] if lik == 'bernoulli' else [0, 0.7, -3]
    g = np.array(np.meshgrid(HEAD_FM, HEAD_FV, ys, indexing='ij'), dtype=np.float64).reshape(3, -1)
    n = g.shape[1]
    assert n == 264
    Nv = n * T
    Nc = sr.round_up(Nv, 1024)
    rep = lambda a: np.concatenate([np.repeat(a, T), np.zeros(Nc - Nv)])      # noqa: E731
    part = np.zeros((3, 1, Nc))
    part[0, 0], part[2, 0] = rep(g[0]), rep(g[1] - 1.0)
    Y, X = np.repeat(g[2], T), np.zeros((Nv, 1))
    stage = 'dense-head/%s noise=%g' % (lik, noise)
    run = lambda mode, **kw: engine.test_pointwise(mode, part, None, 1, 1, X, None if mode == 'predict' else Y, 0, Nv, 1.0, 0.0, noise,      # noqa: E731
                                                   head=lik, **kw)
    pr = run('predict')['out9']
    fm_all, fv_all = sr.pw_plane_sum(part[0], 1), 1.0 - sr.pw_plane_sum(part[1], 1) + sr.pw_plane_sum(part[2], 1)
    assert np.array_equal(fv_all, 1.0 + sr.pw_plane_sum(part[2], 1))
    assert np.array_equal(pr[0], fm_all[:Nv]) and np.array_equal(pr[1], fv_all[:Nv]), '%s: the evaluation point is not the plane sum' % stage
    assert np.array_equal(run('predict', whiten=True)['out9'], pr), '%s: the two variance forms of predict differ' % stage
    print('STAGE-LOG %-12s %-34s bit-equal (evaluation point rows, both variance forms)' % (stage, 'predict rows 0, 1'))
    fm, fv, y = pr[0, ::T].copy(), pr[1, ::T].copy(), g[2]
    truth, ref, S = sr.head_mp(lik, fm, fv, y, noise), sr.head_np(lik, fm, fv, y, noise), sr.head_scales(lik, fm, fv, y, noise)
    for row, k in ((2, 'pm'), (3, 'pv')):
        assert np.array_equal(pr[row], np.repeat(pr[row, ::T], T)), 'the 64 copies of a point differ'
        _rule(stage, 'predict ' + k, pr[row, ::T], ref[k], truth[k], S[k])
    gr = run('grad')
    for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv')):
        assert np.array_equal(gr[k][:Nv], np.repeat(gr[k][:Nv:T], T)), 'the 64 copies of a point differ'
        assert not gr[k][Nv:].any()
        _rule(stage, name, gr[k][:Nv:T], ref[name], truth[name], S[name])
    assert not gr['gm_g'].any() and not gr['gv_g'].any(), '%s: the placeholder cotangents are not exactly 0' % stage
    va = run('value')
    for mode, acc in (('value', va['acc']), ('grad', gr['acc'])):
        for col, key in ((0, 've'), (1, 'dnoise'), (2, 'dfv')):
            _rule(stage, '%s acc[%d] = 64 x %s' % (mode, col, key), acc[:n, col], ref[key], truth[key], S[key], float(T))
        assert not acc[n:].any() and not acc[:, 3:].any(), '%s: a masked block or an unused accumulator is not exactly 0' % stage
    assert np.array_equal(va['acc'], gr['acc'])        # the same doubles in (var - 0 + p2 and var + p2), the same sums out


def _dyadic_case(rows, N, seed):
    """planes [3][rows][1024] of small dyadic numbers (every sum below is exact in any order), rows (X, Y) around the chunk at n0 = 128"""
    rs = np.random.RandomState(seed)
    Nc, n0 = 1024, 128
    part = np.stack([rs.randint(-8, 9, (rows, Nc)) / 8.0, rs.randint(0, 3, (rows, Nc)) / 32.0, rs.randint(0, 9, (rows, Nc)) / 8.0])
    D = {4: 2, 8: 1, 12: 3}[rows]
    mean = {4: None, 8: (np.zeros(1), 0.25), 12: (rs.randint(-4, 5, 3) / 8.0, -0.5)}[rows]
    Nrows = n0 + N
    X = rs.randint(-8, 9, (Nrows, D)) / 8.0
    return part, X, mean, n0, Nc


def _restate(part, np1, np2, gradvar, var_f, mean, X, n0, N):
    """(fm, fv, xs) as the kernel forms them; exact on the dyadic operands (the mean function's fma chain included)"""
    Nc = part.shape[2]
    fm, s2 = sr.pw_plane_sum(part[0], np1), sr.pw_plane_sum(part[2], np2)
    fv = var_f + s2 if gradvar else var_f - sr.pw_plane_sum(part[1], np1) + s2
    xs = np.zeros((Nc, X.shape[1]))
    xs[:N] = X[n0:n0 + N]
    if mean is not None:
        fm = fm + (mean[1] + xs @ np.asarray(mean[0], dtype=np.float64).reshape(-1))
    return fm, fv, xs


@pytest.mark.parametrize('N', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('rows', [4, 8, 12], ids=lambda r: 'Mp%d' % (32 * r))
@pytest.mark.parametrize('lik', hr.LIKS)
def test_plane_sums_masking_and_accumulators_bit_for_bit(engine, lik, rows, N):
    """Dyadic operands, scale 2.5, var_f 2, n0 = 128; plane 2 is summed over one row fewer than planes 0 and 1 (the unused row holds a
    sentinel).  Mean function: off (4 rows), Constant (8), Linear at D = 3 (12).
    Gaussian at noise 1 (log 1 = 0, 1 / noise = 1: every per-point value is one rounding of an exact number): gm_f, gv_f and all four
    accumulator slots -- the block sums through the kernel's xor-shuffle tree -- equal the float64 restatement bit for bit, after one launch
    and after two onto given initial values; at noise 1 / 2 the same without slot 0 (log(1 / 2) is a library value).
    Bernoulli: the evaluation point, the masks, the zeros, and two launches = (init + s) + s with the s of one launch."""
    part, X, mean, n0, Nc = _dyadic_case(rows, N, 100 * rows + N)
    sent = float(np.frombuffer(bytes([0x7f]) * 8, dtype=np.float64)[0])
    np1, np2 = rows, rows - 1
    part[2, np2:] = sent
    var_f, scale = 2.0, 2.5
    rs = np.random.RandomState(N)
    Nrows = n0 + N
    Y = (rs.rand(Nrows) < 0.5) * 1.0 if lik == 'bernoulli' else rs.randint(-4, 5, Nrows) / 4.0
    valid = np.arange(Nc) < N
    y = np.zeros(Nc)
    y[:N] = Y[n0:]
    stage = 'dense-head/dyadic %s rows=%d N=%d' % (lik, rows, N)
    nblk = Nc // T
    D = X.shape[1]
    used = np.zeros((nblk, 13), dtype=bool)
    used[:, :3] = True
    if mean is not None:
        used[:, 4:5 + D] = True
    for noise in ((1.0, 0.5) if lik == 'gaussian' else (1.0,)):
        for mode in ('predict', 'value', 'grad'):
            gradvar = mode == 'grad'
            p = part.copy()
            if gradvar:
                p[1] = sent                                  # a gradient step does not read plane 1
            fm, fv, xs = _restate(p, np1, np2, gradvar, var_f, mean, X, n0, N)
            kw = dict(scale=scale, mean=mean, head=lik)
            out = engine.test_pointwise(mode, p, None, np1, np2, X, None if mode == 'predict' else Y, n0, Nrows, var_f, 0.0, noise, **kw)
            if mode == 'predict':
                o = out['out9']
                assert o.shape == (4, Nrows) and not o[:, :n0].any(), '%s: predict wrote in front of n0' % stage
                assert np.array_equal(o[0, n0:], fm[:N]) and np.array_equal(o[1, n0:], fv[:N]), '%s: plane sums' % stage
                if lik == 'gaussian':
                    assert np.array_equal(o[2, n0:], fm[:N]) and np.array_equal(o[3, n0:], fv[:N] + noise)
                else:
                    assert np.all((o[2, n0:] >= 1e-3) & (o[2, n0:] <= 1 - 1e-3)) and np.array_equal(o[3, n0:], o[2, n0:] * (1.0 - o[2, n0:]))
                w = engine.test_pointwise(mode, p, None, np1, np2, X, None, n0, Nrows, var_f, 0.0, noise, whiten=True, **kw)['out9']
                fm_w, fv_w, _ = _restate(p, np1, np2, True, var_f, mean, X, n0, N)
                assert np.array_equal(w[0, n0:], fm_w[:N]) and np.array_equal(w[1, n0:], fv_w[:N]), '%s: plane sums, whitened predict' % stage
                continue
            acc = out['acc']
            assert np.all(np.isfinite(acc)) and not acc[:, 3].any() and not acc[~used].any()
            live = np.arange(nblk) * T < N
            assert not acc[~live].any(), '%s: a fully masked block added to an accumulator' % stage
            if mode == 'grad':
                for k in ('gm_f', 'gv_f'):
                    assert not out[k][N:].any(), '%s: %s is not exactly 0 at a masked point' % (stage, k)
                assert np.all(np.isfinite(out['gm_f'])) and np.all(np.isfinite(out['gv_f']))
                assert lik == 'bernoulli' or out['gv_f'][:N].all()      # (the Bernoulli dfv is 0 where the plane sums give fm = 0 exactly)
                assert not out['gm_g'].any() and not out['gv_g'].any(), '%s: gm_g / gv_g are not exactly 0' % stage
            if lik == 'gaussian':
                inv = 1.0 / noise
                res = y - fm
                q = res * res + fv
                ve = (LOG2PI_HALF - 0.5 * np.log(noise)) - 0.5 * q * inv
                gmf, gvf = np.where(valid, scale * (res * inv), 0.0), np.where(valid, scale * (-0.5 * inv), 0.0)
                want = np.zeros_like(acc)
                want[:, 0] = hr.wave_sum(np.where(valid, scale * ve, 0.0).reshape(nblk, T))
                want[:, 1] = hr.wave_sum(np.where(valid, scale * (-0.5 * inv + 0.5 * q * inv * inv), 0.0).reshape(nblk, T))
                want[:, 2] = hr.wave_sum(gvf.reshape(nblk, T))
                if mean is not None:
                    want[:, 4] = hr.wave_sum(gmf.reshape(nblk, T))
                    for d in range(D):
                        want[:, 5 + d] = hr.wave_sum((gmf * xs[:, d]).reshape(nblk, T))
                cols = [c for c in range(13) if not (c == 0 and noise != 1.0)]
                assert np.array_equal(acc[:, cols], want[:, cols]), '%s %s noise=%g: accumulators differ from the restatement' % (stage, mode, noise)
                if mode == 'grad':
                    assert np.array_equal(out['gm_f'], gmf) and np.array_equal(out['gv_f'], gvf), '%s: gm_f / gv_f' % stage
            init = rs.randn(*acc.shape)
            twice = engine.test_pointwise(mode, p, None, np1, np2, X, Y, n0, Nrows, var_f, 0.0, noise, repeat=2, acc=init, **kw)['acc']
            assert np.array_equal(twice, np.where(used, (init + acc) + acc, init)), '%s: two launches are not (init + s) + s' % stage
    print('STAGE-LOG %-12s %-34s bit-equal (plane sums, masks, accumulators after two launches, placeholder zeros)' % ('dense-head', stage[11:]))


def test_the_hook_validates_its_arguments(engine):
    from zigp import _lib
    s = _lib.zigp_stage_pointwise()
    for lik in (_lib.LIK_ONOFF, 3):
        assert engine.lib.zigp_test_pointwise_head(engine.ctx, lik, 0, C.byref(s)) == _lib.ZIGP_EARG
        assert b'lik' in engine.lib.zigp_last_error(engine.ctx)
    assert engine.lib.zigp_test_pointwise_head(engine.ctx, _lib.LIK_GAUSSIAN, 0, C.byref(s)) == _lib.ZIGP_EARG      # an empty struct
    assert engine.lib.zigp_test_pointwise_head(engine.ctx, _lib.LIK_GAUSSIAN, 0, None) == _lib.ZIGP_EARG
    with pytest.raises(ValueError):
        engine.test_pointwise('value', np.zeros((3, 1, 1024)), None, 1, 1, np.zeros((1, 1)), np.zeros(1), 0, 1, 1.0, 0.0, 1.0, head='onoff')
