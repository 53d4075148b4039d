"""Stage-level parity of what a whitened call (zigp_set_whiten) launches differently from an unwhitened one, in the style of
tests/test_gpu_stages.py: ONE chunk's stage through the code the chunk loop runs (chunk_forward_white, the whitened point-wise launch;
include/zigp_diag.h zigp_test_chunk_forward_white / zigp_test_pointwise_white) against NumPy over every output element.

  A launch      A = W K (lower-triangular lists) with the weights v = u, s2 = s^2 - 1: plane 0 = sum_m v A, plane 2 = sum_m s2 A^2, plane 1
                untouched; the panel stored in gradient mode only.
  J' launch     J' = (W^T D) A on the upper-triangular lists with a plain storing epilogue; the factor image is D W.
  point-wise    mean = plane 0, var = var0 + plane 2 in value, gradient and predict mode.

(E) exact: small-integer operands whose partial sums stay below 2^53 -- any order gives the same double, the GPU output must be
np.array_equal; (B) normal operands within the componentwise rounding bounds of tests/stage_ref.py."""
import numpy as np
import pytest

import stage_ref as sr

pytestmark = pytest.mark.gpu
TWO53 = 2.0 ** 53


def _pat(r, c, shift=0, dens=1):
    """Small integers in {-3..3} from an integer hash of (row, column): no symmetry, no period (as tests/test_gpu_stages.py)."""
    i, j = np.arange(r, dtype=np.uint64)[:, None], np.arange(c, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(0x9E3779B1) + j * np.uint64(0x85EBCA77) + np.uint64((shift + 1) * 0xC2B2AE3D)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    a = (h % np.uint64(7)).astype(np.float64) - 3.0
    if dens > 1:
        a = np.where((h >> np.uint64(8)) % np.uint64(dens) == 0, a, 0.0)
    return a


def _sentinel():
    from zigp import _lib
    return _lib.STAGE_SENTINEL


def _compare(stage, what, got, ref, bound, exact):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (stage, what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), '%s %s: non-finite output at %s' % (stage, what, np.argwhere(~np.isfinite(got))[:4].tolist())
    err = np.abs(got - ref)
    if exact:
        ok, ratio, k = np.array_equal(got, ref), np.inf, int(np.argmax(err))
    else:
        ratio, k = sr.worst(err, bound)
        ok = ratio <= 1.0
        print('STAGE-LOG %-28s %-30s max error / bound = %.4g' % (stage, what, ratio))
    if not ok:
        idx = np.unravel_index(k, got.shape)
        where = sr.locate(int(idx[0]), int(idx[1])) if got.ndim == 2 else 'column %d = column panel %d' % (idx[-1], idx[-1] // 128)
        pytest.fail('%s, %s: %s at %s: gpu %.17g ref %.17g; %d of %d elements off' % (
            stage, what, 'NOT bit-equal' if exact else 'error / bound = %.3g' % ratio, where, got[idx], ref[idx],
            int(np.sum(got != ref)) if exact else int(np.sum(err > bound)), got.size))


def _operands(M, Nc, kind, seed):
    """W lower triangular, K, the weights v (= u) and d (= s^2 - 1, mixed signs: s < 1 is legal) and the factor image D W."""
    if kind == 'int':
        dens = 1 if M <= 600 else 3
        W, K = np.tril(_pat(M, M, seed, dens)), _pat(M, Nc, seed + 2, dens)
        v = (np.arange(M) * 3 + seed) % 5 - 2.0
        d = (np.arange(M) + seed) % 4 - 1.0                  # -1 (s -> 0), 0 (s = 1), 1, 2
    else:
        rs = np.random.RandomState(300 + seed)
        W, K, v = np.tril(rs.randn(M, M)), rs.randn(M, Nc), rs.randn(M)
        d = (0.3 + rs.rand(M)) ** 2 - 1.0
    return dict(M=M, W=W, v=v, s2=d, K=K, Rt=d[:, None] * W)


def _check_latent(stage, tag, q, out, facts, h, need_grad, exact):
    name = 'latent %s M=%d' % (tag, q['M'])
    M, Mp = q['M'], sr.round_up(q['M'], 128)
    np_alloc, np1, np2 = facts['np'][h], facts['np1'][h], facts['np2'][h]
    part, sent = out['part'], _sentinel()
    assert part.shape[1] == np_alloc and 0 < np1 <= np_alloc and np2 == np1
    for plane in (0, 2):
        assert not np.any(part[plane, :np1] == sent), '%s %s: plane %d has unwritten partial rows below %d' % (stage, name, plane, np1)
        assert np.all(part[plane, np1:] == sent), '%s %s: plane %d written at or beyond row %d' % (stage, name, plane, np1)
    assert np.all(part[1] == sent), '%s %s: plane 1 was written (the whitened A launch owns planes 0 and 2)' % (stage, name)
    a = sr.forward_a1(q['W'], q['v'], q['K'])
    A, B = a['A1'][0], np.abs(q['W']) @ np.abs(q['K'])
    if exact:
        assert max(np.max(np.abs(q['v']) @ B), np.max(np.abs(q['s2']) @ (B * B))) < TWO53
    _compare(stage, name + ' plane 0 = sum v A', sr.pw_plane_sum(part[0], np1), a['s_vA1'][0], a['s_vA1'][1], exact)
    # sum_m d_m A_mn^2: the bound of stage_ref.forward_a1's sum A1^2 with the weights' magnitudes (one more rounding for d_m A)
    _compare(stage, name + ' plane 2 = sum d A^2', sr.pw_plane_sum(part[2], np1), q['s2'] @ (A * A),
             2 * sr.gamma(2 * M + Mp + 5) * (np.abs(q['s2']) @ (B * B)), exact)
    if not need_grad:
        assert out['A1'] is None and out['Jp'] is None
        return
    _compare(stage, name + ' A panel', out['A1'], A, a['A1'][1], exact)
    jp = sr.forward_jp(q['Rt'], q['K'], out['A1'])           # against the panel the J' launch read
    if exact:
        assert np.max(np.abs(q['Rt'].T) @ np.abs(out['A1'])) < TWO53
    _compare(stage, name + " J' panel", out['Jp'], jp['Jp'][0], jp['Jp'][1], exact)


def _run(engine, Mf, Mg, Nc, need_grad, kind, only=None, expect_paired=None):
    lat = [_operands(Mf, Nc, kind, 0), _operands(Mg, Nc, kind, 1)]
    outs, facts = engine.test_chunk_forward(lat[0], lat[1], Nc, need_grad, only=only, whiten=True)
    if expect_paired is not None:
        assert facts['paired'] == expect_paired, facts
    stage = 'white/%s/%s (%d,%d,%d)' % ('grad' if need_grad else 'value', kind, Mf, Mg, Nc)
    for h, tag in enumerate('fg'):
        if only is not None and only != h:
            assert outs[h] is None
            continue
        _check_latent(stage, tag, lat[h], outs[h], facts, h, need_grad, kind == 'int')


LPT = [(1, 1), (9, 9), (127, 129), (200, 136), (300, 100), (100, 520)]
PAIRED = [(128, 128, 32768), (128, 520, 16384), (300, 128, 37888), (128, 128, 56320)]     # whole waves; tails reaching into both lists


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('shape', LPT, ids=lambda s: '%dx%d' % s)
def test_forward_lpt(engine, shape, kind, need_grad):
    """LPT regime, per-latent launches, one and three column-panel groups: (E) and (B)."""
    for Nc in (1024, 3072):
        _run(engine, shape[0], shape[1], Nc, need_grad, kind, expect_paired=0)


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('case', PAIRED, ids=lambda s: '%dx%dx%d' % s)
def test_forward_paired_and_tail(engine, case, kind, need_grad):
    """Paired order, merged f|g launch, with and without the re-dealt tail: the A lists (lower) and the J' lists (upper)."""
    _run(engine, case[0], case[1], case[2], need_grad, kind, expect_paired=1)


@pytest.mark.parametrize('only', [0, 1], ids=['f_alone', 'g_alone'])
def test_forward_one_latent_alone(engine, only):
    for case in ((127, 129, 1024), (300, 128, 37888)):
        for need_grad in (0, 1):
            _run(engine, case[0], case[1], case[2], need_grad, 'int', only=only)


def test_forward_large_M(engine):
    """M = 1100 (nine row blocks): long units, sparse integers keep the sums exact."""
    _run(engine, 1100, 64, 1024, 1, 'int')
    _run(engine, 1100, 64, 1024, 0, 'normal')


# ---- point-wise stage ---------------------------------------------------------------------------------------------------------------
def _rule(stage, name, gpu, np_val, truth, S, scale=1.0):
    """err_gpu <= 4 err_np + 16 eps S per element against the 50-digit evaluation (the rule of tests/test_gpu_stages.py)."""
    if scale != 1.0:
        truth = np.array([t * scale for t in truth], dtype=object)
    e_g, e_n = sr.mp_err(gpu, truth), sr.mp_err(np.asarray(np_val) * scale, truth)
    S = np.asarray(S) * abs(scale)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e_g == 0, 0.0, e_g / (sr.EPS * S))
    print('STAGE-LOG %-28s %-30s max err_gpu / (eps S) = %.4g' % (stage, name, float(np.max(r))))
    bad = e_g > 4 * e_n + 16 * sr.EPS * S
    if bad.any():
        k = int(np.argmax(np.where(bad, r, 0)))
        pytest.fail('%s, %s: point %d: gpu %.17g truth %.17g err_gpu %.3g > 4 * %.3g + 16 eps * %.3g; %d of %d points off' % (
            stage, name, k, np.asarray(gpu).reshape(-1)[k], float(truth[k]), e_g[k], e_n[k], S[k], int(bad.sum()), bad.size))


def _planes(rs, np_alloc, rows, Nc, scale0, lo):
    plane = np.full((np_alloc, Nc), _sentinel())
    plane[:rows] = (lo + rs.rand(rows, Nc)) * scale0 / rows
    return plane


@pytest.mark.parametrize('row_end', [1, 800, 1024], ids=lambda v: 'row_end%d' % v)
def test_pointwise_whitened_mode(engine, row_end):
    """mean = plane 0, var = var0 + plane 2 in all three modes, plane 1 never read (it holds the sentinel, 1.38e306: one read of it and
    nothing stays finite); np1 != np2 per latent; masked columns; the Linear mean function; g_offset; scale.  The latent rows of predict
    are the plane sums bit for bit; the moments, the cotangents and the accumulators follow the 50-digit rule; value mode's accumulators
    equal gradient mode's bit for bit (the same arithmetic with no cotangents written)."""
    Nc, n0, np_alloc, D = 1024, 128, 8, 3
    np1, np2 = (5, 2), (3, 7)
    rs = np.random.RandomState(row_end)
    Nrows = n0 + row_end
    X = rs.randint(-8, 9, (Nrows, D)) / 8.0                 # dyadic: the kernel's fma chain for the mean function is exact
    Y = np.where(rs.rand(Nrows) < 0.4, 0.0, rs.randn(Nrows))
    mean = (rs.randint(-4, 5, D) / 8.0, 0.25)
    var_f, var_g, noise, g_offset, scale = 1.0, 5.0, 0.05, -1.0, 2.5
    sent_plane = np.full((np_alloc, Nc), _sentinel())
    # plane 2 = sum (s^2 - 1) A^2 in (-var, ...): negative where s < 1, the variance stays positive
    pf = np.stack([_planes(rs, np_alloc, np1[0], Nc, 1.0, -0.5), sent_plane, _planes(rs, np_alloc, np2[0], Nc, 0.8, -0.6)])
    pg = np.stack([_planes(rs, np_alloc, np1[1], Nc, 2.0, -0.5), sent_plane, _planes(rs, np_alloc, np2[1], Nc, 4.0, -0.6)])
    fm, fv, gm, gv = sr.pw_inputs(pf, pg, np1, np2, var_f, var_g, g_offset, True, mean=mean, X=X, n0=n0, row_end=Nrows)
    assert fv.min() > 0 and gv.min() > 0
    nv = row_end
    y = np.zeros(Nc)
    y[:nv] = Y[n0:n0 + nv]
    truth = sr.pointwise_mp(fm, fv, gm, gv, y, noise)
    ref = sr.pointwise_np(fm, fv, gm, gv, y, noise)
    S = sr.pointwise_scales(fm, fv, gm, gv, y, noise)
    stage = 'white/pointwise row_end=%d' % row_end
    kw = dict(g_offset=g_offset, scale=scale, mean=mean, whiten=True)
    out = engine.test_pointwise('predict', pf, pg, np1, np2, X, None, n0, Nrows, var_f, var_g, noise, **kw)
    o9 = out['out9'][:, n0:]
    assert np.all(np.isfinite(o9)) and not out['out9'][:, :n0].any()
    for row, want in ((3, fm), (4, fv), (5, gm), (6, gv)):
        _compare(stage, 'predict row %d (plane sums)' % row, o9[row][None, :], want[:nv][None, :], None, True)
    for row, k in ((0, 'gfmean'), (1, 'gfvar'), (2, 'gfmeanu'), (7, 'e1'), (8, 'ev')):
        _rule(stage, 'predict ' + k, o9[row], ref[k][:nv], truth[k][:nv], S[k][:nv])
    grad = engine.test_pointwise('grad', pf, pg, np1, np2, X, Y, n0, Nrows, var_f, var_g, noise, **kw)
    for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv'), ('gm_g', 'dgm'), ('gv_g', 'dgv')):
        assert not grad[k][nv:].any(), '%s: %s is not exactly 0 in a masked column' % (stage, k)
        _rule(stage, name, grad[k][:nv], ref[name][:nv], truth[name][:nv], S[name][:nv], scale)
    valid = np.arange(Nc) < nv
    zero = np.array([0 * t for t in truth['ve']], dtype=object)
    for col, key in ((0, 've'), (1, 'dnoise'), (2, 'dfv'), (3, 'dgv'), (4, 'dfm')):
        tr = np.where(valid, truth[key], zero)
        Sb = np.where(valid, S[key], 0.0).reshape(-1, 64).sum(1)
        nb = np.where(valid, ref[key], 0.0).reshape(-1, 64).sum(1)
        trb = np.array([sum(tr[b * 64:(b + 1) * 64]) for b in range(Nc // 64)], dtype=object)
        live = Sb > 0
        assert not grad['acc'][~live, col].any()
        _rule(stage, 'acc[%d] = block sums of %s' % (col, key), grad['acc'][live, col], nb[live], trb[live], Sb[live], scale)
    value = engine.test_pointwise('value', pf, pg, np1, np2, X, Y, n0, Nrows, var_f, var_g, noise, **kw)
    assert np.array_equal(value['acc'], grad['acc']), stage + ': value mode and gradient mode disagree in the accumulators'
