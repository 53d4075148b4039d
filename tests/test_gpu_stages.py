"""Stage-level parity of the chunk loop's production kernels: each stage of ONE chunk, run through the code the loop runs
(DenseEngine.test_chunk_forward / test_pointwise / test_kgrad / test_rank_update, include/zigp_diag.h), against the host references of
tests/stage_ref.py over EVERY output element.

(E) exact: small-integer operands, every partial sum an integer below 2^53 (asserted on the reference's magnitude sums), so any summation
    order gives the same double and the GPU output must be np.array_equal to the reference.  This is the structural check.
(B) rounding bound: random operands against the componentwise bound written next to each reference; the largest error / bound is printed
    per stage (lines starting with STAGE-LOG; profiles/r08_stage_parity.log keeps a run's).
A failure names stage, latent, row block, column panel, 16 x 16 sub-tile and, for the split-K update, the slice windows."""
import ctypes

import numpy as np
import pytest

from conftest import make_problem
import stage_ref as sr

pytestmark = pytest.mark.gpu

TWO53 = 2.0 ** 53


def _log(stage, what, ratio):
    print('STAGE-LOG %-12s %-34s max error / bound = %.4g' % (stage, what, ratio))


def _pat(r, c, shift=0, dens=1):
    """Small-integer pattern in {-3..3} without symmetry or period (an integer hash of (row, column): a periodic pattern such as
    arange % 7 would hide a k block read 560 columns off, and a symmetric one a mirrored sub-tile), so that a row / column swap, a block
    taken twice or not at all, or a scale at the wrong index changes the product; dens > 1 keeps about one entry in dens (large M: the
    partial sums stay below 2^53)."""
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


def _assert_exact_premise(*mags):
    m = max(float(np.max(x)) for x in mags)
    assert m < TWO53, 'integer premise broken: a magnitude sum reaches %.3g >= 2^53' % m


def _compare(stage, what, got, ref, bound, exact, columns_only=False, extra=None):
    """array_equal (exact) or error <= bound element-wise; the message locates the worst element."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (stage, what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), '%s %s: non-finite output at %s' % (stage, what, np.argwhere(~np.isfinite(got))[:4].tolist())
    err = np.abs(got - ref)
    if exact:
        ok = np.array_equal(got, ref)
        ratio, k = (0.0, 0) if ok else (np.inf, int(np.argmax(err)))
    else:
        ratio, k = sr.worst(err, bound)
        ok = ratio <= 1.0
        _log(stage, what, ratio)
    if not ok:
        idx = np.unravel_index(k, got.shape)
        where = ('column %d = column panel %d, sub-tile column %d' % (idx[-1], idx[-1] // 128, idx[-1] % 128 // 16)) if columns_only \
            else sr.locate(int(idx[0]), int(idx[1]))
        nbad = int(np.sum(got != ref)) if exact else int(np.sum(err > bound))
        msg = '%s, %s: %s at %s: gpu %.17g ref %.17g (error %.3g, bound %s); %d of %d elements off' % (
            stage, what, 'NOT bit-equal' if exact else 'error / bound = %.3g' % ratio, where, got[idx], ref[idx], err[idx],
            'exact' if exact else '%.3g' % np.asarray(bound)[idx], nbad, got.size)
        if not columns_only and got.ndim == 2:
            bi, bj = np.nonzero((got != ref) if exact else (err > bound))
            tiles = sorted(set(zip((bi // 128).tolist(), (bj // 128).tolist())))
            t0 = tiles[0]
            sub = sorted(set(zip((bi[(bi // 128 == t0[0]) & (bj // 128 == t0[1])] % 128 // 16).tolist(),
                                 (bj[(bi // 128 == t0[0]) & (bj // 128 == t0[1])] % 128 // 16).tolist())))
            msg += '; %d (row block, column panel) tiles affected, first %s; in tile %s the sub-tiles %s%s' % (
                len(tiles), tiles[:6], t0, sub[:10], ' ...' if len(sub) > 10 else '')
        if extra is not None:
            msg += '; ' + extra(idx)
        pytest.fail(msg)
    return ratio


def sr_sentinel():
    from zigp import _lib
    return _lib.STAGE_SENTINEL


# =====================================================================================================================================
# forward products
# =====================================================================================================================================
def _latent_operands(M, Nc, kind, seed, need_grad):
    """kind 'int' (E), 'normal' or 'spread' (B: entries over 1e-8 ... 1e8, mixed signs)."""
    if kind == 'int':
        dens = 1 if M <= 600 else 3
        W = np.tril(_pat(M, M, seed, dens))
        K = _pat(M, Nc, seed + 2, dens)
        v = (np.arange(M) * 3 + seed) % 5 - 2.0
        s2 = (np.arange(M) + seed) % 3 * 1.0
        Rt = _pat(M, M, seed + 4, dens) if need_grad else None
    else:
        rs = np.random.RandomState(100 + seed)
        W, K, v, s2 = np.tril(rs.randn(M, M)), rs.randn(M, Nc), rs.randn(M), rs.rand(M) + 0.1
        Rt = rs.randn(M, M) if need_grad else None
        if kind == 'spread':
            W = W * 10.0 ** rs.uniform(-8, 8, W.shape)
            K = K * 10.0 ** rs.uniform(-8, 8, K.shape)
            v = v * 10.0 ** rs.uniform(-8, 8, v.shape)
            s2 = s2 * 10.0 ** rs.uniform(-8, 8, s2.shape)
            if need_grad:
                Rt = Rt * 10.0 ** rs.uniform(-8, 8, Rt.shape)
    return dict(M=M, W=W, v=v, s2=s2, K=K, Rt=Rt)


def _check_forward_latent(tag, q, out, facts, h, need_grad, exact, stage):
    """Panels, and every column sum as the sum of the partial rows the point-wise stage is told to add."""
    name = 'latent %s M=%d' % (tag, q['M'])
    np_alloc, np1, np2 = facts['np'][h], facts['np1'][h], facts['np2'][h]
    part = out['part']
    assert part.shape[1] == np_alloc and 0 < np1 <= np_alloc and 0 < np2 <= np_alloc
    sent = sr_sentinel()
    for plane, rows in ((0, np1), (1, np1), (2, np2)):
        assert not np.any(part[plane, :rows] == sent), '%s %s: plane %d has unwritten partial rows below np = %d: rows %s' % (
            stage, name, plane, rows, sorted(set(np.argwhere(part[plane, :rows] == sent)[:, 0].tolist()))[:8])
        assert np.all(part[plane, rows:] == sent), '%s %s: plane %d was written at or beyond row np = %d' % (stage, name, plane, rows)
    a1 = sr.forward_a1(q['W'], q['v'], q['K'])
    if exact:
        B = np.abs(q['W']) @ np.abs(q['K'])
        _assert_exact_premise(B, np.abs(q['v']) @ B, np.sum(B * B, 0))
    r = [_compare(stage, name + ' A1 panel', out['A1'], a1['A1'][0], a1['A1'][1], exact)]
    for plane, key in ((0, 's_vA1'), (1, 's_A1sq')):
        r.append(_compare(stage, name + ' ' + key, sr.pw_plane_sum(part[plane], np1), a1[key][0], a1[key][1], exact, columns_only=True))
    A1 = out['A1']                                   # the panel the second kernel read
    if need_grad:
        jp = sr.forward_jp(q['Rt'], q['K'], A1)
        if exact:
            B = np.abs(q['Rt'].T) @ np.abs(A1)
            _assert_exact_premise(B, np.sum(np.abs(q['K']) * B, 0))
        r.append(_compare(stage, name + " J' panel", out['Jp'], jp['Jp'][0], jp['Jp'][1], exact))
        r.append(_compare(stage, name + " s_KJ", sr.pw_plane_sum(part[2], np2), jp['s_KJ'][0], jp['s_KJ'][1], exact, columns_only=True))
    else:
        a2 = sr.forward_a2(q['W'], q['s2'], A1)
        if exact:
            B = np.abs(q['W'].T) @ np.abs(A1)
            _assert_exact_premise(np.abs(q['s2']) @ (B * B))
        r.append(_compare(stage, name + ' s_s2A2sq', sr.pw_plane_sum(part[2], np2), a2['s_s2A2sq'][0], a2['s_s2A2sq'][1], exact, columns_only=True))
    return max(r)


def _run_forward(engine, Mf, Mg, Nc, need_grad, kind, only=None, expect=None):
    lat = [_latent_operands(Mf, Nc, kind, 0, need_grad), _latent_operands(Mg, Nc, kind, 1, need_grad)]
    outs, facts = engine.test_chunk_forward(lat[0], lat[1], Nc, need_grad, only=only)
    if expect is not None:
        assert (facts['paired'], facts['tail_f'], facts['tail_g']) == expect, ('the planner left the regime this case is about', facts)
    stage = 'forward/%s/%s' % ('grad' if need_grad else 'value', kind)
    for h, tag in enumerate('fg'):
        if only is not None and only != h:
            assert outs[h] is None
            continue
        assert facts['Mp'][h] == sr.round_up(lat[h]['M'], 128)
        _check_forward_latent(tag, lat[h], outs[h], facts, h, need_grad, kind == 'int', '%s (%d,%d,%d)%s' % (
            stage, Mf, Mg, Nc, '' if only is None else ' latent %s alone' % tag))
    return facts


LPT_SHAPES = [(1, 1), (9, 9), (127, 129), (200, 136), (300, 100), (100, 520), (1100, 64)]
# (Mf, Mg, Nc) -> [wg_f, wg_g, per_f, per_g, tail_f, tail_g, worst, paired] of the A1 lists (zigp_test_trmm_list, lower = 1, tail on)
PAIRED = {(128, 128, 32768): [256, 256, 2, 2, 0, 0, 0, 1], (128, 520, 16384): [128, 384, 2, 2, 0, 0, 0, 1],
          (300, 128, 37888): [408, 104, 3, 3, 592, 296, 5, 1], (128, 128, 56320): [256, 256, 2, 2, 440, 440, 2, 1]}


def test_paired_regimes_are_the_planned_ones(engine):
    """The four paired shapes below run the regime they are meant to: a planner change that silently leaves it is noticed here."""
    for (Mf, Mg, Nc), want in PAIRED.items():
        out = (ctypes.c_int64 * 8)()
        assert engine.lib.zigp_test_trmm_list(1, Mf, Mg, Nc, 1, out) == 0
        assert list(out) == want, ((Mf, Mg, Nc), list(out))
    for Mf, Mg in LPT_SHAPES:
        for Nc in (1024, 3072):
            out = (ctypes.c_int64 * 8)()
            assert engine.lib.zigp_test_trmm_list(1, Mf, Mg, Nc, 1, out) == 0
            assert out[7] == 0 and out[4] == 0 and out[5] == 0, ((Mf, Mg, Nc), list(out))


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('Nc', [1024, 3072])
@pytest.mark.parametrize('shape', LPT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_forward_lpt_exact(engine, shape, Nc, need_grad):
    """(E) LPT regime, per-latent launches: every element of A1, J' and of the fused column sums bit-equal to the integer reference."""
    _run_forward(engine, shape[0], shape[1], Nc, need_grad, 'int', expect=(0, 0, 0))


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('Nc', [1024, 3072])
@pytest.mark.parametrize('shape', LPT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_forward_lpt_bound(engine, shape, Nc, need_grad):
    """(B) the same launches on normal operands, within the componentwise rounding bound."""
    _run_forward(engine, shape[0], shape[1], Nc, need_grad, 'normal', expect=(0, 0, 0))


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('case', sorted(PAIRED), ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('kind', ['int', 'normal'])
def test_forward_paired_and_tail(engine, kind, case, need_grad):
    """Paired order + merged f|g launch, whole waves and with the LPT tail reaching into both latents' lists: (E) and (B)."""
    want = PAIRED[case]
    _run_forward(engine, case[0], case[1], case[2], need_grad, kind, expect=(1, want[4], want[5]))


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('case', [(200, 136, 1024), (300, 128, 37888)], ids=lambda s: '%dx%dx%d' % s)
def test_forward_spread_operands(engine, case, need_grad):
    """(B) entries spread over 1e-8 ... 1e8 with mixed signs: cancellation is real, the bound still holds element-wise."""
    _run_forward(engine, case[0], case[1], case[2], need_grad, 'spread')


@pytest.mark.parametrize('need_grad', [0, 1], ids=['value', 'grad'])
@pytest.mark.parametrize('case', [(127, 129, 1024), (300, 100, 3072), (128, 520, 16384), (300, 128, 37888)], ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('only', [0, 1], ids=['f_alone', 'g_alone'])
def test_forward_one_latent_alone(engine, only, case, need_grad):
    """(E) one latent's lists of the pair's plan on their own: its outputs do not depend on the other latent's workgroups."""
    _run_forward(engine, case[0], case[1], case[2], need_grad, 'int', only=only)


# =====================================================================================================================================
# rank-N update
# =====================================================================================================================================
def _syrk_chunks(M, Ncs, kind, seed=0):
    chunks = []
    for i, Nc in enumerate(Ncs):
        if kind == 'int':
            A1 = _pat(M, Nc, seed + i)
            gv = _pat(1, Nc, seed + i + 50)[0]               # mixed signs, exact zeros, no period along k
        else:
            rs = np.random.RandomState(200 + seed + i)
            A1, gv = rs.randn(M, Nc), rs.randn(Nc)
            gv[::11] = 0.0
            if kind == 'spread':
                A1 = A1 * 10.0 ** rs.uniform(-8, 8, A1.shape)
                gv = gv * 10.0 ** rs.uniform(-8, 8, gv.shape)
        chunks.append((A1, gv))
    return chunks


def _slice_report(chunks, plan, got, ref):
    """For the worst element's row inside its tile: the slice windows and single BK steps whose reference contribution, dropped or taken
    twice, is the observed difference (compared over the tile's whole row, so that a coincidence in one element does not count)."""
    def f(idx):
        i, j = int(idx[0]), int(idx[1])
        S = plan[1] if i // 128 == j // 128 else plan[0]
        cols = slice(j // 128 * 128, min(j // 128 * 128 + 128, got.shape[1]))
        diff = got[i, cols] - ref[i, cols]
        parts, steps = [], []

        def matches(A1, gv, k0, k1):
            c = (A1[i, k0:k1] * gv[k0:k1]) @ A1[cols, k0:k1].T
            tol = 1e-9 * max(np.max(np.abs(c)), 1e-300)
            return np.any(c != 0) and (np.all(np.abs(diff + c) <= tol) or np.all(np.abs(diff - c) <= tol))
        for c, (A1, gv) in enumerate(chunks):
            win = sr.slice_windows(A1.shape[1] // 16, S)
            for s, (k0, k1) in enumerate(win):
                if matches(A1, gv, k0, k1):
                    parts.append('chunk %d slice %d of %d, k window [%d, %d)' % (c, s, S, k0, k1))
            for k0 in range(0, A1.shape[1], 16):
                if matches(A1, gv, k0, k0 + 16):
                    w = [n for n, (a, b) in enumerate(win) if a <= k0 < b][0]
                    steps.append('chunk %d BK step [%d, %d) of slice %d, window [%d, %d)' % (c, k0, k0 + 16, w, win[w][0], win[w][1]))
        return 'split-K plan So=%d Sd=%d, %s tile; slices whose contribution (dropped or doubled) is the difference of this row: %s; single BK steps: %s' % (
            plan[0], plan[1], 'diagonal' if i // 128 == j // 128 else 'off-diagonal', parts[:4] or 'none', steps[:4] or 'none')
    return f


def _run_syrk(engine, M, Ncs, kind):
    chunks = _syrk_chunks(M, Ncs, kind)
    C1, plan = engine.test_rank_update(chunks)
    assert plan == sr.syr_plan(sr.round_up(M, 128) // 128), ('split-K plan', plan)
    ref, bound = sr.rank_update(chunks)
    if kind == 'int':
        _assert_exact_premise(sum((np.abs(A) * np.abs(g)[None, :]) @ np.abs(A).T for A, g in chunks))
    stage = 'rank-N/%s M=%d Nc=%s' % (kind, M, '+'.join(map(str, Ncs)))
    assert np.array_equal(C1, C1.T), stage + ': C1 is not symmetric'
    _compare(stage, 'C1', C1, ref, bound, kind == 'int', extra=_slice_report(chunks, plan, C1, ref))
    return plan


SYR_PLANS = [(100, (64, 32)), (256, (64, 32)), (384, (64, 32)), (512, (64, 32)), (640, (32, 16)), (768, (16, 8)), (896, (16, 8)),
             (1024, (16, 8)), (1152, (16, 8)), (2048, (16, 8))]


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('M,plan', SYR_PLANS, ids=lambda v: str(v))
def test_rank_update_every_plan(engine, M, plan, kind):
    """Every plan syr_plan can return, at Nc = 1024: 64 BK steps, i.e. ONE step per off-diagonal slice and two per diagonal slice at So = 64."""
    assert _run_syrk(engine, M, [1024], kind) == plan


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('Ncs', [[2048], [8192], [8192, 1024]], ids=lambda v: '+'.join(map(str, v)))
@pytest.mark.parametrize('M', [512, 1000, 1100])
def test_rank_update_chunks_and_ragged_rows(engine, M, Ncs, kind):
    """Longer k ranges, accumulation over two chunks of different size (EpiAccum), M not a multiple of 128."""
    _run_syrk(engine, M, Ncs, kind)


def test_rank_update_spread_operands(engine):
    _run_syrk(engine, 300, [2048], 'spread')


@pytest.mark.parametrize('M', [200, 640, 1024])
def test_rank_update_invalid_columns_contribute_nothing(engine, M):
    """gv = 0 on every column >= row_end (what the point-wise stage's sc = valid ? scale : 0 promises) with large finite garbage in those
    columns of A1: bit-identical to the same call with the columns zeroed."""
    Nc, row_end = 2048, 1500
    rs = np.random.RandomState(M)
    A1, gv = rs.randn(M, Nc), rs.randn(Nc)
    gv[row_end:] = 0.0
    clean = A1.copy()
    clean[:, row_end:] = 0.0
    A1[:, row_end:] = 1e150 * rs.randn(M, Nc - row_end)
    a, _ = engine.test_rank_update([(A1, gv)])
    b, _ = engine.test_rank_update([(clean, gv)])
    assert np.all(np.isfinite(a))
    _compare('rank-N/masked M=%d' % M, 'C1 (garbage columns against zeroed ones)', a, b, None, True)


# =====================================================================================================================================
# Kuf cotangent reductions
# =====================================================================================================================================
def _kgrad_operands(M, D, Nc, Nrows, kind, seed=0):
    if kind == 'int':
        Jp, K = _pat(M, Nc, seed), _pat(M, Nc, seed + 3)
        alpha = (np.arange(M) * 2 + seed) % 5 - 2.0
        gm, gv = _pat(1, Nc, seed + 7)[0], _pat(1, Nc, seed + 9)[0]
        X, Z = _pat(Nrows, D, seed + 1), _pat(M, D, seed + 5)
    else:
        rs = np.random.RandomState(300 + seed)
        Jp, K, alpha, gm, gv = rs.randn(M, Nc), rs.rand(M, Nc), rs.randn(M), rs.randn(Nc), rs.randn(Nc)
        X, Z = rs.rand(Nrows, D), rs.rand(M, D)
    return Jp, K, alpha, gm, gv, X, Z


def _kgrad_check(stage, got_slabs, ref, bound, exact, init=None):
    got = got_slabs.sum(0) if init is None else got_slabs.sum(0) - init.sum(0)
    D = (ref.shape[1] - 2) // 2
    cols = ['sum FK'] + ['sum FK dx_%d' % d for d in range(D)] + ['sum FK dx_%d^2' % d for d in range(D)] + ['sum K gm']
    extra = lambda idx: 'inducing row %d (kgrad block %d), column %s' % (idx[0], idx[0] // 4, cols[idx[1]])
    return _compare(stage, 'krow', got, np.asarray(ref, dtype=np.float64), bound, exact, extra=extra)


@pytest.mark.parametrize('D', range(1, 9))
def test_kgrad_exact_every_dimension(engine, D):
    """(E) every D x both forms on integer operands: the centred form (integer centre), the per-row form and the reference agree bit for
    bit; M not a multiple of KG_ROWS, n0 > 0, fewer rows than columns (nmax clipping inside the last split)."""
    for M in (1, 2, 3, 5, 130):
        Nc, Nrows, n0 = 1024, 1500, 600                     # 900 valid columns: the last KG_SPLIT span is cut at 132 of 256
        Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, Nrows, 'int', seed=D)
        gm[Nrows - n0:] = 0.0                               # what the point-wise stage leaves in masked columns
        gv[Nrows - n0:] = 0.0
        ref, bnd = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=np.ones(D))
        _assert_exact_premise(bnd / sr.gamma(min(Nc, Nrows - n0) + 8))
        centred = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, centre=np.ones(D), exact=False)
        per_row = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, exact=True)
        _kgrad_check('kgrad/int D=%d M=%d centred' % (D, M), centred, ref, None, True)
        _kgrad_check('kgrad/int D=%d M=%d per-row' % (D, M), per_row, ref, None, True)
        assert np.array_equal(centred, per_row), 'the two forms differ in a slab'


@pytest.mark.parametrize('exact', [0, 1], ids=['centred', 'per_row'])
@pytest.mark.parametrize('D', range(1, 9))
def test_kgrad_bound_every_dimension(engine, D, exact):
    """(B) every D x both forms on random operands against the extended-precision reference; the host's own centre and rule (exact=None)
    give the centred form at this spread, bit for bit."""
    M, Nc, Nrows, n0 = 130, 2048, 2500, 700
    Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, Nrows, 'normal', seed=D)
    gm[Nrows - n0:] = 0.0
    gv[Nrows - n0:] = 0.0
    c = Z.mean(0)
    ref, bnd = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=None if exact else c, dtype=np.longdouble)
    got = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, exact=bool(exact), ell=np.ones(D))
    _kgrad_check('kgrad/normal D=%d %s' % (D, 'per-row' if exact else 'centred'), got, ref, bnd * (1 + 2.0 ** -11), False)
    if not exact:
        auto = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, ell=np.ones(D))
        assert np.array_equal(auto, got), "the host's centre is not the mean inducing input, or its rule chose the per-row form"


@pytest.mark.parametrize('row_end', [1, 100, 256, 257, 900, 1023, 1024])
def test_kgrad_row_end_inside_the_splits(engine, row_end):
    """The last valid column inside the first / last KG_SPLIT span, at a span boundary and at 1 (three splits with no valid column)."""
    M, D, Nc = 7, 3, 1024
    Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, row_end, 'int', seed=row_end)
    gm[row_end:] = 0.0
    gv[row_end:] = 0.0
    ref, _ = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, 0, centre=np.ones(D))
    for exact in (False, True):
        got = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, centre=np.ones(D), exact=exact)
        _kgrad_check('kgrad/int row_end=%d %s' % (row_end, 'per-row' if exact else 'centred'), got, ref, None, True)
        span = Nc // 4
        for sp in range(4):
            if sp * span >= row_end:
                assert not got[sp].any(), 'split %d has no valid column and wrote something' % sp


def test_kgrad_second_call_accumulates(engine):
    M, D, Nc = 5, 2, 1024
    a = _kgrad_operands(M, D, Nc, Nc, 'int', seed=1)
    b = _kgrad_operands(M, D, Nc, Nc, 'int', seed=2)
    first = engine.test_kgrad(*a[:5], a[5], a[6], centre=np.ones(D), exact=False)
    both = engine.test_kgrad(*b[:5], b[5], b[6], centre=np.ones(D), exact=False, krow=first)
    ra, _ = sr.kgrad(*a[:5], a[5], a[6], 0, centre=np.ones(D))
    rb, _ = sr.kgrad(*b[:5], b[5], b[6], 0, centre=np.ones(D))
    _kgrad_check('kgrad/int accumulate', both, ra + rb, None, True)


def test_kgrad_centred_form_at_300_lengthscales(engine):
    """The centred form with the inducing inputs spread over 300 lengthscales (ell = 1), against the extended-precision reference with
    the bound of the centred sums: pins the kernel comment's '(|dz| / ell)^2 ulp of cancellation'."""
    M, D, Nc = 64, 2, 4096
    rs = np.random.RandomState(7)
    Z = rs.uniform(-150.0, 150.0, (M, D))
    X = Z[rs.randint(0, M, Nc)] + rs.randn(Nc, D)            # data near the inducing inputs, so that K is not negligible
    K = np.exp(-0.5 * ((X[None, :, :] - Z[:, None, :]) ** 2).sum(2))
    Jp, alpha, gm, gv = rs.randn(M, Nc), rs.randn(M), rs.randn(Nc), rs.randn(Nc)
    c = Z.mean(0)
    ref, bnd = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, 0, centre=c, dtype=np.longdouble)
    got = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, ell=np.ones(D))           # the host's rule: spread 150 < 1e3 -> centred
    assert np.array_equal(got, engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, centre=c, exact=False))
    _kgrad_check('kgrad/spread300 centred', got, ref, bnd * (1 + 2.0 ** -11), False)
    ref_x, bnd_x = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, 0, dtype=np.longdouble)
    _kgrad_check('kgrad/spread300 per-row', engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, exact=True), ref_x, bnd_x * (1 + 2.0 ** -11), False)


# =====================================================================================================================================
# point-wise stage
# =====================================================================================================================================
def _rule(stage, name, gpu, np_val, truth, S, scale=1.0):
    """err_gpu <= 4 err_np + 16 eps S per element (truth: mpmath, 50 digits); prints the largest err_gpu / (eps S)."""
    if scale != 1.0:
        truth = np.array([t * scale for t in truth], dtype=object)
    e_g, e_n = sr.mp_err(gpu, truth), sr.mp_err(np.asarray(np_val) * scale, truth)
    S = np.asarray(S) * abs(scale)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e_g == 0, 0.0, e_g / (sr.EPS * S))
        r_np = np.where(e_n == 0, 0.0, e_n / (sr.EPS * S))
    print('STAGE-LOG %-12s %-34s max err_gpu / (eps S) = %.4g (numpy: %.4g)' % (stage, name, float(np.max(r)), float(np.max(r_np))))
    bad = e_g > 4 * e_n + 16 * sr.EPS * S
    if bad.any():
        k = int(np.argmax(np.where(bad, r, 0)))
        pytest.fail('%s, %s: point %d (block %d, lane %d): gpu %.17g truth %.17g err_gpu %.3g > 4 * %.3g + 16 eps * %.3g; %d of %d points off' % (
            stage, name, k, k // 64, k % 64, np.asarray(gpu).reshape(-1)[k], float(truth[k]), e_g[k], e_n[k], S[k], int(bad.sum()), bad.size))


def _block_sums_mp(vals):
    return np.array([sum(vals[b * 64:(b + 1) * 64]) for b in range(len(vals) // 64)], dtype=object)


def _pw_planes(rs, np_alloc, rows, Nc, sentinel, scale0, positive):
    """[np_alloc][Nc] plane whose first `rows` rows hold a value split over them, the rest the sentinel."""
    plane = np.full((np_alloc, Nc), sentinel)
    plane[:rows] = (rs.rand(rows, Nc) if positive else rs.randn(rows, Nc)) * scale0 / max(rows, 1)
    return plane


@pytest.mark.parametrize('mean_kind,D', [('off', 2), ('constant', 1), ('linear', 1), ('linear', 3), ('linear', 8)])
@pytest.mark.parametrize('row_end', [1, 640, 800, 1024], ids=lambda v: 'row_end%d' % v)
def test_pointwise_partial_rows_masking_and_accumulators(engine, row_end, mean_kind, D):
    """(i) The part-plane accumulation (np1 != np2, the sentinel in every row >= np*, plane 1 all sentinel in gradient mode), row_end in
    the middle of a 64-point block / at a block boundary / at 1, scale != 1, g_offset = -1, the mean function's sums, two accumulating
    launches.  Masked columns give exactly 0 in gm / gv and add exactly 0 to every accumulator."""
    Nc, n0, np_alloc = 1024, 128, 8
    np1, np2 = (5, 2), (3, 7)
    sent = sr_sentinel()
    rs = np.random.RandomState(row_end + D)
    Nrows = n0 + row_end
    X = rs.randint(-8, 9, (Nrows, D)) / 8.0                 # dyadic: the kernel's fma chain for the mean function is exact, so numpy replicates it
    Y = np.where(rs.rand(Nrows) < 0.4, 0.0, rs.randn(Nrows))
    mean = None if mean_kind == 'off' else ((np.zeros(D) if mean_kind == 'constant' else rs.randint(-4, 5, D) / 8.0), 0.25)
    var_f, var_g, noise, g_offset, scale = 1.0, 5.0, 0.05, -1.0, 2.5
    re_abs = n0 + row_end
    for mode in ('predict', 'value', 'grad'):
        gradvar = mode == 'grad'
        pf = np.stack([_pw_planes(rs, np_alloc, np1[0], Nc, sent, 1.0, False),
                       np.full((np_alloc, Nc), sent) if gradvar else _pw_planes(rs, np_alloc, np1[0], Nc, sent, 0.5, True),
                       _pw_planes(rs, np_alloc, np2[0], Nc, sent, 0.3, True)])
        pg = np.stack([_pw_planes(rs, np_alloc, np1[1], Nc, sent, 2.0, False),
                       np.full((np_alloc, Nc), sent) if gradvar else _pw_planes(rs, np_alloc, np1[1], Nc, sent, 2.0, True),
                       _pw_planes(rs, np_alloc, np2[1], Nc, sent, 1.0, True)])
        fm, fv, gm, gv = sr.pw_inputs(pf, pg, np1, np2, var_f, var_g, g_offset, gradvar, mean=mean, X=X, n0=n0, row_end=re_abs)
        nv = row_end
        y = np.zeros(Nc)
        y[:nv] = Y[n0:n0 + nv]
        stage = 'pointwise/%s row_end=%d mean=%s D=%d' % (mode, row_end, mean_kind, D)
        out = engine.test_pointwise(mode, pf, pg, np1, np2, X, None if mode == 'predict' else Y, n0, re_abs, var_f, var_g, noise,
                                    g_offset=g_offset, scale=scale, mean=mean)
        if mode == 'predict':
            o9 = out['out9'][:, n0:]
            for row, ref in ((3, fm), (4, fv), (5, gm), (6, gv)):      # the doubles the kernel evaluates at: the plane sums, bit for bit
                _compare(stage, 'out9 row %d (plane sums)' % row, o9[row][None, :], ref[:nv][None, :], None, True, columns_only=True)
            assert not out['out9'][:, :n0].any(), 'predict wrote in front of n0'
            truth = sr.pointwise_mp(fm[:nv], fv[:nv], gm[:nv], gv[:nv], y[:nv], noise)
            ref = sr.pointwise_np(fm[:nv], fv[:nv], gm[:nv], gv[:nv], y[:nv], noise)
            S = sr.pointwise_scales(fm[:nv], fv[:nv], gm[:nv], gv[:nv], y[:nv], noise)
            for row, k in ((0, 'gfmean'), (1, 'gfvar'), (2, 'gfmeanu'), (7, 'e1'), (8, 'ev')):
                _rule(stage, k, o9[row], ref[k], truth[k], S[k])
            continue
        truth = sr.pointwise_mp(fm, fv, gm, gv, y, noise)
        ref = sr.pointwise_np(fm, fv, gm, gv, y, noise)
        S = sr.pointwise_scales(fm, fv, gm, gv, y, noise)
        valid = np.arange(Nc) < nv
        if mode == 'grad':
            for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv'), ('gm_g', 'dgm'), ('gv_g', 'dgv')):
                assert not out[k][nv:].any(), '%s: %s is not exactly 0 in a masked column' % (stage, k)
                _rule(stage, name, out[k][:nv], ref[name][:nv], truth[name][:nv], S[name][:nv], scale)
        # accumulators: block sums of the valid points (S and the truth summed per block; masked points add exactly 0)
        acc = out['acc']
        zero = np.array([0 * t for t in truth['ve']], dtype=object)
        cols = [(0, 've'), (1, 'dnoise'), (2, 'dfv'), (3, 'dgv')]
        extra_S, extra_np, extra_tr = {}, {}, {}
        if mean is not None:
            cols.append((4, 'dfm'))
            xs = np.zeros((Nc, D))
            xs[:nv] = X[n0:n0 + nv]
            for d in range(D):
                key = 'dfm_x%d' % d
                cols.append((5 + d, key))
                extra_S[key], extra_np[key] = S['dfm'] * np.abs(xs[:, d]), ref['dfm'] * xs[:, d]
                extra_tr[key] = np.array([t * float(x) for t, x in zip(truth['dfm'], xs[:, d])], dtype=object)
        for col, key in cols:
            tr = extra_tr.get(key, truth.get(key))
            tr = np.where(valid, tr, zero)
            Sb = np.where(valid, extra_S.get(key, S.get(key)), 0.0).reshape(-1, 64).sum(1)
            nb = np.where(valid, extra_np.get(key, ref.get(key)), 0.0).reshape(-1, 64).sum(1)
            live = Sb > 0
            assert not acc[~live, col].any(), '%s: a fully masked block added to accumulator %d' % (stage, col)
            if live.any():
                _rule(stage, 'acc[%d] = block sums of %s' % (col, key), acc[live, col], nb[live], _block_sums_mp(tr)[live], Sb[live], scale)
        if mean is None:
            assert not acc[:, 4:].any()
        else:
            assert not acc[:, 5 + D:].any()
        # acc keeps accumulating: two launches onto given initial values = (init + s) + s with the s of the single launch, bit for bit
        init = rs.randn(*acc.shape)
        twice = engine.test_pointwise(mode, pf, pg, np1, np2, X, Y, n0, re_abs, var_f, var_g, noise, g_offset=g_offset, scale=scale, mean=mean,
                                      repeat=2, acc=init)['acc']
        used = np.zeros_like(acc, dtype=bool)
        used[:, :4] = True
        if mean is not None:
            used[:, 4:5 + D] = True
        want = np.where(used, (init + acc) + acc, init)
        assert np.array_equal(twice, want), '%s: the accumulators of two launches are not (init + s) + s' % stage


GRID = dict(gm=[-40, -8, -3, -1, -1e-3, 0, 1e-3, 1, 3, 8, 40], gv=[1e-8, 1e-3, 0.1, 1, 10, 1e3, 1e6], fm=[-5, -0.1, 0, 0.3, 7],
            fv=[1e-10, 1e-3, 1, 50], y=[0, 0.7, -3])


@pytest.mark.parametrize('noise', [1e-4, 1e-2, 1.0])
def test_pointwise_arithmetic_over_the_grid(engine, noise):
    """(ii) pointwise_eval over gm x gv x fm x fv x y (4620 points per noise value; the noise is a launch argument, so the 13 860 points are
    three launches per mode) against the 50-digit evaluation: err_gpu <= 4 err_np + 16 eps S per point and output, nothing excluded.  The
    planes are built so that the kernel's few additions (var + plane 2, var - plane 1 + plane 2, + g_offset) are replicated exactly: the
    grid values are targets, the doubles the kernel really evaluates at (rows 3 ... 6 of out9, bit-equal to the numpy replica) are what
    both references are fed.
    The m2 / mv branch values 0 and 0.5 of the reverse pass (e2r <= 0, evr <= 0) are unreachable through the formulas -- cdf >= 1e-3 keeps
    cdf - 2 T and cdf - 2 T - cdf^2 positive on this grid and everywhere we could find -- so no input is invented for them."""
    g = np.array(np.meshgrid(GRID['gm'], GRID['gv'], GRID['fm'], GRID['fv'], GRID['y'], indexing='ij'), dtype=np.float64).reshape(5, -1)
    n = g.shape[1]
    assert n == 4620
    Nc = sr.round_up(n, 1024)
    pad = lambda a, fill: np.concatenate([a, np.full(Nc - n, fill)])
    var_f, var_g = 1.0, 1.0
    pf, pg = np.zeros((3, 1, Nc)), np.zeros((3, 1, Nc))
    pf[0, 0], pf[2, 0] = pad(g[2], 0.0), pad(g[3] - var_f, 0.0)
    pg[0, 0], pg[2, 0] = pad(g[0], 0.0), pad(g[1] - var_g, 0.0)
    Y = g[4].copy()
    X = np.zeros((n, 1))
    np1 = np2 = (1, 1)
    fm, fv, gm, gv = (a[:n] for a in sr.pw_inputs(pf, pg, np1, np2, var_f, var_g, 0.0, False))
    fm2, fv2, gm2, gv2 = (a[:n] for a in sr.pw_inputs(pf, pg, np1, np2, var_f, var_g, 0.0, True))
    assert np.array_equal(fv, fv2) and np.array_equal(gv, gv2)      # var - 0 + p2 and var + p2: one double
    truth = sr.pointwise_mp_cached(fm, fv, gm, gv, Y, noise)      # the Kronecker wrapper's grid test evaluates at the same doubles
    ref = sr.pointwise_np(fm, fv, gm, gv, Y, noise)
    S = sr.pointwise_scales(fm, fv, gm, gv, Y, noise)
    stage = 'pointwise/grid noise=%g' % noise
    assert all(t > 0 for t in truth['e2']) and all(t > 0 for t in truth['ev']), 'a grid point reaches a clipping branch (the clipped value is exactly 0)'
    pr = engine.test_pointwise('predict', pf, pg, np1, np2, X, None, 0, n, var_f, var_g, noise)['out9']
    for row, a in ((3, fm), (4, fv), (5, gm), (6, gv)):
        _compare(stage, 'out9 row %d (evaluation point)' % row, pr[row][None, :], a[None, :], None, True, columns_only=True)
    for row, k in ((0, 'gfmean'), (1, 'gfvar'), (2, 'gfmeanu'), (7, 'e1'), (8, 'ev')):
        _rule(stage, k, pr[row], ref[k], truth[k], S[k])
    gr = engine.test_pointwise('grad', pf, pg, np1, np2, X, Y, 0, n, var_f, var_g, noise)
    for k, name in (('gm_f', 'dfm'), ('gv_f', 'dfv'), ('gm_g', 'dgm'), ('gv_g', 'dgv')):
        _rule(stage, name, gr[k][:n], ref[name], truth[name], S[name])
    va = engine.test_pointwise('value', pf, pg, np1, np2, X, Y, 0, n, var_f, var_g, noise)
    nb = (n + 63) // 64
    zero = [0 * truth['ve'][0]] * (nb * 64 - n)
    for mode, acc in (('value', va['acc']), ('grad', gr['acc'])):
        for col, key in ((0, 've'), (1, 'dnoise')):
            tr = _block_sums_mp(list(truth[key]) + zero)
            Sb = np.concatenate([S[key], np.zeros(nb * 64 - n)]).reshape(-1, 64).sum(1)
            rb = np.concatenate([ref[key], np.zeros(nb * 64 - n)]).reshape(-1, 64).sum(1)
            _rule(stage, '%s acc[%d] = summed %s' % (mode, col, key), acc[:nb, col], rb, tr, Sb)
        assert not acc[nb:].any()
    assert np.array_equal(va['acc'][:, :2], gr['acc'][:, :2])        # the same doubles in, the same sums out


# =====================================================================================================================================
# the stages composed, tied to the real call
# =====================================================================================================================================
def _compose(engine, X, Y, p, Nc, need_grad, jitter=1e-6):
    """Value mode: W from test_potrf_trtri and v = W u formed on the host, nothing else differs from the step.  Gradient mode: the J' launch
    also reads Rt = (Q W^T)^T, an M x M product chain whose rounding the variance sees times cond(Kuu) (a host-formed Rt moves the data
    term by 4e-12), so W, v, alpha and Rt are the ones the step's own M x M forward leaves (test_latents_forward)."""
    N = X.shape[0]
    lat = []
    dev = engine.test_latents_forward(p, jitter, True) if need_grad else None
    for h, tag in enumerate('fg'):
        Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
        M = Z.shape[0]
        K = np.zeros((M, Nc))
        K[:, :N] = engine.test_kuf(X, Z, ell, var)
        Kuu = engine.rbf_K(Z, None, ell, var) + jitter * np.eye(M)
        L, W = engine.test_potrf_trtri(Kuu, split_k=True)
        u, s2 = p['u_%sm' % tag].reshape(-1), p['u_%ss_sqrt' % tag].reshape(-1) ** 2
        v, alpha, Rt = W @ u, None, None                               # value mode: v formed on the host
        if need_grad:
            assert np.array_equal(W, dev[h]['W']), 'test_potrf_trtri and the M x M forward give different factors'
            v, alpha, Rt = dev[h]['v'], dev[h]['alpha'], dev[h]['Rt']
        lat.append(dict(M=M, W=W, v=v, s2=s2, K=K, Rt=Rt, alpha=alpha, Z=Z, var=var))
    outs, facts = engine.test_chunk_forward(lat[0], lat[1], Nc, need_grad)
    pw = engine.test_pointwise('grad' if need_grad else 'value', outs[0]['part'], outs[1]['part'], facts['np1'], facts['np2'], X, Y, 0, N,
                               p['var_f'], p['var_g'], p['noise'])
    res = dict(data=float(np.sum(pw['acc'][:, 0])), acc=pw['acc'])
    if need_grad:
        res.update(gm_f=pw['gm_f'], gv_f=pw['gv_f'], gm_g=pw['gm_g'], gv_g=pw['gv_g'])
        for h, tag in enumerate('fg'):
            res['krow_' + tag] = engine.test_kgrad(outs[h]['Jp'], lat[h]['K'], lat[h]['alpha'], pw['gm_' + tag], pw['gv_' + tag], X, lat[h]['Z'],
                                                   ell=p['ell_' + tag])
            res['C1_' + tag] = engine.test_rank_update([(outs[h]['A1'], pw['gv_' + tag])])[0]
    return res


def test_composition_matches_the_real_step(engine):
    """A ragged two-latent problem through the diagnostics, one stage into the next (K from test_kuf, W from test_potrf_trtri): bit for bit
    what a second run of the composition gives, and the data term of engine.elbo to 1e-12 relative -- the bar
    test_automatic_rule_takes_a_short_row_range... sets for the same kernels run in a different split."""
    X, Y, p = make_problem(2900, 100, 3, seed=21, Mg=136)
    engine.set_data(X, Y)
    for need_grad in (False, True):
        ed, _, _ = engine.elbo(p, jitter=1e-6, need_grad=need_grad)
        a = _compose(engine, X, Y, p, 3072, need_grad)
        b = _compose(engine, X, Y, p, 3072, need_grad)
        for k in a:
            assert np.array_equal(a[k], b[k]), 'composition not bit-stable: ' + k
        rel = abs(a['data'] - ed) / abs(ed)
        print('STAGE-LOG composition  need_grad=%d data term %.15e engine %.15e rel %.3g' % (need_grad, a['data'], ed, rel))
        assert rel <= 1e-12, (need_grad, a['data'], ed)
        if need_grad:
            for k in ('gm_f', 'gv_f', 'gm_g', 'gv_g'):
                assert not a[k][X.shape[0]:].any()
            assert np.array_equal(a['C1_f'], a['C1_f'].T)


def test_stage_calls_leave_the_context_usable(engine):
    """A stage call of every kind between two identical engine.elbo calls: identical bits."""
    X, Y, p = make_problem(2000, 96, 3, seed=7)
    engine.set_data(X, Y)
    first = engine.elbo(p, jitter=1e-6)
    _run_forward(engine, 200, 136, 1024, 1, 'int')
    _run_forward(engine, 9, 9, 1024, 0, 'int')
    _run_syrk(engine, 256, [1024], 'int')
    a = _kgrad_operands(5, 2, 1024, 1024, 'int')
    engine.test_kgrad(*a[:5], a[5], a[6], centre=np.ones(2), exact=False)
    second = engine.elbo(p, jitter=1e-6)
    assert first[0] == second[0] and first[1] == second[1]
    for k in first[2]:
        assert np.array_equal(np.asarray(first[2][k]), np.asarray(second[2][k])), k


def test_stage_entry_points_validate_their_arguments(engine):
    from zigp import _lib
    lib = engine.lib
    assert lib.zigp_test_chunk_forward(None, 1024, 0, -1, None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_pointwise(None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kgrad(None, 1, 1, 1024, 1, 0, *([None] * 9), 0, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_rank_update(None, 1, 1, None, None, None, None, None) == _lib.ZIGP_EARG
    q = _latent_operands(9, 1024, 'int', 0, 0)
    with pytest.raises(ValueError):
        engine.test_chunk_forward(dict(q, K=q['K'][:, :1000]), q, 1000, 0)          # not a multiple of 1024
    with pytest.raises(ValueError):
        engine.test_rank_update([(np.zeros((4, 1000)), np.zeros(1000))])
    with pytest.raises(ValueError):
        a = _kgrad_operands(3, 2, 1024, 1024, 'int')
        engine.test_kgrad(*a[:5], a[5], a[6], n0=5000)
    with pytest.raises(ValueError):
        engine.test_pointwise('value', np.zeros((3, 2, 1024)), np.zeros((3, 2, 1024)), (3, 1), (1, 1), np.zeros((10, 1)), np.zeros(10), 0, 10, 1, 1, 1)
