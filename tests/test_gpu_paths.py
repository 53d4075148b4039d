"""GPU tests of the sample paths (include/zigp.h "sample paths"; csrc/zigp_paths.hip): the path kernel against the 50-digit sum under the
point-wise rule, the bit-equal tiers, zigp_sample_paths against zigp_predict (eps = 0, a = 0) and against its NumPy restatement (real
draws) under the predict bound, the refusals, and the model surface.  Every measured figure is printed (the PATHS- lines of a run are
profiles/paths_parity.log)."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem, relerr
import paths_ref as pr
import matern_ref as mr
import fullcov_ref as fr

pytestmark = pytest.mark.gpu
EPS = pr.EPS


def _latent(rs, kind, M, R, D, S, ell=None, var=1.0, xscale=1.0, lin=False, shift=0.0, zero=False):
    ell = (0.4 + 0.1 * np.arange(D)) * xscale if ell is None else ell
    q = dict(kind=kind, Z=rs.rand(M, D) * xscale, ell=ell, var=var, V=rs.randn(M, S), omega=rs.randn(R, D) / ell, phase=rs.uniform(0, 2 * np.pi, R),
             amp=rs.randn(R, S) * np.sqrt(2.0 * var / max(R, 1)), shift=shift)
    if lin:
        q['lin'] = rs.randn(D)
    if zero:
        q['V'], q['amp'] = np.zeros((M, S)), np.zeros((R, S))
    return q


def _case(name):
    """(latents, X, S): the smallest shapes that reach every tail -- M in {1, 5, 50, 137}, R in {0, 1, 7, 64, 200}, S in {1, 3, 16, 17, 40},
    D in {1, 3, 8}, N in {1, 15, 16, 17, 63, 65, 300}, the three kinds, one latent and pairs with different M, R and kind; S = 64 on top: the
    one-, two- and four-tile passes of the kernel all run (S <= 16; 17 and 40; 64)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == 'one_point':             # one inducing point, no features, one sample, one row
        return [_latent(rs, 'rbf', 1, 0, 1, 1)], rs.rand(1, 1), 1
    if name == 'pair_d3_s3':
        return [_latent(rs, 'rbf', 5, 1, 3, 3), _latent(rs, 'matern32', 50, 7, 3, 3, var=5.0)], rs.rand(15, 3), 3
    if name == 'pair_d8_s16':
        return [_latent(rs, 'matern52', 137, 64, 8, 16), _latent(rs, 'rbf', 1, 200, 8, 16, var=2.0)], rs.rand(16, 8), 16
    if name == 'mean_part_s17':         # lin and shift on f, a conditional-mean-only g (R = 0)
        return [_latent(rs, 'matern32', 5, 200, 3, 17, lin=True, shift=-0.7), _latent(rs, 'matern52', 50, 0, 3, 17, shift=-1.0)], rs.rand(17, 3), 17
    if name == 'large_arguments':       # inputs in [0, 1e4] and frequencies of 100: cosine arguments up to 1e6
        f = _latent(rs, 'rbf', 137, 7, 1, 40, xscale=1e4)
        g = _latent(rs, 'matern32', 5, 64, 1, 40, xscale=1e4)
        f['omega'], g['omega'] = rs.uniform(-100, 100, (7, 1)), rs.uniform(-100, 100, (64, 1))
        X = rs.rand(63, 1) * 1e4
        X[0] = 1e4
        g['omega'][0] = 100.0
        return [f, g], X, 40
    if name == 'near_half_pi':          # phases set so that rows land on odd and even multiples of pi / 2 to the last bit of the argument
        f, g = _latent(rs, 'matern52', 50, 64, 3, 40), _latent(rs, 'rbf', 5, 64, 3, 40)
        X = rs.rand(65, 3)
        for q in (f, g):
            for r in range(0, 64, 4):
                n = (7 * r) % 65
                q['phase'][r] = (r // 4 + 1) * (np.pi / 2) - float(X[n] @ q['omega'][r])
        return [f, g], X, 40
    if name == 'zero_weights':          # V = 0 and amp = 0: the mean part alone, 300 rows (three blocks, the last partial)
        return [_latent(rs, 'rbf', 50, 64, 8, 3, lin=True, shift=0.3, zero=True), _latent(rs, 'matern52', 137, 1, 8, 3)], rs.rand(300, 8), 3
    if name == 'four_tiles_d8':         # 64 samples: four sample tiles in one pass, at the widest D (the largest register footprint)
        return [_latent(rs, 'matern32', 5, 7, 8, 64, lin=True), _latent(rs, 'rbf', 1, 1, 8, 64)], rs.rand(17, 8), 64
    raise KeyError(name)


CASES = ['one_point', 'pair_d3_s3', 'pair_d8_s16', 'mean_part_s17', 'large_arguments', 'near_half_pi', 'zero_weights', 'four_tiles_d8']


@pytest.mark.parametrize('name', CASES)
def test_path_rows_against_the_50_digit_sum(engine, name):
    """err_gpu <= 4 err_np + 16 eps S at every checked element, S the magnitude of paths_ref.path_sum_np; up to 16 rows x 6 samples per
    latent carry the 50-digit value (the ends and the 16-row tile boundaries first), and every element is finite"""
    lats, X, S = _case(name)
    out = engine.path_rows(lats, X, S)
    assert out.shape == (len(lats), S, X.shape[0]) and np.all(np.isfinite(out))
    rows, cols = pr.pick(X.shape[0], 16), pr.pick(S, 6)
    worst = 0.0
    for h, q in enumerate(lats):
        ref_np, mag = pr.path_sum_np(q, X)
        exact = pr.path_sum_mp(q, X, rows, cols)
        sel = np.ix_(cols, rows)
        err_gpu, err_np = np.abs(out[h][sel] - exact), np.abs(ref_np[sel] - exact)
        ratio = float(np.max(err_gpu / np.maximum(EPS * mag[sel], 1e-300)))
        worst = max(worst, ratio)
        line = 'PATHS-PARITY %s latent %d (%s M=%d R=%d D=%d S=%d N=%d): max err_gpu / (eps S) %.2f, err_np / (eps S) %.2f' % (
            name, h, q['kind'], q['Z'].shape[0], q['phase'].size, X.shape[1], S, X.shape[0], ratio,
            float(np.max(err_np / np.maximum(EPS * mag[sel], 1e-300))))
        print(line)
        assert np.all(err_gpu <= 4 * err_np + 16 * EPS * mag[sel]), line
    if name == 'zero_weights':          # the mean part alone: shift + sum_d lin_d x_d in ascending d with fused multiply-adds, nothing else
        want = np.full(X.shape[0], lats[0]['shift'])
        assert np.all(np.abs(out[0] - (want + X @ lats[0]['lin'])[None, :]) <= 16 * EPS * pr.path_sum_np(lats[0], X)[1])
        assert np.all(out[0] == out[0][0][None, :])


def test_bit_equal_tiers(engine):
    """A repeated call returns the same bits; row n alone equals row n inside any batch; column s alone equals column s of a 40-sample
    call; one latent alone equals the same latent in a pair; the host call equals the device call; the device call leaves the elements
    of a larger sentinel-filled tensor outside the (nlat, S, N) view untouched"""
    import torch
    rs = np.random.RandomState(11)
    D, S, N = 3, 40, 300
    f, g = _latent(rs, 'matern32', 50, 64, D, S, lin=True, shift=0.2), _latent(rs, 'rbf', 137, 7, D, S, var=3.0)
    X = rs.rand(N, D)
    a = engine.path_rows([f, g], X, S)
    assert np.array_equal(a, engine.path_rows([f, g], X, S))
    for n in (0, 15, 16, 17, 127, 128, 299):
        assert np.array_equal(engine.path_rows([f, g], X[n:n + 1], S)[:, :, 0], a[:, :, n]), n
    assert np.array_equal(engine.path_rows([f, g], X[37:102], S), a[:, :, 37:102])
    for s in (0, 15, 16, 17, 39):
        one = [dict(q, V=np.ascontiguousarray(q['V'][:, s:s + 1]), amp=np.ascontiguousarray(q['amp'][:, s:s + 1])) for q in (f, g)]
        assert np.array_equal(engine.path_rows(one, X, 1)[:, 0, :], a[:, s, :]), s
    first17 = [dict(q, V=np.ascontiguousarray(q['V'][:, :17]), amp=np.ascontiguousarray(q['amp'][:, :17])) for q in (f, g)]
    assert np.array_equal(engine.path_rows(first17, X, 17), a[:, :17, :])
    assert np.array_equal(engine.path_rows([f], X, S)[0], a[0]) and np.array_equal(engine.path_rows([g], X, S)[0], a[1])
    assert np.array_equal(engine.path_rows([g, f], X, S), a[::-1])
    Xt = torch.from_numpy(X).cuda()
    assert np.array_equal(engine.path_rows_device([f, g], Xt, S).cpu().numpy(), a)
    big = torch.full((2 * S * N + 999,), 7.25, dtype=torch.float64, device='cuda')
    engine.path_rows_device([f, g], Xt, S, out=big)
    big = big.cpu().numpy()
    assert np.array_equal(big[:2 * S * N].reshape(2, S, N), a) and np.all(big[2 * S * N:] == 7.25)


def _cond(p, jitter=1e-6):
    return max(float(np.linalg.cond(pr.kern_np(p.get('kern_' + t, 'rbf'), p['Z' + t], p['Z' + t], p['ell_' + t], float(p['var_' + t])) + jitter * np.eye(p['Z' + t].shape[0])))
               for t in 'fg')


def _bound(c):
    return min(max(1e-9, 1e-13 * c), 1e-6)


def _draws(p, R, S, seed):
    from zigp import pathwise
    rs = np.random.RandomState(seed)
    return {t: pathwise.draw(p.get('kern_' + t, 'rbf'), R, p['Zf'].shape[1], p['Z' + t].shape[0], S, rs) for t in 'fg'}


def _mode(p, mode):
    if mode == 'white':
        return dict(p, whiten=True)
    if mode == 'white_full':
        return fr.make_lq(p, seed=3, negative=2)
    return dict(p)


MEAN_CASES = [('diag', {}, {}), ('white', dict(kern_f='matern32'), dict(mean_b=0.4)), ('white_full', dict(kern_g='matern52'), dict(mean_a=True, mean_b=-0.2)),
              ('diag', dict(kern_f='matern52', kern_g='matern32'), dict(mean_a=True))]


@pytest.mark.parametrize('mode,kinds,mean', MEAN_CASES, ids=lambda v: v if isinstance(v, str) else '_'.join(sorted(v)) or 'plain')
def test_sample_paths_collapse_onto_predict(engine, mode, kinds, mean):
    """eps = 0 and a = 0: every sample equals rows 3 and 5 (fmean, gmean) of engine.predict on the same inputs, under the predict bound
    min(max(1e-9, 1e-13 cond(Kuu)), 1e-6) normalised by the row's largest entry -- the three parametrisations, a Matern latent, a
    Constant and a Linear mean function, g_offset = -1; and gf = Phi~(g) f of the returned planes under the point-wise rule"""
    X, Y, p = mr.problem(1500, 50, 37, 3)
    X = X[:300]
    p = dict(_mode(p, mode), **kinds)
    if mean.get('mean_a'):
        p['mean_a'] = np.array([0.3, -0.2, 0.1])
    if 'mean_b' in mean:
        p['mean_b'] = mean['mean_b']
    c, S = _cond(p), 17
    draws = pr.zero_draws(_draws(p, 64, S, 5))
    for g_off in (0.0, -1.0):
        r = engine.sample_paths(p, X, n_samples=S, draws=draws, jitter=1e-6, g_offset=g_off)
        out = engine.predict(p, X, jitter=1e-6, g_offset=g_off)
        ef, eg = relerr(r['f'], np.tile(out[3], (S, 1))), relerr(r['g'], np.tile(out[5], (S, 1)))
        print('PATHS-MEAN %s %s %s g_offset %+.0f: cond(Kuu) %.2e f relerr %.2e g relerr %.2e (bound %.1e)' % (mode, kinds, sorted(mean), g_off, c, ef, eg, _bound(c)))
        assert ef < _bound(c) and eg < _bound(c)
        assert all(np.array_equal(r[k][s], r[k][0]) for k in ('f', 'g') for s in range(S))
        idx = np.unravel_index(np.linspace(0, S * X.shape[0] - 1, 60).astype(int), (S, X.shape[0]))
        fs, gs = r['f'][idx], r['g'][idx]
        exact = pr.link_times_mp(gs, fs)
        err_gpu, err_np = np.abs(r['gf'][idx] - exact), np.abs(pr.link(gs) * fs - exact)
        assert np.all(err_gpu <= 4 * err_np + 16 * EPS * np.abs(exact) * (1 + np.abs(gs)))


DRAW_CASES = [((1500, 50, 37, 3), 'diag'), ((1500, 50, 37, 3), 'white'), ((1500, 50, 37, 3), 'white_full'), ((700, 137, 137, 1), 'diag'),
              ((700, 137, 137, 1), 'white')]


@pytest.mark.parametrize('shape,mode', DRAW_CASES, ids=lambda v: v if isinstance(v, str) else 'N%d_M%d_%d_D%d' % v)
def test_sample_paths_against_the_numpy_restatement(engine, shape, mode):
    """Real draws, host and device call, against paths_ref.sample_paths_np (Cholesky and triangular solves) under the predict bound,
    normalised per plane: the Matern tests' well-conditioned fixture (1500, 50 / 37, 3) in all three parametrisations and their
    ill-conditioned one (700, 137, 1); cond(Kuu) is printed"""
    import torch
    X, Y, p = mr.problem(*shape)
    X = X[::5]
    p = dict(_mode(p, mode), kern_f='matern52' if shape[3] == 3 else 'rbf', mean_b=0.1)
    c, S = _cond(p), 20
    draws = _draws(p, 200, S, 9)
    r = engine.sample_paths(p, X, n_samples=S, draws=draws, jitter=1e-6, g_offset=-1.0)
    ref = pr.sample_paths_np(p, X, draws, 1e-6, -1.0)
    e = {k: relerr(r[k], ref[k]) for k in ('f', 'g', 'gf')}
    line = 'PATHS-DRAWS %s N=%d M=%d/%d D=%d: cond(Kuu) %.2e relerr f %.2e g %.2e gf %.2e (bound %.1e)' % ((mode, X.shape[0]) + shape[1:] + (c, e['f'], e['g'], e['gf'], _bound(c)))
    print(line)
    d = engine.sample_paths_device(p, torch.from_numpy(X).cuda(), n_samples=S, draws=draws, jitter=1e-6, g_offset=-1.0)
    assert all(np.array_equal(d[k].cpu().numpy(), r[k]) for k in ('f', 'g', 'gf'))
    assert np.std(r['f'], 0).max() > 1e-3 and np.std(r['g'], 0).max() > 1e-3          # the draws do move the paths
    assert all(v < _bound(c) for v in e.values()), line


def test_same_draws_other_inputs(engine):
    """the draws handed back give the same paths: a subset of the rows returns the subset of the bits"""
    X, Y, p = make_problem(200, 20, 2, seed=3, Mg=9)
    r = engine.sample_paths(p, X, n_samples=5, n_features=33, rng=4)
    assert r['f'].shape == (5, 200) and r['draws']['f']['R'] == 33
    q = engine.sample_paths(p, X[50:70], n_samples=5, draws=r['draws'])
    assert all(np.array_equal(q[k], r[k][:, 50:70]) for k in ('f', 'g', 'gf'))
    z = engine.sample_paths(p, X, n_samples=5, n_features=0, rng=4)                      # R = 0: the conditional-mean part and eps alone
    assert np.all(np.isfinite(z['f']))


def test_refusals_leave_the_context_usable(engine):
    """every refusal of the C entry points is a ValueError that names the argument; after each, a good call returns the earlier bits"""
    from zigp.engine import _check, _Packed
    from zigp import _lib
    rs = np.random.RandomState(2)
    D, S, N = 2, 3, 20
    q = _latent(rs, 'rbf', 6, 8, D, S)
    X = rs.rand(N, D)
    good = engine.path_rows([q], X, S)
    lib, ctx = engine.lib, engine.ctx
    out = np.full((1, S, N), 3.5)

    def raw(recs, D_=D, S_=S, X_=X, fn='zigp_path_rows'):
        _check(lib, ctx, getattr(lib, fn)(ctx, C.cast(recs, C.c_void_p), 1, D_, S_, X_.ctypes.data, N, out.ctypes.data))

    def after(match, call):
        with pytest.raises(ValueError, match=match):
            call()
        assert np.all(out == 3.5)
        assert np.array_equal(engine.path_rows([q], X, S), good)

    recs, keep = engine._path_latents([q], D, S)
    after('D = 9', lambda: raw(recs, D_=9))
    after('S = 0', lambda: raw(recs, S_=0))
    after('S = 257', lambda: raw(recs, S_=257))
    for field in ('V', 'Z', 'ell', 'omega', 'phase', 'amp'):
        recs, keep = engine._path_latents([q], D, S)
        setattr(recs[0], field, None)
        after(field + ' is NULL', lambda: raw(recs))
    recs, keep = engine._path_latents([q], D, S)
    recs[0].R = -1
    after('R is negative', lambda: raw(recs))
    for field, bad in (('V', np.inf), ('amp', np.nan), ('omega', -np.inf), ('phase', np.nan), ('Z', np.nan), ('lin', np.inf)):
        arr = np.array(q[field] if field != 'lin' else np.zeros(D), dtype=np.float64)
        arr.reshape(-1)[-1] = bad
        after(field + ' has a non-finite entry', lambda: engine.path_rows([dict(q, **{field: arr})], X, S))
    recs, keep = engine._path_latents([q], D, S)
    after('device memory', lambda: raw(recs, fn='zigp_path_rows_device'))
    # zigp_sample_paths: the same refusals through the model call
    Xp, Y, p = make_problem(N, 6, D, seed=1, Mg=4)
    draws = _draws(p, 8, S, 0)
    goodp = engine.sample_paths(p, Xp, n_samples=S, draws=draws)
    pk = _Packed(p)
    dr, rec2, keep2 = engine._path_draws(pk, pk.kinds, S, 8, None, draws)
    out3 = np.full((3, S, N), 3.5)

    def rawp(S_=S, fn='zigp_sample_paths', rf=None, rg=None):
        rf, rg = rf or rec2[0], rg or rec2[1]
        _check(lib, ctx, getattr(lib, fn)(ctx, C.byref(pk.struct), Xp.ctypes.data, N, 1e-6, 0.0, C.addressof(rf), C.addressof(rg), S_, out3.ctypes.data))

    def afterp(match, call):
        with pytest.raises(ValueError, match=match):
            call()
        assert np.all(out3 == 3.5)
        r = engine.sample_paths(p, Xp, n_samples=S, draws=draws)
        assert all(np.array_equal(r[k], goodp[k]) for k in ('f', 'g', 'gf'))

    afterp('S = 0', lambda: rawp(S_=0))
    afterp('S = 300', lambda: rawp(S_=300))
    afterp('device memory', lambda: rawp(fn='zigp_sample_paths_device'))
    for field in ('omega0', 'phase', 'a', 'eps'):
        bad = _lib.zigp_path_draw()
        C.memmove(C.addressof(bad), C.addressof(rec2[1]), C.sizeof(bad))
        setattr(bad, field, None)
        afterp(r'draw_g\.%s is NULL' % field, lambda: rawp(rg=bad))
    neg = _lib.zigp_path_draw()
    C.memmove(C.addressof(neg), C.addressof(rec2[0]), C.sizeof(neg))
    neg.R = -2
    afterp('draw_f: R is negative', lambda: rawp(rf=neg))
    nf = dict(draws, f=dict(draws['f'], eps=np.where(np.arange(6 * S).reshape(6, S) == 4, np.nan, draws['f']['eps'])))
    afterp(r'draw_f\.eps has a non-finite entry', lambda: engine.sample_paths(p, Xp, n_samples=S, draws=nf))
    X9, Y9, p9 = make_problem(N, 6, 9, seed=1)
    pk9 = _Packed(p9)
    d9 = {t: dict(R=0, omega0=np.zeros((0, 9)), phase=np.zeros(0), a=np.zeros((0, S)), eps=np.zeros((6, S))) for t in 'fg'}
    r9 = []
    for t in 'fg':
        rec = _lib.zigp_path_draw()
        rec.R, rec.eps = 0, d9[t]['eps'].ctypes.data
        r9.append(rec)
    engine._set_modes(p9)
    with pytest.raises(ValueError, match='D = 9'):
        _check(lib, ctx, lib.zigp_sample_paths(ctx, C.byref(pk9.struct), X9.ctypes.data, N, 1e-6, 0.0, C.addressof(r9[0]), C.addressof(r9[1]), S, out3.ctypes.data))
    assert np.all(out3 == 3.5)
    r = engine.sample_paths(p, Xp, n_samples=S, draws=draws)
    assert all(np.array_equal(r[k], goodp[k]) for k in ('f', 'g', 'gf'))


def test_model_surface():
    """predict_onoffgp_samples: shapes (num_samples, N, 1); the same seed gives the same arrays; over 256 samples on the toy data each
    row's sample mean of f lies within 6 standard errors (taken from the samples) of predict_onoffgp's fmean -- deterministic at the
    fixed seed: it guards the wiring, not the approximation"""
    from test_gpu_model import _toy_model
    m, X, Y = _toy_model()
    f, g, gf = m.predict_onoffgp_samples(X, 256, n_features=256, seed=12)
    N = X.shape[0]
    assert f.shape == g.shape == gf.shape == (256, N, 1)
    f2, g2, gf2 = m.predict_onoffgp_samples(X, 256, n_features=256, seed=12)
    assert np.array_equal(f, f2) and np.array_equal(g, g2) and np.array_equal(gf, gf2)
    f3 = m.predict_onoffgp_samples(X[:7], 4, n_features=16, seed=13)[0]
    assert f3.shape == (4, 7, 1) and not np.array_equal(f3[0], f3[1])
    fmean = m.predict_onoffgp(X)[3].reshape(-1)
    mean, se = f[:, :, 0].mean(0), f[:, :, 0].std(0, ddof=1) / np.sqrt(256.0)
    z = np.abs(mean - fmean) / se
    print('PATHS-MODEL toy data: largest |sample mean - fmean| / standard error %.2f over %d rows (256 samples)' % (z.max(), N))
    assert np.all(se > 0) and z.max() <= 6.0
