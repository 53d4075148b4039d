"""GPU tests of the Kronecker sample paths (include/zigp_kronpaths.h): the kernel against a
50-digit evaluation of its sum under the project's point-wise rule, the bit-equal tiers, the existing path kernel on the expanded
grid, and the model calls (OnOff and both heads) against zigp_kron_predict and the NumPy restatement of tests/kronpaths_ref.py."""
import numpy as np
import pytest

import kron_nd
import kronpaths_ref as kr
import paths_ref as pr
from zigp import NotPositiveDefiniteError

pytestmark = pytest.mark.gpu


def _case(grids, dims, R, S, N, zero=False, far=False, n_rows=8, n_cols=8):
    return dict(grids=grids, dims=dims, R=R if isinstance(R, tuple) else (R,) * len(grids), S=S, N=N, zero=zero, far=far, n_rows=n_rows, n_cols=n_cols)


# Every grid, R, S, (D0, D1) and N of the issue's list appears at least once: 3 x 7 has an M1 that is no multiple of 4; S = 1 .. 16 is
# one sample tile a pass, 17 two, 40 two (three tiles, padded to four), 64 four; N = 300 fills more than one block at every block size (128, 64 and 32 rows).
KERNEL_CASES = {
    '1x1': _case([(1, 1)], (1, 1), 0, 1, 1),
    '1x5': _case([(1, 5)], (2, 1), 1, 3, 15),
    '5x1': _case([(5, 1)], (1, 2), 7, 16, 16),
    '3x7': _case([(3, 7)], (4, 4), 64, 17, 17),
    '10x12': _case([(10, 12)], (7, 1), 7, 40, 127),
    '32x32': _case([(32, 32)], (1, 7), 64, 64, 129),
    '16x112': _case([(16, 112)], (2, 1), 1, 17, 300, n_rows=6, n_cols=5),
    '10x100-S64': _case([(10, 100)], (2, 1), 7, 64, 129, n_rows=6, n_cols=6),      # one row tile a wave with four sample tiles a pass
    '16x112-S49': _case([(16, 112)], (4, 4), 1, 49, 65, n_rows=5, n_cols=5),       # the same pair at D = 8 and the fewest samples that have four tiles
    '128x128': _case([(128, 128)], (2, 1), 0, 3, 17, n_rows=4, n_cols=3),          # 12 elements: 16 384 terms each at 50 digits
    'pair-3x7-10x12': _case([(3, 7), (10, 12)], (2, 1), (7, 64), 40, 129),
    'pair-32x32-5x1': _case([(32, 32), (5, 1)], (1, 2), (0, 7), 16, 300, n_rows=6, n_cols=5),
    'zero-weights': _case([(10, 12)], (2, 1), 7, 3, 17, zero=True),
    'far-rows': _case([(10, 12)], (2, 1), 1, 16, 17, far=True),
}


def _kernel_problem(name):
    k = KERNEL_CASES[name]
    rs = np.random.RandomState(7000 + list(KERNEL_CASES).index(name))
    D0, D1 = k['dims']
    lats = [kr.random_latent(rs, g[0], g[1], D0, D1, R, k['S'], zero=k['zero'], shift=0.3 - h) for h, (g, R) in enumerate(zip(k['grids'], k['R']))]
    X = rs.rand(k['N'], D0 + D1)
    if k['far']:
        # rows 0 .. 5: each exponent about -400, so k0 and k1 are normal and k0 k1 underflows; rows 6 .. 9: factor 0 alone goes
        # subnormal (exponent about -730: the element function's own branch); the others stay near the grid
        e0, e1 = lats[0]['ell']
        X[0:6, :D0] = 1.0 + e0 * np.sqrt(800.0 / D0) * (1 + 0.01 * rs.rand(6, D0))
        X[0:6, D0:] = 1.0 + e1 * np.sqrt(800.0 / D1) * (1 + 0.01 * rs.rand(6, D1))
        X[6:10, :D0] = 1.0 + e0 * np.sqrt(1460.0 / D0) * (1 + 0.004 * rs.rand(4, D0))
    return k, lats, X


@pytest.mark.parametrize('name', list(KERNEL_CASES))
def test_kernel_against_50_digits(engine, name):
    """zigp_kron_path_rows under the point-wise rule err_gpu <= 4 err_np + 16 eps S at about 60 sampled elements per latent (12 at the
    largest grid): S = sum |term| (1 + |argument|), the argument of a grid term |a0| + |a1|."""
    k, lats, X = _kernel_problem(name)
    out = engine.kron_path_rows(lats, X, k['S'], k['dims'])
    assert out.shape == (len(lats), k['S'], k['N']) and np.all(np.isfinite(out))
    rows = list(range(10)) if k['far'] else pr.pick(k['N'], k['n_rows'])
    cols = pr.pick(k['S'], k['n_cols'])
    for h, lat in enumerate(lats):
        ref_np, mag = kr.kron_path_sum_np(lat, X)
        ref_mp = kr.kron_path_sum_mp(lat, X, rows, cols)
        ix = np.ix_(cols, rows)
        ratio, excess = kr.pointwise_ratio(out[h][ix], ref_np[ix], ref_mp, mag[ix])
        print('%s latent %d: %d elements, largest err_gpu / (eps S) = %.3f' % (name, h, len(rows) * len(cols), ratio))
        assert excess <= 0.0
        # away from the sampled elements there is no 50-digit value: the whole block against NumPy, with the rule's 16 eps S for the
        # kernel and n eps S for NumPy's own sum of n terms (its worst case) -- wide, but a wrong row, tile or column is O(1) away
        n_terms = k['grids'][h][0] * k['grids'][h][1] + k['R'][h] + 8
        assert np.all(np.abs(out[h] - ref_np) <= (16 + n_terms) * kr.EPS * mag)
    if k['far']:
        k0 = kr.factor_np(X[:6, :2], lats[0]['Z'][0], lats[0]['ell'][0], lats[0]['var'][0])[0]
        k1 = kr.factor_np(X[:6, 2:], lats[0]['Z'][1], lats[0]['ell'][1], lats[0]['var'][1])[0]
        assert np.all(k0 > 1e-300) and np.all(k1 > 1e-300) and np.all(k0.max(1) * k1.max(1) < 1e-320)       # the product underflows, not the factors


def test_bit_equal_tiers(engine, monkeypatch):
    """The same element at another N and row position, another S and sample column, one, two and four sample tiles a pass, with and
    without a second latent (in either slot; one that changes the row tiles a wave holds), from host and from device memory: the same
    bits.  S = 64 is four sample tiles, so the caps 1, 2 and 4 run NST = 1, 2 and 4; the 10 x 12 grid runs two row tiles a wave and the
    10 x 100 grid one, each under every cap."""
    import torch
    rs = np.random.RandomState(77)
    S, N, dims = 64, 300, (2, 1)
    lat, other = kr.random_latent(rs, 10, 12, 2, 1, 7, S), kr.random_latent(rs, 3, 7, 2, 1, 64, S)
    big = kr.random_latent(rs, 10, 100, 2, 1, 5, S)              # a grid that takes a launch to one row tile a wave
    X = rs.rand(N, 3)
    base = engine.kron_path_rows([lat], X, S, dims)[0]
    base_big = engine.kron_path_rows([big], X, S, dims)[0]
    sub = engine.kron_path_rows([lat], X[37:166], S, dims)[0]                       # another N, every row at another position
    assert np.array_equal(sub, base[:, 37:166])
    one = engine.kron_path_rows([lat], X[299:300], S, dims)[0]
    assert np.array_equal(one, base[:, 299:300])
    assert np.array_equal(engine.kron_path_rows([big], X[37:166], S, dims)[0], base_big[:, 37:166])
    cols = [33, 5, 63]                                                              # another S (one tile a pass), other columns
    few = engine.kron_path_rows([dict(lat, V=lat['V'][:, cols], amp=lat['amp'][:, cols])], X, 3, dims)[0]
    assert np.array_equal(few, base[cols])
    few_big = engine.kron_path_rows([dict(big, V=big['V'][:, cols], amp=big['amp'][:, cols])], X, 3, dims)[0]
    assert np.array_equal(few_big, base_big[cols])
    half = list(range(20, 60))                                                      # 40 samples: three tiles, two a pass
    mid = engine.kron_path_rows([dict(big, V=big['V'][:, half], amp=big['amp'][:, half])], X, 40, dims)[0]
    assert np.array_equal(mid, base_big[half])
    for cap in ('1', '2', '4'):
        monkeypatch.setenv('ZIGP_PATH_TILES', cap)
        assert np.array_equal(engine.kron_path_rows([lat], X, S, dims)[0], base), cap
        assert np.array_equal(engine.kron_path_rows([big], X, S, dims)[0], base_big), cap
    monkeypatch.delenv('ZIGP_PATH_TILES')
    two = engine.kron_path_rows([lat, other], X, S, dims)
    assert np.array_equal(two[0], base)
    swapped = engine.kron_path_rows([other, lat], X, S, dims)
    assert np.array_equal(swapped[1], base) and np.array_equal(swapped[0], two[1])
    dev = engine.kron_path_rows_device([lat, other], torch.from_numpy(X).cuda(), S, dims)
    assert np.array_equal(dev.cpu().numpy(), two)
    mixed = engine.kron_path_rows([lat, big], X, S, dims)                           # lat now runs one row tile a wave
    assert np.array_equal(mixed[0], base) and np.array_equal(mixed[1], base_big)


def test_rows_on_grid_points_with_dyadic_weights_equal_numpy_bits(engine):
    """Column s has the dyadic weight 2^-s at one grid point (i_s, j_s) and zero weights elsewhere; row s sits on that grid point.  There
    k0 = var0 and k1 = var1 exactly (exp(0) = 1), every other term is an exact zero, so out[s][s] = fl(var0 var1) 2^-s bit for bit."""
    rs = np.random.RandomState(3)
    M0, M1, S = 5, 7, 20
    lat = kr.random_latent(rs, M0, M1, 2, 1, 0, S, zero=True, shift=0.0)
    pts = [(int(rs.randint(M0)), int(rs.randint(M1))) for _ in range(S)]
    V = np.zeros((M0 * M1, S))
    X = np.zeros((S, 3))
    for s, (i, j) in enumerate(pts):
        V[i * M1 + j, s] = (-1.0) ** s * 2.0 ** -s
        X[s] = np.concatenate([lat['Z'][0][i], lat['Z'][1][j]])
    lat['V'] = V
    out = engine.kron_path_rows([lat], X, S, (2, 1))[0]
    want = np.array([(lat['var'][0] * lat['var'][1]) * V[i * M1 + j, s] for s, (i, j) in enumerate(pts)])
    assert np.array_equal(np.diagonal(out), want)
    ref, mag = kr.kron_path_sum_np(lat, X)
    assert np.all(np.abs(out - ref) <= (16 + M0 * M1) * kr.EPS * mag)      # off the diagonal: one inexact term, NumPy's sum of M0 M1


@pytest.mark.parametrize('grid,dims,R', [((3, 7), (2, 1), 7), ((10, 12), (4, 4), 64), ((32, 32), (1, 2), 0)])
def test_against_the_existing_kernel_on_the_expanded_grid(engine, grid, dims, R):
    """kron_path_rows against path_rows over the M0 M1 grid points with var0 var1: two kernels, one sum -- the difference is within the
    sum of the two point-wise bounds at the sampled elements (each kernel's 4 err_np + 16 eps S against 50 digits)."""
    rs = np.random.RandomState(91)
    S, N = 17, 129
    lat = kr.random_latent(rs, grid[0], grid[1], dims[0], dims[1], R, S)
    X = rs.rand(N, dims[0] + dims[1])
    a = engine.kron_path_rows([lat], X, S, dims)[0]
    dense = kr.expand(lat)
    b = engine.path_rows([dense], X, S)[0]
    rows, cols = pr.pick(N, 6), pr.pick(S, 5)
    ix = np.ix_(cols, rows)
    np_k, mag_k = kr.kron_path_sum_np(lat, X)
    np_d, mag_d = pr.path_sum_np(dense, X)
    mp_k, mp_d = kr.kron_path_sum_mp(lat, X, rows, cols), pr.path_sum_mp(dense, X, rows, cols)
    bound = 4 * np.abs(np_k[ix] - mp_k) + 16 * kr.EPS * mag_k[ix] + 4 * np.abs(np_d[ix] - mp_d) + 16 * kr.EPS * mag_d[ix]
    diff = np.abs(a[ix] - b[ix])
    print('%dx%d: largest difference / bound = %.3f' % (grid[0], grid[1], float(np.max(diff / bound))))
    assert np.all(diff <= bound)


# ---- the model calls ------------------------------------------------------------------------------------------------------------------
def _bound(name, tags=('f', 'g')):
    X, Y, p = kron_nd.problem(name)
    return kr.path_bound(p, tags, kr.MODEL_JITTER)


@pytest.mark.parametrize('name', kr.MODEL_CASES)
def test_zero_draws_equal_kron_predict(engine, name):
    """a = 0, eps = 0: every path is the posterior mean -- rows 3 and 5 of zigp_kron_predict, at g_offset 0 and -1 and with an f_mu"""
    X, Y, p = kron_nd.problem(name)
    z = pr.zero_draws(kr.model_draws(name))
    bound, c = _bound(name)
    for g_offset, f_mu in ((0.0, None), (-1.0, 0.7)):
        got = engine.kron_sample_paths(p, X, n_samples=kr.MODEL_S, draws=z, jitter=kr.MODEL_JITTER, g_offset=g_offset, f_mu=f_mu)
        ref = engine.kron_predict(p, X, jitter=kr.MODEL_JITTER, g_offset=g_offset, f_mu=f_mu)
        ef = max(kr.plane_err(got['f'][s], ref[3]) for s in range(kr.MODEL_S))
        eg = max(kr.plane_err(got['g'][s], ref[5]) for s in range(kr.MODEL_S))
        print('%s g_offset %g: cond product %.2e, bound %.2e, f %.2e, g %.2e' % (name, g_offset, c, bound, ef, eg))
        assert ef <= bound and eg <= bound
        assert np.array_equal(got['f'][0], got['f'][-1])


@pytest.mark.parametrize('name', kr.MODEL_CASES)
def test_real_draws_match_the_restatement(engine, name):
    """R = 200, S = 20: f, g and gf against kron_sample_paths_np, each plane normalised by its largest entry, under the path bound; the
    host and the device call agree bit for bit; the draws move the paths; the paths of a slice of X are the slice of the paths."""
    import torch
    X, Y, p = kron_nd.problem(name)
    d = kr.model_draws(name)
    ref = kr.model_ref(name, -1.0, 0.25)
    bound, c = _bound(name)
    got = engine.kron_sample_paths(p, X, n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER, g_offset=-1.0, f_mu=0.25)
    errs = {k: kr.plane_err(got[k], ref[k]) for k in ('f', 'g', 'gf')}
    print('%s: cond product %.2e, bound %.2e, f %.2e, g %.2e, gf %.2e' % (name, c, bound, errs['f'], errs['g'], errs['gf']))
    assert max(errs.values()) <= bound
    dev = engine.kron_sample_paths_device(p, torch.from_numpy(np.array(X)).cuda(), n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER,
                                          g_offset=-1.0, f_mu=0.25)
    for k in ('f', 'g', 'gf'):
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k
    assert got['draws'] is d
    spread = np.std(got['f'], axis=0)
    assert np.min(spread) > 0 and not np.array_equal(got['f'][0], got['f'][1])
    part = engine.kron_sample_paths(p, X[40:171], n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER, g_offset=-1.0, f_mu=0.25)
    for k in ('f', 'g', 'gf'):
        assert np.array_equal(part[k], got[k][:, 40:171]), k


@pytest.mark.parametrize('name', kr.MODEL_CASES)
@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_heads_match_the_restatement(engine, name, lik):
    """Both heads against kron_head_sample_paths_np under the path bound; the Bernoulli probability plane under the point-wise rule
    against 50 digits from the call's own f (S: the link's two constants, and its erf term times 1 + |f|)."""
    import mpmath as mp
    import torch
    X, Y, p = kron_nd.problem(name)
    hp = kron_nd.head_params(p)
    d = kr.model_draws(name)['f']
    bound, c = _bound(name, ('f',))
    ref = kr.kron_head_sample_paths_np(hp, X, lik, d, kr.MODEL_JITTER, 0.4)
    got = engine.kron_head_sample_paths(hp, X, lik, n_samples=kr.MODEL_S, draws={'f': d}, jitter=kr.MODEL_JITTER, f_mu=0.4)
    err = kr.plane_err(got['f'], ref['f'])
    print('%s %s: bound %.2e, f %.2e' % (name, lik, bound, err))
    assert err <= bound
    assert ('p' in got) == (lik == 'bernoulli')
    if lik == 'bernoulli':
        assert kr.plane_err(got['p'], ref['p']) <= bound
        f = got['f'][::7, ::23]
        with mp.workdps(50):
            erf_mp = [[mp.erf(mp.mpf(float(v)) / mp.sqrt(2)) for v in row] for row in f]
            pm = np.array([[float((1 + e) / 2 * (1 - mp.mpf('2e-3')) + mp.mpf('1e-3')) for e in row] for row in erf_mp])
            erf_abs = np.array([[float(abs(e)) for e in row] for row in erf_mp])
        mag = 0.5 * (1 - 2e-3) + 1e-3 + 0.5 * (1 - 2e-3) * erf_abs * (1 + np.abs(f))      # the constants once, the erf term with its argument
        e_gpu, e_np = np.abs(got['p'][::7, ::23] - pm), np.abs(pr.link(f) - pm)
        print('%s probability plane: largest err / (eps S) = %.3f' % (name, float(np.max(e_gpu / (kr.EPS * mag)))))
        assert np.all(e_gpu <= 4 * e_np + 16 * kr.EPS * mag)
    dev = engine.kron_head_sample_paths_device(hp, torch.from_numpy(np.array(X)).cuda(), lik, n_samples=kr.MODEL_S, draws={'f': d},
                                               jitter=kr.MODEL_JITTER, f_mu=0.4)
    for k in ref:
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k


def test_refusals_leave_the_context_usable(engine):
    import ctypes as C
    import torch
    from zigp import _lib
    from zigp._lib import ptr
    rs = np.random.RandomState(1)
    S, dims = 4, (2, 1)
    lat = kr.random_latent(rs, 3, 5, 2, 1, 6, S)
    X = rs.rand(20, 3)
    good = engine.kron_path_rows([lat], X, S, dims)

    def raw(recs, nlat=1, D0=2, D1=1, S_=S, Xp=X, N=20, device=False):
        out = np.zeros((2, max(S_, 1), 20))
        fn = engine.lib.zigp_kron_path_rows_device if device else engine.lib.zigp_kron_path_rows
        rc = fn(engine.ctx, C.cast(recs, C.c_void_p), nlat, D0, D1, S_, ptr(Xp) if Xp is not None else None, N, ptr(out))
        return rc, engine.lib.zigp_last_error(engine.ctx).decode()

    def recs_of(**over):
        recs, keep = engine._kron_path_latents([lat], dims, S)
        for k, v in over.items():
            setattr(recs[0], k, v)
        return recs, keep

    bad_v = lat['V'].copy()
    bad_v[3, 1] = np.nan
    bad_om = lat['omega'].copy()
    bad_om[0, 0] = np.inf
    cases = [
        (dict(), dict(D0=0), 'D0'), (dict(), dict(D0=5, D1=4), 'D0 + D1'), (dict(), dict(S_=0), 'S ='), (dict(), dict(S_=257), 'S ='),
        (dict(M0=0), dict(), 'M0'), (dict(M0=129), dict(), 'M0'), (dict(M1=0), dict(), 'M1'), (dict(M1=200), dict(), 'M1'),
        (dict(R=-1), dict(), 'R is negative'), (dict(Z0=None), dict(), 'Z0 is NULL'), (dict(Z1=None), dict(), 'Z1 is NULL'),
        (dict(ell0=None), dict(), 'ell0 is NULL'), (dict(ell1=None), dict(), 'ell1 is NULL'), (dict(V=None), dict(), 'V is NULL'),
        (dict(omega=None), dict(), 'omega is NULL'), (dict(phase=None), dict(), 'phase is NULL'), (dict(amp=None), dict(), 'amp is NULL'),
        (dict(V=ptr(bad_v)), dict(), 'V has a non-finite'), (dict(omega=ptr(bad_om)), dict(), 'omega has a non-finite'),
        (dict(shift=float('nan')), dict(), 'shift'), (dict(var0=-1.0), dict(), 'var0'), (dict(), dict(nlat=3), 'nlat'),
        (dict(), dict(Xp=None), 'X or out'), (dict(), dict(N=-1), 'N is negative'), (dict(), dict(device=True), 'device memory'),
    ]
    for over, kw, word in cases:
        recs, keep = recs_of(**over)
        rc, msg = raw(recs, **kw)
        assert rc == _lib.ZIGP_EARG and word in msg and msg.startswith('zigp_kron_path_rows'), (over, kw, msg)
        assert np.array_equal(engine.kron_path_rows([lat], X, S, dims), good)
    # the model calls: a grid beyond 128, a draw of the wrong size is caught in Python, a non-finite draw in the library
    Xn, Y, p = kron_nd.problem('d21-12')
    d = kr.model_draws('d21-12')
    ok = engine.kron_sample_paths(p, Xn[:30], n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER)
    bad_a = d['f']['a'].copy()
    bad_a[1, 2] = np.nan
    with pytest.raises(ValueError, match='draw_f.a has a non-finite'):
        engine.kron_sample_paths(p, Xn[:30], n_samples=kr.MODEL_S, draws=dict(d, f=dict(d['f'], a=bad_a)), jitter=kr.MODEL_JITTER)
    with pytest.raises(ValueError, match='draw_g.eps must be'):
        engine.kron_sample_paths(p, Xn[:30], n_samples=kr.MODEL_S, draws=dict(d, g=dict(d['g'], eps=d['g']['eps'][:9])), jitter=kr.MODEL_JITTER)
    with pytest.raises(ValueError, match='inducing points per factor'):
        big = dict(p, Zf=[np.random.RandomState(0).rand(130, 2), p['Zf'][1]], u_fm=np.zeros(130 * 20), u_fs_sqrt=np.ones(130 * 20))
        engine.kron_sample_paths(big, Xn[:30], n_samples=2, n_features=4, rng=0)
    with pytest.raises(ValueError, match='g_offset'):
        engine.kron_sample_paths(p, Xn[:30], n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER, g_offset=float('inf'))
    with pytest.raises(ValueError, match='cuda'):
        engine.kron_sample_paths_device(p, torch.from_numpy(Xn[:30].copy()), n_samples=kr.MODEL_S, draws=d)
    with pytest.raises(ValueError, match="lik must be"):
        engine.kron_head_sample_paths(kron_nd.head_params(p), Xn[:30], 'onoff', n_samples=2)
    # the library's own refusal of host pointers in the _device model calls (the Python wrappers above never let one through)
    sk, keepk, dk = engine._pack_kron(p)
    _, dr, keepd = engine._kron_path_draws(sk, dk, ('f', 'g'), kr.MODEL_S, 0, None, d)
    Xh, outh = np.ascontiguousarray(Xn[:30]), np.zeros((3, kr.MODEL_S, 30))
    rc = engine.lib.zigp_kron_sample_paths_device(engine.ctx, C.byref(sk), C.c_void_p(ptr(Xh)), 30, kr.MODEL_JITTER, 0.0, 0.0, C.addressof(dr['f']),
                                                  C.addressof(dr['g']), kr.MODEL_S, C.c_void_p(ptr(outh)))
    msg = engine.lib.zigp_last_error(engine.ctx).decode()
    assert rc == _lib.ZIGP_EARG and msg.startswith('zigp_kron_sample_paths_device') and 'device memory' in msg, msg
    sh, keeph, dh = engine._pack_kron(kron_nd.head_params(p), tags=('f',))
    rc = engine.lib.zigp_kron_head_sample_paths_device(engine.ctx, C.byref(sh), _lib.LIK_BERNOULLI, C.c_void_p(ptr(Xh)), 30, kr.MODEL_JITTER, 0.0,
                                                       C.addressof(dr['f']), kr.MODEL_S, C.c_void_p(ptr(outh)))
    msg = engine.lib.zigp_last_error(engine.ctx).decode()
    assert rc == _lib.ZIGP_EARG and msg.startswith('zigp_kron_head_sample_paths_device') and 'device memory' in msg, msg
    assert not outh.any()
    dup = dict(p, Zf=[np.vstack([p['Zf'][0][:9], p['Zf'][0][:1]]), p['Zf'][1]])       # a repeated inducing input: factor 0 is singular at jitter 0
    with pytest.raises(NotPositiveDefiniteError, match='Kronecker factor'):
        engine.kron_sample_paths(dup, Xn[:30], n_samples=kr.MODEL_S, draws=d, jitter=0.0)
    again = engine.kron_sample_paths(p, Xn[:30], n_samples=kr.MODEL_S, draws=d, jitter=kr.MODEL_JITTER)
    for k in ('f', 'g', 'gf'):
        assert np.array_equal(again[k], ok[k])


def test_sample_onoff_mean_stays_within_six_standard_errors(engine, tmp_path):
    """sample_onoff from a checkpoint written here: over 256 seeded samples the sample mean of f at every test row stays within 6
    standard errors (the sample's own standard deviation / 16) of predict_onoff's fmean.  n_features = 1024 random features carry the
    prior part of a path; their error is part of what the 6 standard errors allow."""
    from onofftf import predict_onoff, sample_onoff
    from onofftf.model import init_params, save_checkpoint
    rs = np.random.RandomState(12)
    Xtr = np.hstack([rs.rand(400, 2) * 10.0, rs.rand(400, 1)])
    Xte = np.hstack([rs.rand(90, 2) * 10.0, rs.rand(90, 1)])
    grid = np.array([6, 8])
    np.random.seed(5)
    pset = init_params(Xtr, grid, grid, init_noisevar=0.001, kmeans_seed=3)
    pset.params['f_kern/lengthscale_0'].value = np.array([3.0, 3.5])
    pset.params['f_kern/lengthscale_1'].value = np.array([0.3])
    pset.params['g_kern/lengthscale_0'].value = np.array([2.5, 3.0])
    pset.params['g_kern/lengthscale_1'].value = np.array([0.25])
    for t in ('f', 'g'):
        for q in (0, 1):
            pset.params['%s_kern/variance_%d' % (t, q)].value = np.array([1.5])
        pset.params['%s_ind/value' % t].value = rs.randn(48, 1)
        pset.params['%s_ind/variance' % t].value = 0.3 + 0.4 * rs.rand(48, 1)
    save_checkpoint(pset, str(tmp_path / 'model'))
    np.random.seed(5)
    _, pred = predict_onoff(Xtr, Xte, str(tmp_path) + '/', grid, grid, engine=engine)
    np.random.seed(5)
    sm = sample_onoff(Xtr, Xte, str(tmp_path) + '/', 256, grid, grid, n_features=1024, seed=2024, engine=engine)
    assert sm['f'].shape == (256, 90) and set(sm) == {'f', 'g', 'gf', 'draws'}
    mean, se = sm['f'].mean(0), sm['f'].std(0, ddof=1) / 16.0
    z = np.abs(mean - pred['fmean'].reshape(-1)) / se
    print('sample_onoff: largest |sample mean - fmean| / standard error = %.2f' % float(np.max(z)))
    assert np.all(z <= 6.0)
    np.random.seed(5)
    again = sample_onoff(Xtr, Xte, str(tmp_path) + '/', 256, grid, grid, n_features=1024, seed=2024, engine=engine)
    assert np.array_equal(again['f'], sm['f'])


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_sample_svgp_and_sample_scgp_from_a_checkpoint(engine, tmp_path, lik):
    """sample_svgp / sample_scgp from a head checkpoint written here (an f_mu in the classifier's): the paths are those of
    kron_head_sample_paths on the restored parameters with the same draws, bit for bit; over 256 seeded samples the mean of f stays
    within 6 standard errors of predict_svgp's fmean (the Gaussian head returns it; the classifier's f has no predict row)."""
    from onofftf.heads import init_head_params, head_engine_params, head_f_mu
    from onofftf.model import save_checkpoint
    from onofftf.svgppred import predict_svgp, sample_svgp
    from onofftf.svcppred import sample_scgp
    rs = np.random.RandomState(21)
    Xtr = np.hstack([rs.rand(300, 2) * 10.0, rs.rand(300, 1)])
    Xte = np.hstack([rs.rand(70, 2) * 10.0, rs.rand(70, 1)])
    grid, fmu = np.array([5, 7]), lik == 'bernoulli'
    np.random.seed(6)
    pset = init_head_params(Xtr, grid, lik, include_f_mu=fmu, kmeans_seed=4)
    pset.params['f_kern/lengthscale_0'].value = np.array([3.0, 3.5])
    pset.params['f_kern/lengthscale_1'].value = np.array([0.3])
    for q in (0, 1):
        pset.params['f_kern/variance_%d' % q].value = np.array([1.4])
    pset.params['f_ind/value'].value = rs.randn(35, 1)
    pset.params['f_ind/variance'].value = 0.3 + 0.4 * rs.rand(35, 1)
    if fmu:
        pset.params['f_mu'].value = np.array([0.35])
    save_checkpoint(pset, str(tmp_path / 'model'))
    np.random.seed(6)
    if lik == 'gaussian':
        sm = sample_svgp(Xtr, Xte, str(tmp_path) + '/', 256, grid, n_features=512, seed=99, engine=engine)
        assert set(sm) == {'f', 'draws'}
    else:
        sm = sample_scgp(Xtr, Xte, str(tmp_path) + '/', 256, grid, include_f_mu=True, n_features=512, seed=99, engine=engine)
        assert set(sm) == {'f', 'p', 'draws'} and np.all((sm['p'] >= 1e-3) & (sm['p'] <= 1 - 1e-3))
        assert np.array_equal(sm['p'] > 0.5, sm['f'] > 0)
    assert sm['f'].shape == (256, 70)
    direct = engine.kron_head_sample_paths(head_engine_params(pset), Xte, lik, n_samples=256, draws=sm['draws'], jitter=1e-6, f_mu=head_f_mu(pset))
    for k in ('f', 'p') if lik == 'bernoulli' else ('f',):
        assert np.array_equal(direct[k], sm[k]), k
    if lik == 'gaussian':
        np.random.seed(6)
        _, pred = predict_svgp(Xtr, Xte, str(tmp_path) + '/', grid, engine=engine)
        z = np.abs(sm['f'].mean(0) - pred['fmean'].reshape(-1)) / (sm['f'].std(0, ddof=1) / 16.0)
        print('sample_svgp: largest |sample mean - fmean| / standard error = %.2f' % float(np.max(z)))
        assert np.all(z <= 6.0)
