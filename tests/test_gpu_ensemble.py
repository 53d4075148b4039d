"""Sample-path scores on the device (include/zigp_ensemble.h; csrc/zigp_ensemble.hip) against
tests/ensemble_ref.py: the bound tier (err_gpu <= 4 err_np + 16 eps S_w against the truth), the exact tier (bit equality on small-integer
operands, and of one group wherever it stands), the agreement of the host, device and strided forms, the model calls end to end, and the
refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.io as sio

import ensemble_ref as er
import kron_nd
from conftest import make_problem, ROOT
from zigp import _lib
from zigp._lib import ptr

pytestmark = pytest.mark.gpu

KEYS = ('total', 'total_obs', 'crps_total', 'energy', 'dist')


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _all(engine, E, y, off, a=None, fair=False, p=None):
    r = engine.ensemble_scores(E, y, groups=off, weights=a, fair=fair, variogram=p, return_dist=True)
    return r


# ---- 1. bound tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', er.BOUND_G)
@pytest.mark.parametrize('S', er.BOUND_S)
def test_bound_tier(engine, S, G):
    """Every output element and every variogram order: |gpu - truth| <= 4 |np - truth| + 16 eps S_w.  The ensemble is a view of a wider
    buffer (ld = N + 5) whose padding columns are NaN: a read outside the rows would poison the result."""
    f = er.fixture(S, G)
    worst = {}
    for p in (None,) + er.VARIO_PS:
        ref, truth = er.reference(S, G, p)
        if p is None:
            got = engine.ensemble_scores(f['E'], f['y'], groups=f['off'], weights=f['a'], fair=f['fair'], return_dist=True)
        else:
            got = engine.ensemble_scores(f['E'], f['y'], groups=f['off'], weights=f['a'], fair=f['fair'], energy=False, totals=False, variogram=p)
        for k in er.keys_of(p):
            t = np.asarray(truth[k], dtype=np.longdouble)
            eg = np.abs(got[k].astype(np.longdouble) - t).astype(np.float64)
            en = np.abs(ref[k][0].astype(np.longdouble) - t).astype(np.float64)
            bar = 4 * en + 16 * er.EPS * ref[k][1]
            name = k if p is None else 'variogram p=%g' % p
            with np.errstate(divide='ignore', invalid='ignore'):
                worst[name] = float(np.max(np.where(eg == 0, 0.0, eg / bar)))
            assert np.all(eg <= bar), (name, worst[name])
    print('S %d G %d N %d: max err_gpu / (4 err_np + 16 eps S_w) = %s' % (S, G, f['N'], {k: '%.4f' % v for k, v in worst.items()}))


# ---- 2. exact tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('S', [4, 16])
def test_integer_operands_equal_the_restatement_bit_for_bit(engine, S, weighted):
    """Small integers, S a power of two: total, total_obs, dist (the correctly rounded square root of an exact integer) and the p = 1 and
    p = 2 variograms are exact, energy and crps_total are the documented order of additions of the same numbers."""
    E, y, a, off = er.integer_case(40 + S, S, [1, 2, 63, 64, 65, 131, 0, 5], weighted)
    for fair in (False, True):
        ref = er.scores_np(E, y, a, off, fair)
        got = _all(engine, E, y, off, a, fair)
        for k in KEYS:
            assert _bits(got[k], ref[k][0]), (k, fair)
    for p in (1.0, 2.0):
        ref = er.scores_np(E, y, a, off, vario_p=p, want=())
        got = engine.ensemble_scores(E, y, groups=off, weights=a, energy=False, totals=False, variogram=p)
        assert _bits(got['variogram'], ref['variogram'][0]), p


def test_a_group_has_the_same_bits_wherever_it_stands(engine):
    """One group of 131 rows at three offsets, inside different N, G and ld, next to empty groups; a repeated call; fewer outputs."""
    rs = np.random.RandomState(8)
    S, n = 17, 131
    B = np.exp(rs.randn(S, n))
    yb, ab = np.exp(rs.randn(n)), rs.rand(n)
    got = []
    for before, after, pad in ((0, 0, 0), (70, 3, 9), (257, 640, 1)):
        N = before + n + after
        buf = rs.randn(S, N + pad)
        y, a = rs.randn(N), rs.rand(N)
        buf[:, before:before + n], y[before:before + n], a[before:before + n] = B, yb, ab
        head = [before // 2, before - before // 2] if before else []
        tail = [after // 3, after - after // 3] if after else []
        off = np.concatenate([[0], np.cumsum(head + [0, n, 0] + tail)])       # an empty group on either side
        g = len(head) + 1
        assert off[g] == before and off[g + 1] == before + n and off[-1] == N
        r = _all(engine, buf[:, :N], y, off, a, False, 0.5)
        got.append({k: np.array(r[k][..., g] if k == 'total' else r[k][g]) for k in KEYS + ('variogram',)})
        again = _all(engine, buf[:, :N], y, off, a, False, 0.5)
        for k in KEYS + ('variogram',):
            assert _bits(r[k], again[k]), k
        only = engine.ensemble_scores(buf[:, :N], y, groups=off, weights=a, totals=False)
        assert _bits(only['energy'], r['energy']) and only['dist'] is None and only['total'] is None
        only = engine.ensemble_scores(buf[:, :N], y, groups=off, weights=a, energy=False)
        assert all(_bits(only[k], r[k]) for k in ('total', 'total_obs', 'crps_total'))
        only = engine.ensemble_scores(buf[:, :N], y, groups=off, weights=a, energy=False, totals=False, return_dist=True)
        assert _bits(only['dist'], r['dist'])
    for k in KEYS + ('variogram',):
        assert _bits(got[0][k], got[1][k]) and _bits(got[0][k], got[2][k]), k
    assert np.all(got[0]['dist'] == got[0]['dist'].T) and np.all(np.diag(got[0]['dist']) == 0)


def _raw(engine, fn, E, ld, S, N, y, a, off, G, fair, p, outs):
    """the C entry itself: outs = six arrays or None (host), or six device pointers"""
    o = _lib.zigp_ens_opts()
    o.fair, o.vario_p = fair, p
    off = np.ascontiguousarray(off, dtype=np.int64)
    P = lambda v: None if v is None else (v if isinstance(v, int) else ptr(v))     # noqa: E731
    return getattr(engine.lib, fn)(engine.ctx, P(E), ld, S, N, P(y), P(a), off.ctypes.data_as(C.POINTER(C.c_int64)), G, C.byref(o), *[P(v) for v in outs])


def test_single_outputs_leave_sentinels_beyond_their_extent(engine):
    """Each output asked for alone at the C boundary: its bits are those of the full call, and the sentinel-filled buffer is untouched
    beyond the output's extent."""
    f = er.fixture(16, 70)
    S, N, G = f['S'], f['N'], f['G']
    E = np.ascontiguousarray(f['E'])
    full = engine.ensemble_scores(E, f['y'], groups=f['off'], weights=f['a'], variogram=2.0, return_dist=True)
    sizes = dict(total=S * G, total_obs=G, crps_total=G, energy=G, variogram=G, dist=G * (S + 1) * (S + 1))
    for i, k in enumerate(('total', 'total_obs', 'crps_total', 'energy', 'variogram', 'dist')):
        buf = np.full(sizes[k] + 7, -777.25)
        outs = [None] * 6
        outs[i] = buf
        rc = _raw(engine, 'zigp_ensemble_scores', E, N, S, N, f['y'], f['a'], f['off'], G, 0, 2.0 if k == 'variogram' else 0.0, outs)
        assert rc == 0, engine.lib.zigp_last_error(engine.ctx)
        assert _bits(buf[:sizes[k]], full[k].reshape(-1)), k
        assert np.all(buf[sizes[k]:] == -777.25), k


# ---- 3. the forms agree ----------------------------------------------------------------------------------------------------------
def test_host_device_and_strided_views_agree(engine):
    import torch
    rs = np.random.RandomState(4)
    S, N = 16, 700
    block = rs.randn(3, S, N)
    y, a = rs.randn(N), rs.rand(N)
    off = np.array([0, 64, 64, 300, 700])
    t = torch.from_numpy(block).cuda()
    y_t, a_t = torch.from_numpy(y).cuda(), torch.from_numpy(a).cuda()
    host = engine.ensemble_scores(block[2], y, groups=off, weights=a, variogram=0.5, return_dist=True)
    dev = engine.ensemble_scores_device(t[2], y_t, groups=off, weights=a_t, variogram=0.5, return_dist=True)
    for k in KEYS + ('variogram',):
        assert dev[k].is_cuda and _bits(dev[k].cpu().numpy(), host[k]), k
    # every other member of a plane: a row stride of 2 N on both sides
    hs = engine.ensemble_scores(block[2, ::2], y, groups=off, weights=a, variogram=0.5, return_dist=True)
    ds = engine.ensemble_scores_device(t[2, ::2], y_t.reshape(N, 1), groups=off, weights=a_t, variogram=0.5, return_dist=True)
    hc = engine.ensemble_scores(np.ascontiguousarray(block[2, ::2]), y, groups=off, weights=a, variogram=0.5, return_dist=True)
    for k in KEYS + ('variogram',):
        assert _bits(ds[k].cpu().numpy(), hs[k]) and _bits(hs[k], hc[k]), k
    # a column window of the block: ld > N
    win = engine.ensemble_scores_device(t[1, :, 100:400], y_t[100:400].contiguous(), groups=None, weights=None)
    hw = engine.ensemble_scores(block[1, :, 100:400], y[100:400])
    assert _bits(win['energy'].cpu().numpy(), hw['energy']) and _bits(win['total'].cpu().numpy(), hw['total'])


def test_unsorted_labels_equal_the_sorted_call(engine):
    import torch
    rs = np.random.RandomState(6)
    S, N = 8, 500
    E, y, a = rs.randn(S, N), rs.randn(N), rs.rand(N)
    labels = rs.randint(0, 9, N) * 3 - 4
    r = engine.ensemble_scores(E, y, groups=labels, weights=a, variogram=1.0, return_dist=True)
    order = np.argsort(labels, kind='stable')
    uniq, counts = np.unique(labels, return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    s = engine.ensemble_scores(E[:, order], y[order], groups=off, weights=a[order], variogram=1.0, return_dist=True)
    d = engine.ensemble_scores_device(torch.from_numpy(E).cuda(), torch.from_numpy(y).cuda(), groups=labels, weights=torch.from_numpy(a).cuda(),
                                      variogram=1.0, return_dist=True)
    assert np.array_equal(r['labels'], uniq) and np.array_equal(r['offsets'], off) and np.array_equal(d['labels'], uniq)
    for k in KEYS + ('variogram',):
        assert _bits(r[k], s[k]) and _bits(d[k].cpu().numpy(), s[k]), k


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def test_path_scores_device_is_ensemble_scores_of_the_fetched_paths(engine):
    import torch
    X, Y, p = make_problem(200, 20, 2, seed=3, Mg=9)
    X_t, Y_t = torch.from_numpy(X).cuda(), torch.from_numpy(np.ascontiguousarray(Y[:, 0])).cuda()
    labels = (np.arange(200) * 7) % 5
    a = np.random.RandomState(1).rand(200)
    for member in ('gf', 'f'):
        r = engine.path_scores_device(p, X_t, Y_t, groups=labels, n_samples=8, member=member, weights=torch.from_numpy(a).cuda(), variogram=1.0,
                                      return_dist=True, rng=5)
        paths = engine.sample_paths_device(p, X_t, n_samples=8, draws=r['draws'])
        h = engine.ensemble_scores(paths[member].cpu().numpy(), Y[:, 0], groups=labels, weights=a, variogram=1.0, return_dist=True)
        for k in KEYS + ('variogram',):
            assert _bits(r[k].cpu().numpy(), h[k]), (member, k)
    eps = torch.from_numpy(np.random.RandomState(2).randn(8, 200)).cuda()
    r = engine.path_scores_device(p, X_t, Y_t, n_samples=8, noise_eps=eps, draws=r['draws'])
    noisy = (engine.sample_paths_device(p, X_t, n_samples=8, draws=r['draws'])['gf'] + float(np.sqrt(p['noise'])) * eps).cpu().numpy()
    h = engine.ensemble_scores(noisy, Y[:, 0])
    assert _bits(r['energy'].cpu().numpy(), h['energy']) and _bits(r['crps_total'].cpu().numpy(), h['crps_total'])
    with pytest.raises(ValueError, match='member must be'):
        engine.path_scores_device(p, X_t, Y_t, member='y')
    with pytest.raises(ValueError, match='noise_eps'):
        engine.path_scores_device(p, X_t, Y_t, n_samples=8, noise_eps=eps[:4])


@pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)
def test_kron_path_scores_device_is_ensemble_scores_of_the_fetched_paths(engine):
    import torch
    X, Y, p = kron_nd.problem('d21-12')
    X = np.array(X)
    y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).reshape(-1))
    N = X.shape[0]
    X_t, Y_t = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    off = np.array([0, N // 3, N // 3, N])
    r = engine.kron_path_scores_device(p, X_t, Y_t, groups=off, n_samples=16, variogram=0.5, return_dist=True, rng=7, jitter=kron_nd.JITTER, g_offset=-1.0)
    paths = engine.kron_sample_paths(p, X, n_samples=16, draws=r['draws'], jitter=kron_nd.JITTER, g_offset=-1.0)
    h = engine.ensemble_scores(paths['gf'], y, groups=off, variogram=0.5, return_dist=True)
    for k in KEYS + ('variogram',):
        assert _bits(r[k].cpu().numpy(), h[k]), k
    assert np.all(h['energy'][[0, 2]] > 0) and h['energy'][1] == 0


def test_crps_of_single_row_groups_is_predict_crps_within_monte_carlo_error(engine):
    """Toy model, S = 256 members with observation noise (noise_eps), single-row groups, fair = True: the ensemble CRPS of a row is an
    unbiased estimate of the CRPS predict_crps has in closed form.  Compared in the sum over the rows: the standard error of that sum comes
    from the ensemble itself -- the same estimate on each of 8 disjoint blocks of 32 members (independent draws of the whole field, so the
    correlation between rows is in it), their standard deviation over sqrt(8).  Ratio printed; the bar is 5 standard errors."""
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    mat = sio.loadmat(os.path.join(ROOT, 'tests', 'golden', 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(0)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=2.), onoffgpf.kernels.RBF(1, lengthscales=2., variance=5.), OnOffLikelihood(), Z, Z.copy())
    m.likelihood.variance = 0.01
    m.optimize(maxiter=5)
    N, S = X.shape[0], 256
    eps = np.random.RandomState(12).randn(S, N)
    r = m.predict_path_scores(X, Y, groups=np.arange(N + 1), num_samples=S, noise_eps=eps, fair=True, energy=False, n_features=4096, seed=3)
    exact = m.predict_crps(X, Y)[:, 0]
    y = np.asarray(Y, dtype=np.float64).reshape(-1)
    direct = np.array([er.ensemble_crps_sorted(r['total'][:, n], y[n], True) for n in range(N)])
    assert np.max(np.abs(direct - r['crps_total'])) <= 1e-12 * np.max(np.abs(direct))
    blocks = np.array([sum(er.ensemble_crps_sorted(r['total'][32 * b:32 * b + 32, n], y[n], True) for n in range(N)) for b in range(8)])
    se = float(np.std(blocks, ddof=1) / np.sqrt(8))
    ratio = abs(float(np.sum(r['crps_total'])) - float(np.sum(exact))) / se
    print('N %d: sum of ensemble CRPS %.6f, closed form %.6f, standard error %.6f, ratio %.3f' % (N, np.sum(r['crps_total']), np.sum(exact), se, ratio))
    assert ratio <= 5


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_next_call_unchanged(engine):
    import torch
    f = er.fixture(3, 3)
    S, N, G = 3, f['N'], 3
    E, y, off = np.ascontiguousarray(f['E']), f['y'], f['off']
    a = np.ones(N) if f['a'] is None else f['a']
    good = lambda: engine.ensemble_scores(E, y, groups=off, weights=a, variogram=1.0, return_dist=True)     # noqa: E731
    base = good()
    out = [np.full(S * G, 5.5), np.full(G, 5.5), np.full(G, 5.5), np.full(G, 5.5), None, None]
    neg, nan = a.copy(), a.copy()
    neg[5], nan[7] = -1e-300, np.nan
    big = np.array([0, 4097])
    cases = [
        ('off', dict(off=np.array([1, 63, 127, N]))), ('off', dict(off=np.array([0, 63, 127, N - 1]))), ('off', dict(off=np.array([0, 130, 127, N]))),
        ('row weights', dict(a=neg)), ('row weights', dict(a=nan)), ('vario_p', dict(p=1.5)), ('vario_p', dict(p=1.0)), ('fair', dict(fair=2)), ('fair', dict(fair=1, S=1)),
        ('S must', dict(S=257)), ('S must', dict(S=0)), ('N must', dict(N=0)), ('ld', dict(ld=N - 1)), ('G must', dict(G=0)), ('E or y', dict(y=None)),
    ]
    for word, kw in cases:
        args = dict(E=E, ld=N, S=S, N=N, y=y, a=a, off=off, G=G, fair=0, p=0.0)
        args.update(kw)
        rc = _raw(engine, 'zigp_ensemble_scores', args['E'], args['ld'], args['S'], args['N'], args['y'], args['a'], args['off'], args['G'],
                  args['fair'], args['p'], out)
        msg = engine.lib.zigp_last_error(engine.ctx).decode()
        assert rc == _lib.ZIGP_EARG and msg.startswith('zigp_ensemble_scores: ') and word in msg, (word, kw, rc, msg)
        assert all(np.all(o == 5.5) for o in out[:4])
        again = good()
        for k in KEYS + ('variogram',):
            assert _bits(again[k], base[k]), (word, k)
    # a variogram group beyond 4096 rows
    Eb, yb, vb = np.zeros((2, 4097)), np.zeros(4097), np.full(1, 5.5)
    rc = _raw(engine, 'zigp_ensemble_scores', Eb, 4097, 2, 4097, yb, None, big, 1, 0, 1.0, [None, None, None, None, vb, None])
    assert rc == _lib.ZIGP_EARG and 'ZIGP_ENS_VARIO_MAX_ROWS' in engine.lib.zigp_last_error(engine.ctx).decode() and vb[0] == 5.5
    # a host pointer handed to the device call
    E_t, y_t = torch.from_numpy(E).cuda(), torch.from_numpy(y).cuda()
    e_t = torch.full((G,), 5.5, dtype=torch.float64, device='cuda')
    rc = _raw(engine, 'zigp_ensemble_scores_device', E_t.data_ptr(), N, S, N, y, None, off, G, 0, 0.0, [None, None, None, e_t.data_ptr(), None, None])
    msg = engine.lib.zigp_last_error(engine.ctx).decode()
    assert rc == _lib.ZIGP_EARG and msg.startswith('zigp_ensemble_scores_device: ') and 'device memory' in msg
    assert torch.all(e_t == 5.5).item()
    again = good()
    for k in KEYS + ('variogram',):
        assert _bits(again[k], base[k]), k
    with pytest.raises(ValueError, match='ensemble_scores_device: E needs'):
        engine.ensemble_scores_device(torch.from_numpy(E), y_t)
    with pytest.raises(ValueError, match='ensemble_scores_device: y needs'):
        engine.ensemble_scores_device(E_t, y_t[:5])


def test_score_onoff_paths_is_ensemble_scores_of_sample_onoff(engine, tmp_path):
    """score_onoff_paths from a checkpoint written here: the same seed gives sample_onoff's paths, and the scores that come back are
    ensemble_scores of those paths' gf plane bit for bit (week labels, unsorted)."""
    from onofftf import sample_onoff, score_onoff_paths
    from onofftf.model import init_params, save_checkpoint
    rs = np.random.RandomState(12)
    Xtr = np.hstack([rs.rand(400, 2) * 10.0, rs.rand(400, 1)])
    Xte = np.hstack([rs.rand(90, 2) * 10.0, rs.rand(90, 1)])
    yte = np.abs(rs.randn(90))
    grid = np.array([6, 8])
    np.random.seed(5)
    pset = init_params(Xtr, grid, grid, init_noisevar=0.001, kmeans_seed=3)
    for t in ('f', 'g'):
        pset.params['%s_ind/value' % t].value = rs.randn(48, 1)
        pset.params['%s_ind/variance' % t].value = 0.3 + 0.4 * rs.rand(48, 1)
    save_checkpoint(pset, str(tmp_path / 'model'))
    weeks = (Xte[:, 2] * 4).astype(np.int64)
    np.random.seed(5)
    sm = sample_onoff(Xtr, Xte, str(tmp_path) + '/', 16, grid, grid, seed=2024, engine=engine)
    np.random.seed(5)
    sc = score_onoff_paths(Xtr, Xte, yte, str(tmp_path) + '/', weeks, 16, grid, grid, variogram=0.5, seed=2024, engine=engine)
    h = engine.ensemble_scores(sm['gf'], yte, groups=weeks, variogram=0.5)
    assert isinstance(sc['energy'], np.ndarray) and np.array_equal(sc['labels'], np.unique(weeks)) and 'draws' in sc
    for k in ('total', 'total_obs', 'crps_total', 'energy', 'variogram'):
        assert _bits(sc[k], h[k]), k
