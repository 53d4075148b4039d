"""GPU tests of the k-means entry points (include/zigp.h "inducing inputs"): an exact tier on small-integer
operands, one step on random operands against the long-double evaluation, whole runs on the seeded fixtures of kmeans_ref, the fixed
point and repeatability, every refusal of the boundary, and the Python surface.  Accuracy rule of the project:
err_gpu <= 4 err_np + 16 eps S per entry (S = sum |x| / count for a centroid, the inertia itself for the inertia)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import scipy.io as sio

import kmeans_ref as kr
from conftest import make_problem
from zigp import inducing, _lib

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
EPS = kr.EPS


@pytest.fixture(scope='module')
def eng():
    """an engine of the module's own: the tests below change its resident data and its selection"""
    import zigp
    e = zigp.DenseEngine(0)
    yield e
    e.close()


def raw(e, X, C0, max_iter, col0=0, D=None, M=None, N=None, ld=None, hist_fill=0.0, form='host', want=True):
    """The C entry point itself (no Python-side check in front of it): returns (rc, C, labels, counts, history, n_iter, message)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Cm = np.array(C0, dtype=np.float64, order='C')
    N = X.shape[0] if N is None else N
    ld = X.shape[1] if ld is None else ld
    D = Cm.shape[1] if D is None else D
    M = Cm.shape[0] if M is None else M
    lab, cnt = np.full(max(N, 1), -7, dtype=np.int32), np.full(max(M, 1), -7, dtype=np.int64)
    hist = np.full((max(max_iter, 1), 2), hist_fill)
    n = C.c_int32(-7)
    outs = (lab.ctypes.data, cnt.ctypes.data, hist.ctypes.data) if want else (None, None, None)
    if form == 'host':
        rc = e.lib.zigp_kmeans(e.ctx, X.ctypes.data, N, ld, col0, D, M, Cm.ctypes.data, max_iter, outs[0], outs[1], outs[2], C.byref(n))
    elif form == 'host_as_device':
        rc = e.lib.zigp_kmeans_device(e.ctx, C.c_void_p(X.ctypes.data), N, ld, col0, D, M, Cm.ctypes.data, max_iter, outs[0], outs[1], outs[2], C.byref(n))
    else:
        rc = e.lib.zigp_kmeans_resident(e.ctx, col0, D, M, Cm.ctypes.data, max_iter, outs[0], outs[1], outs[2], C.byref(n))
    msg = e.lib.zigp_last_error(e.ctx)
    return rc, Cm, lab, cnt, hist, n.value, (msg.decode() if msg else '')


def bits(*arrays):
    return b''.join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---- 1. exact tier -------------------------------------------------------------------------------------------------------------------
# (N, M, D, ld, col0): every N of {1, 63, 255, 256, 257, 1000}, M of {1, 2, 5, 33, 257, 1024} and D of {1, 2, 3, 8, 9, 17, 64}; N = 1500
# carries M = 1024 (M <= N), N = 300001 is 1172 row tiles over 1024 workgroups, i.e. spans of two tiles (D <= 8: half a group of four
# tiles per pass over the centroids), N = 1048577 is 4097 tiles in spans of five (a whole group and a single tile).  They cross: more than
# one row tile (257 and up), more than one workgroup (257 and up), spans of more than one tile and more than one group (300001, 1048577),
# more than one owner round (M = 257, 1024), the centroid count that is no multiple of the wide kernel's four (M = 5, 33, 257), and the
# D = 8 | 9 switch.
EXACT = ((1, 1, 1, 1, 0), (63, 2, 2, 5, 3), (255, 5, 3, 4, 1), (256, 33, 8, 9, 1), (257, 257, 9, 11, 2), (1000, 5, 17, 20, 3),
         (1000, 33, 64, 66, 1), (1000, 257, 2, 3, 1), (1500, 1024, 3, 5, 2), (1500, 1024, 9, 10, 1), (257, 2, 8, 8, 0), (63, 33, 1, 2, 1),
         (300001, 2, 1, 2, 1), (300001, 5, 9, 10, 1), (1048577, 3, 2, 3, 1))


def exact_case(N, M, D, ld, col0, identical_pair=False):
    """small-integer rows (many duplicates), integer centroids; rows exactly midway between centroids 0 and 1; centroids 1 and 2 (or, for
    identical_pair, 0 and 1) identical"""
    rs = np.random.RandomState(1000 * D + M + N)
    X = rs.randint(-8, 9, size=(N, ld)).astype(np.float64)
    C0 = rs.randint(-8, 9, size=(M, D)).astype(np.float64)
    if M >= 2:
        C0[1] = C0[0]
        if not identical_pair:
            C0[1, 0] += 2.0
            mid = C0[0].copy()
            mid[0] += 1.0                                  # d = 1 to both: the lower index must win
            for i in range(0, N, 7):
                X[i, col0:col0 + D] = mid
    if M >= 3:
        C0[2] = C0[1]
    if N >= 2:
        X[1] = X[0]
    return X, C0


def check_exact(eng, X, C0, col0, D):
    Cn, info = inducing.kmeans_np(X[:, col0:col0 + D], C0, 1)                # every operation exact: NumPy's bits are THE bits
    rc, Cg, lab, cnt, hist, n, msg = raw(eng, X, C0, 1, col0=col0)
    assert rc == 0, msg
    assert n == 1 and np.array_equal(lab, info['labels']) and np.array_equal(cnt, info['counts'])
    assert bits(Cg) == bits(Cn)
    assert hist[0, 0] == info['inertia'][0] and hist[0, 1] == X.shape[0]
    return Cg, lab, cnt


@pytest.mark.parametrize('N,M,D,ld,col0', EXACT)
def test_exact_tier(eng, N, M, D, ld, col0):
    X, C0 = exact_case(N, M, D, ld, col0)
    Cg, lab, cnt = check_exact(eng, X, C0, col0, D)
    if M >= 2:
        mids = lab[np.arange(0, N, 7)]                      # rows midway between centroids 0 and 1 (and 2, the copy of 1)
        assert not np.any((mids == 1) | (mids == 2))        # never the higher index of the tie (a random centroid may sit closer still)
        if M == 2:
            assert np.all(mids == 0)
    if M >= 3:
        assert cnt[2] == 0 and bits(Cg[2]) == bits(C0[2])   # the second of two identical centroids: empty and unchanged
    if N >= 2:
        assert lab[1] == lab[0]


def test_exact_tier_two_identical_centroids(eng):
    X, C0 = exact_case(257, 2, 3, 4, 1, identical_pair=True)
    Cg, lab, cnt = check_exact(eng, X, C0, 1, 3)
    assert cnt.tolist() == [257, 0] and bits(Cg[1]) == bits(C0[1]) and np.all(lab == 0)


# ---- 2. one step on random operands, no exclusions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M,D', ((1000, 33, 3), (1000, 5, 8), (777, 257, 9), (1000, 33, 64), (1500, 1024, 2), (300, 7, 17)))
def test_one_step_on_random_operands(eng, N, M, D):
    rs = np.random.RandomState(N + M + D)
    X = rs.randn(N, D + 2)
    C0 = X[rs.choice(N, M, replace=False), 1:1 + D] + 0.05 * rs.randn(M, D)
    rc, Cg, lab, cnt, hist, n, msg = raw(eng, X, C0, 1, col0=1)
    assert rc == 0, msg
    Xc = np.ascontiguousarray(X[:, 1:1 + D])
    d = kr.distances(Xc, C0)
    assert lab.min() >= 0 and lab.max() < M
    own = d[np.arange(N), lab]
    assert np.all(own <= (1 + 16 * np.longdouble(EPS)) * d.min(axis=1))          # every label optimal to rounding
    ref, counts, S = kr.means_of(Xc, lab, C0)                                    # the means of the DEVICE's labels
    assert np.array_equal(cnt, counts)
    err_np = kr.means_np_error(Xc, lab, C0)
    err = np.abs(Cg - ref)
    worst = float(np.max(err[counts > 0] / (EPS * S[counts > 0])))
    assert np.all(err <= 4 * err_np + 16 * EPS * S)
    for j in np.nonzero(counts == 0)[0]:
        assert bits(Cg[j]) == bits(C0[j])
    inertia = math.fsum(float(v) for v in own)
    e = np.zeros(N)
    for k in range(D):
        e += (Xc[:, k] - C0[lab, k]) ** 2
    err_in, err_in_np = abs(hist[0, 0] - inertia), abs(float(np.sum(e)) - inertia)
    print('KMEANS-STEP N=%d M=%d D=%d: centroid err / (eps S) max %.2f; inertia err / (eps S) %.2f' % (N, M, D, worst, err_in / (EPS * inertia)))
    assert err_in <= 4 * err_in_np + 16 * EPS * inertia


# ---- 3. whole runs on the fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(kr.FIXTURES)))
def test_whole_runs_on_the_fixtures(eng, i):
    X, C0, ref = kr.fixture_run(i)
    assert ref['min_gap'] >= kr.MIN_GAP
    Cg, info = eng.kmeans(X, C0.shape[0], init=C0, max_iter=100, return_info=True)
    assert info['n_iter'] == ref['n_iter']
    assert np.array_equal(info['labels'], ref['labels']) and np.array_equal(info['counts'], ref['counts'])
    assert np.array_equal(info['changed'], ref['changed'])
    err_np = kr.means_np_error(X, ref['labels'], C0)
    err = np.abs(Cg - ref['C'])
    live = ref['counts'] > 0
    print('KMEANS-RUN fixture %d: n_iter %d, centroid err / (eps S) max %.2f' % (i, info['n_iter'], float(np.max(err[live] / (EPS * ref['S'][live])))))
    assert np.all(err[live] <= 4 * err_np[live] + 16 * EPS * ref['S'][live])
    err_in, err_in_np = np.abs(info['inertia'] - ref['inertia']), np.abs(inducing.kmeans_np(X, C0, 100)[1]['inertia'] - ref['inertia'])
    assert np.all(err_in <= 4 * err_in_np + 16 * EPS * ref['inertia'])
    assert info['n_empty'] == (0, 0, 0, 1)[i]
    for j in np.nonzero(~live)[0]:
        # The fourth fixture's cluster 4 takes 13 rows in iteration 1 (its start is a data row, at distance 0 from itself) and none
        # afterwards, so what it keeps bit for bit is the centroid of the last iteration that gave it rows -- not its start row, which
        # the definition has already replaced by then.  The run cut at that iteration shows those bits.
        assert info['counts'][j] == 0
        cuts = [eng.kmeans(X, C0.shape[0], init=C0, max_iter=k, return_info=True) for k in range(1, info['n_iter'] + 1)]
        last = max(k for k, (_, q) in enumerate(cuts) if q['counts'][j] > 0)
        assert last < info['n_iter'] - 1 and bits(Cg[j]) == bits(cuts[last][0][j])
        assert np.all(np.abs(Cg[j] - ref['C'][j]) <= 4 * kr.means_np_error(X, cuts[last][1]['labels'], C0)[j] + 16 * EPS * ref['S'][j])
    # max_iter = 2 stops at 2 and leaves the history rows beyond n_iter as they were
    rc, C2, lab2, cnt2, hist, n, msg = raw(eng, X, C0, 5, hist_fill=-123.25)
    assert rc == 0 and n == min(5, ref['n_iter'])
    rc, C2, lab2, cnt2, hist, n, msg = raw(eng, X, C0, 2, hist_fill=-123.25)
    assert rc == 0 and n == 2 and np.array_equal(hist[:, 1], ref['changed'][:2])
    big = np.full((9, 2), -123.25)
    nn = C.c_int32(0)
    Cb = C0.copy()
    assert eng.lib.zigp_kmeans(eng.ctx, X.ctypes.data, X.shape[0], X.shape[1], 0, X.shape[1], C0.shape[0], Cb.ctypes.data, 2, None, None,
                               big.ctypes.data, C.byref(nn)) == 0
    assert nn.value == 2 and np.all(big[2:] == -123.25) and bits(big[:2]) == bits(hist) and bits(Cb) == bits(C2)


# ---- 4. fixed point and repeatability ---------------------------------------------------------------------------------------------------
def test_fixed_point_repeatability_and_the_three_forms(eng):
    import torch
    X, C0, ref = kr.fixture_run(0)
    N, D = X.shape
    C1, a = eng.kmeans(X, C0.shape[0], init=C0, return_info=True)
    # From the returned C the first assignment is the last one again and the update reproduces C bit for bit.  changed_1 = N by the
    # definition of t = 1, so the loop needs a second iteration to see changed = 0: n_iter = 2 and changed = (N, 0); cut at
    # max_iter = 1 it is n_iter = 1 and changed = (N).
    C2, b = eng.kmeans(X, C0.shape[0], init=C1, return_info=True)
    assert b['n_iter'] == 2 and b['changed'].tolist() == [N, 0] and bits(C2) == bits(C1) and np.array_equal(b['labels'], a['labels'])
    assert b['inertia'][0] == b['inertia'][1] == a['inertia'][-1]
    C2, b = eng.kmeans(X, C0.shape[0], init=C1, max_iter=1, return_info=True)
    assert b['n_iter'] == 1 and b['changed'].tolist() == [N] and bits(C2) == bits(C1) and np.array_equal(b['labels'], a['labels'])
    C3, c = eng.kmeans(X, C0.shape[0], init=C0, return_info=True)           # two identical calls: identical bits in every output
    keys = ('labels', 'counts', 'inertia', 'changed')
    assert bits(C3, *[c[k] for k in keys]) == bits(C1, *[a[k] for k in keys]) and c['n_iter'] == a['n_iter']
    # the three forms, on rows embedded in a wider array (ld = 5, col0 = 1)
    W = np.random.RandomState(3).randn(N, 5)
    W[:, 1:4] = X
    Y = np.zeros(N)
    Ch, h = eng.kmeans(W, C0.shape[0], init=C0, cols=(1, 3), return_info=True)
    assert bits(Ch, *[h[k] for k in keys]) == bits(C1, *[a[k] for k in keys])      # the stride and the offset change nothing
    Wt = torch.from_numpy(W).cuda()
    Cd, d = eng.kmeans_device(Wt, C0.shape[0], init=C0, cols=(1, 3), return_info=True)
    eng.set_data(W, Y)
    Cr, r = eng.kmeans_resident(C0.shape[0], init=C0, cols=(1, 3), return_info=True)
    for Cx, x in ((Cd, d), (Cr, r)):
        assert bits(Cx, *[x[k] for k in keys]) == bits(Ch, *[h[k] for k in keys]) and x['n_iter'] == h['n_iter']
    # init = None samples the same rows in the host and the device form
    Cs, s = eng.kmeans(W, 12, seed=5, cols=(1, 3), return_info=True)
    Ct, t = eng.kmeans_device(Wt, 12, seed=5, cols=(1, 3), return_info=True)
    assert bits(Cs, s['labels']) == bits(Ct, t['labels'])
    assert bits(Cs) == bits(eng.kmeans(W, 12, init=W[inducing.sample_rows(N, 12, 5), 1:4], cols=(1, 3)))


def test_resident_form_ignores_and_keeps_the_selection(eng):
    X, Y, p = make_problem(700, 24, 3, seed=11)
    eng.set_data(X, Y)
    C0 = X[inducing.sample_rows(700, 9, 2)]
    whole = eng.kmeans_resident(9, init=C0, return_info=True)
    idx = np.random.RandomState(0).choice(700, 200, replace=False)
    eng.select_rows(idx)
    e0 = eng.elbo(p, jitter=1e-6)
    sel = eng.kmeans_resident(9, init=C0, return_info=True)
    assert bits(sel[0], sel[1]['labels'], sel[1]['counts']) == bits(whole[0], whole[1]['labels'], whole[1]['counts'])
    assert sel[1]['labels'].shape == (700,) and eng.N == 200
    e1 = eng.elbo(p, jitter=1e-6)
    assert e0[0] == e1[0] and e0[1] == e1[1] and all(bits(e0[2][k]) == bits(e1[2][k]) for k in e0[2])
    eng.select_rows(None)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_argument(eng):
    import zigp
    rs = np.random.RandomState(0)
    X = rs.randn(300, 4)
    C0 = X[:6, 1:4].copy()
    rc, Cg, lab, cnt, hist, n, msg = raw(eng, X, C0, 20, col0=1)
    assert rc == 0
    good, n_good = bits(Cg, lab, cnt, hist) + bytes([n]), n

    def again():
        out = raw(eng, X, C0, 20, col0=1)
        assert out[0] == 0 and bits(*out[1:5]) + bytes([out[5]]) == good

    def refused(word, **kw):
        a = dict(X=X, C0=C0, max_iter=20, col0=1)
        a.update(kw)
        rc, Cb, lab, cnt, hist, n, msg = raw(eng, a.pop('X'), a.pop('C0'), a.pop('max_iter'), hist_fill=-1.5, **a)
        assert rc == _lib.ZIGP_EARG and word in msg, (word, rc, msg)
        assert bits(Cb) == bits(np.asarray(kw.get('C0', C0), dtype=np.float64)) and np.all(lab == -7) and np.all(cnt == -7)     # outputs untouched
        assert np.all(hist == -1.5) and n == -7
        again()
    refused('M must be >= 1', M=0)
    refused('M must be <= N', N=5)
    refused('ZIGP_KMEANS_MAX_M', X=np.zeros((4100, 1)), C0=np.zeros((4097, 1)), col0=0)
    refused('D must be', D=0)
    refused('D must be', D=65)
    refused('col0', col0=-1)
    refused('col0', col0=2)                      # col0 + D = 5 > ld = 4
    refused('max_iter', max_iter=0)
    refused('N must be', N=0)
    Xn = X.copy()
    Xn[17, 2] = np.nan
    refused('not finite', X=Xn)
    Xi = X.copy()
    Xi[299, 3] = np.inf
    refused('not finite', X=Xi)
    Cn = C0.copy()
    Cn[5, 0] = np.nan
    refused('not finite', C0=Cn)
    refused('device memory', form='host_as_device')          # a host pointer is refused, not dereferenced
    fresh = zigp.DenseEngine(0)
    try:
        rc, Cb, lab, cnt, hist, n, msg = raw(fresh, X, C0, 20, col0=1, form='resident')
        assert rc == _lib.ZIGP_EARG and 'no resident data' in msg and bits(Cb) == bits(C0) and n == -7
        out = raw(fresh, X, C0, 20, col0=1)                  # the context works afterwards
        assert out[0] == 0 and bits(*out[1:5]) + bytes([out[5]]) == good
    finally:
        fresh.close()
    eng.set_data(X, np.zeros(300))
    refused('col0', form='resident', col0=2)
    rc, Cr, labr, cntr, histr, nr, msg = raw(eng, X, C0, 20, col0=1, form='resident')
    assert rc == 0 and bits(Cr, labr, cntr, histr) + bytes([nr]) == good
    # the optional outputs may be NULL
    rc, Cq, _, _, _, nq, msg = raw(eng, X, C0, 20, col0=1, want=False)
    assert rc == 0 and bits(Cq) == bits(Cg) and nq == n_good


# ---- 6. surface ---------------------------------------------------------------------------------------------------------------------
def test_kmeans_inducing_feeds_the_model(eng):
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    from onoffgpf.inducing import kmeans_inducing
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = kmeans_inducing(X, 9, seed=1, engine=eng)
    assert Z.shape == (9, 1) and np.all(np.isfinite(Z)) and len(set(Z[:, 0].tolist())) == 9
    assert bits(Z) == bits(kmeans_inducing(X, 9, seed=1))                       # an engine of its own gives the same bits
    np.random.seed(0)
    m = OnOffSVGP(X, Y, kernf=onoffgpf.kernels.RBF(1, lengthscales=2.), kerng=onoffgpf.kernels.RBF(1, lengthscales=2., variance=5.),
                  likelihood=OnOffLikelihood(), Zf=Z, Zg=Z.copy())
    assert np.isfinite(m.compute_log_likelihood())


def test_init_params_on_the_device(eng):
    from onofftf.model import init_params
    from onofftf.heads import init_head_params
    rs = np.random.RandomState(4)
    X = np.column_stack([rs.rand(400) * 10, rs.rand(400) * 10, rs.rand(400)])
    ps = init_params(X, (10, 4), (12, 3), rng=np.random.RandomState(1), kmeans_seed=5, kmeans='device', engine=eng)
    for tag, M in (('f', 10), ('g', 12)):
        want = eng.kmeans(X, M, init=X[inducing.sample_rows(400, M, 5), 0:2], cols=(0, 2))
        assert bits(ps.params['%s_ind/z_0' % tag].value) == bits(want)
    ph = init_head_params(X, (10, 4), 'gaussian', rng=np.random.RandomState(1), kmeans_seed=5, kmeans='device', engine=eng)
    assert bits(ph.params['f_ind/z_0'].value) == bits(ps.params['f_ind/z_0'].value)
