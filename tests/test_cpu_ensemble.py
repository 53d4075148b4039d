"""CPU side of the sample-path scores (include/zigp_ensemble.h): the NumPy restatement alone stands inside the
project's floor on every fixture the GPU test uses, hand cases pin the definition, the group handling and every Python-side refusal come
before the library is touched, and the binding matches the header (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ensemble_ref as er
from zigp import _lib, ensemble as ens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('G', er.BOUND_G)
@pytest.mark.parametrize('S', er.BOUND_S)
def test_restatement_is_inside_the_floor(S, G):
    """scores_np in float64 against the truth (mpmath at 50 digits for S <= 3 and G <= 3, long double otherwise) is <= 8 eps S_w for every
    output and every variogram order: the GPU test's reference alone is well inside the bar it applies.  Largest ratio printed."""
    worst = {}
    for p in (None,) + er.VARIO_PS:
        ref, truth = er.reference(S, G, p)
        for k in er.keys_of(p):
            worst[k if p is None else 'variogram p=%g' % p] = er.ratio(ref[k][0], ref[k][1], truth[k])
    print('S %d G %d N %d: |np - truth| / (eps S_w) = %s' % (S, G, er.fixture(S, G)['N'], {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= er.FLOOR


def test_fixtures_cover_the_shapes():
    sizes = set()
    for S in er.BOUND_S:
        for G in er.BOUND_G:
            f = er.fixture(S, G)
            sizes |= set(np.diff(f['off']).tolist())
            assert f['Ebuf'].shape[1] > f['N'] and f['N'] <= 3000 and (S < 256 or f['N'] <= 300)
    assert set(er.SIZES) | {0} <= sizes
    kinds = {(None if er.fixture(S, G)['a'] is None else bool(np.any(er.fixture(S, G)['a'] == 0))) for S in er.BOUND_S for G in er.BOUND_G}
    assert kinds == {None, False, True}
    assert {er.fixture(S, G)['fair'] for S in er.BOUND_S for G in er.BOUND_G} == {False, True}


def test_hand_cases():
    rs = np.random.RandomState(3)
    N = 37
    y, x = rs.randn(N), rs.randn(N)
    off = np.array([0, N])
    # S = 1: energy = D(x_0, y), the second sum is empty
    r = er.scores_np(x[None, :], y, None, off)
    assert r['energy'][0][0] == r['dist'][0][0, 0, 1] and abs(r['energy'][0][0] - np.sqrt(np.sum((x - y) ** 2))) < 1e-13
    # identical members: the second sum is 0 and energy = D
    r = er.scores_np(np.tile(x, (5, 1)), y, None, off)
    assert np.all(r['dist'][0][0, :5, :5] == 0) and r['energy'][0][0] == r['dist'][0][0, 0, 5]
    # single-row groups: energy = the ensemble CRPS of that row = crps_total (weights 1), and both match the sort-based form
    E = rs.randn(8, N)
    for fair in (False, True):
        r = er.scores_np(E, y, None, np.arange(N + 1), fair)
        direct = np.array([er.ensemble_crps_sorted(E[:, n], y[n], fair) for n in range(N)])
        assert np.max(np.abs(r['energy'][0] - direct)) < 1e-14 and np.max(np.abs(r['crps_total'][0] - direct)) < 1e-14
    # crps_total of weighted group totals against the sort-based CRPS of the totals
    a = rs.rand(N)
    off3 = np.array([0, 10, 10, N])
    r = er.scores_np(E, y, a, off3)
    for g, (lo, hi) in enumerate(zip(off3[:-1], off3[1:])):
        T = (E[:, lo:hi] * a[lo:hi]).sum(1)
        assert abs(r['crps_total'][0][g] - er.ensemble_crps_sorted(T, float((y[lo:hi] * a[lo:hi]).sum()))) < 1e-13
    assert r['energy'][0][1] == 0 and r['crps_total'][0][1] == 0 and not np.signbit(r['energy'][0][1])       # the empty group
    # variogram against the definition written out
    for p in er.VARIO_PS:
        v = er.scores_np(E, y, a, off3, vario_p=p, want=())['variogram'][0]
        for g, (lo, hi) in enumerate(zip(off3[:-1], off3[1:])):
            want = sum(a[i] * a[j] * (abs(y[i] - y[j]) ** p - np.mean(np.abs(E[:, i] - E[:, j]) ** p)) ** 2 for i in range(lo, hi) for j in range(i + 1, hi))
            assert abs(v[g] - want) <= 1e-12 * max(want, 1)
    # the 50-digit definition agrees with the restatement
    m = er.scores_mp(E[:3, :12], y[:12], a[:12], np.array([0, 5, 12]), True, 0.5)
    n = er.scores_np(E[:3, :12], y[:12], a[:12], np.array([0, 5, 12]), True, 0.5)
    for k in ('total', 'total_obs', 'crps_total', 'energy', 'dist', 'variogram'):
        assert np.max(np.abs(m[k] - n[k][0])) < 1e-13, k


def test_integer_operands_are_exact():
    """On small-integer operands the first stage is exact: any order gives the same totals, squared distances and p = 1, 2 variograms"""
    E, y, a, off = er.integer_case(5, 4, [3, 0, 70, 131], True)
    r = er.scores_np(E, y, a, off)
    rl = er.scores_np(E, y, a, off, dtype=np.longdouble)
    assert np.array_equal(r['total'][0], rl['total'][0].astype(np.float64))
    Q = np.round(rl['dist'][0].astype(np.float64) ** 2)          # the integer sums of squares
    assert np.array_equal(r['dist'][0], np.sqrt(Q)) and Q.max() > 1e4
    for p in (1.0, 2.0):
        v, vl = (er.scores_np(E, y, a, off, vario_p=p, dtype=dt, want=())['variogram'][0] for dt in (np.float64, np.longdouble))
        assert np.array_equal(v, vl.astype(np.float64))


def test_groups_labels_and_boundaries():
    off, order, labels = ens.plan_groups(None, 7)
    assert off.tolist() == [0, 7] and order is None and labels is None
    off, order, labels = ens.plan_groups([0, 3, 3, 7], 7)
    assert off.tolist() == [0, 3, 3, 7] and order is None and labels is None and off.dtype == np.int64
    off, order, labels = ens.plan_groups([2, 2, 5, 5, 5, 9, 9], 7)                     # sorted labels: no permutation
    assert off.tolist() == [0, 2, 5, 7] and order is None and labels.tolist() == [2, 5, 9]
    off, order, labels = ens.plan_groups(np.array([9, 2, 5, 2, 9, 5, 5]), 7)           # unsorted: one stable sort
    assert off.tolist() == [0, 2, 5, 7] and labels.tolist() == [2, 5, 9] and order.tolist() == [1, 3, 2, 5, 6, 0, 4]
    off, order, labels = ens.plan_groups([0, 1, 3], 3)                                 # N entries that read as boundaries are boundaries
    assert off.tolist() == [0, 1, 3] and labels is None
    off, order, labels = ens.plan_groups([0, 1, 2], 3)                                 # ... and these are labels
    assert off.tolist() == [0, 1, 2, 3] and labels.tolist() == [0, 1, 2]
    for bad in ([0, 3, 2, 7], [1, 7], [0, 6], [[0, 7]], [0.5, 7.0], []):
        with pytest.raises(ValueError, match='groups'):
            ens.plan_groups(bad, 7)


def test_python_side_refusals():
    """ValueErrors that name the argument, raised before the library is touched (the engine object here has no context at all)"""
    from zigp.engine import DenseEngine
    e = object.__new__(DenseEngine)          # no ctx, no lib: any touch of the library is an AttributeError
    E, y = np.zeros((4, 6)), np.zeros(6)
    with pytest.raises(ValueError, match=r'E must be \(S, N\)'):
        e.ensemble_scores(np.zeros(6), y)
    with pytest.raises(ValueError, match='y must have N'):
        e.ensemble_scores(E, np.zeros(5))
    with pytest.raises(ValueError, match='weights must have N'):
        e.ensemble_scores(E, y, weights=np.ones(5))
    with pytest.raises(ValueError, match='weights must be finite and >= 0'):
        e.ensemble_scores(E, y, weights=-np.ones(6))
    with pytest.raises(ValueError, match='weights must be finite and >= 0'):
        e.ensemble_scores(E, y, weights=np.array([1, 1, np.inf, 1, 1, 1.0]))
    with pytest.raises(ValueError, match='ZIGP_PATH_MAX_S'):
        e.ensemble_scores(np.zeros((257, 6)), y)
    with pytest.raises(ValueError, match='ZIGP_PATH_MAX_S'):
        e.ensemble_scores(np.zeros((0, 6)), y)
    with pytest.raises(ValueError, match='N < 2\\^31'):
        e.ensemble_scores(np.zeros((4, 0)), np.zeros(0))
    with pytest.raises(ValueError, match='fair=True'):
        e.ensemble_scores(E[:1], y, fair=True)
    with pytest.raises(ValueError, match='variogram must be'):
        e.ensemble_scores(E, y, variogram=1.5)
    with pytest.raises(ValueError, match='groups'):
        e.ensemble_scores(E, y, groups=[0, 4, 3, 6])
    with pytest.raises(ValueError, match='ZIGP_ENS_VARIO_MAX_ROWS'):
        e.ensemble_scores(np.zeros((2, 4097)), np.zeros(4097), variogram=1)
    with pytest.raises(ValueError, match="member must be"):
        ens.member_plane('y')
    o = ens.check_args(4, 6, np.array([0, 6]), None, 0.5, True)
    assert (o.fair, o.vario_p) == (1, 0.5)
    o = ens.check_args(4, 6, np.array([0, 6]), None, None, False)
    assert (o.fair, o.vario_p) == (0, 0.0)
    nothing = e.ensemble_scores(E, y, energy=False, totals=False)      # nothing asked: nothing run
    assert all(nothing[k] is None for k in DenseEngine.ENS_KEYS) and nothing['offsets'].tolist() == [0, 6]


def test_binding_matches_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'zigp_ensemble.h')).read()
    main = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    assert '#include "zigp_ensemble.h"' in main
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} zigp_ens_opts;', code).group(1)
    names = [d.split()[-1] for d in body.split(';') if d.strip()]
    assert names == [f[0] for f in _lib.zigp_ens_opts._fields_] == ['fair', 'vario_p'] and C.sizeof(_lib.zigp_ens_opts) == 16
    declared = set(re.findall(r'\bint (zigp_[a-z_]+)\(', code))
    assert declared == set(_lib.ENSEMBLE_SIGNATURES) == {'zigp_ensemble_scores', 'zigp_ensemble_scores_device'}
    for fn in declared:
        m = re.search(r'\bint %s\(([^;]*)\);' % fn, code)
        assert len(m.group(1).split(',')) == len(_lib.ENSEMBLE_SIGNATURES[fn][1]) == 16, fn
    assert int(re.search(r'#define ZIGP_ENS_CHUNK (\d+)', hdr).group(1)) == _lib.ENS_CHUNK == er.CHUNK
    assert int(re.search(r'#define ZIGP_ENS_VARIO_MAX_ROWS (\d+)', hdr).group(1)) == _lib.ENS_VARIO_MAX_ROWS == 4096
    assert 'RMSE / MAE' in hdr          # every entry point cites what it replaces
    from zigp import build
    assert '../../include/zigp_ensemble.h' in build.HEADERS


def test_entry_points_resolve_and_reject_a_null_context():
    lib = _lib.load()
    for fn, (res, args) in _lib.ENSEMBLE_SIGNATURES.items():
        blank = [0 if t in (C.c_int32, C.c_int64) else None for t in args[1:]]
        assert getattr(lib, fn)(None, *blank) == _lib.ZIGP_EARG, fn
