"""CPU side of the k-means entry points (include/zigp.h "inducing inputs"): zigp.inducing.kmeans_np against the
long-double evaluation of kmeans_ref on the seeded fixtures, the fixtures' precondition, the prototypes, the NULL-context refusals and
the Python-side refusals, which are raised before the library is touched (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import kmeans_ref as kr
from zigp import inducing, _lib

NEW = (('zigp_kmeans', 13), ('zigp_kmeans_device', 13), ('zigp_kmeans_resident', 10))


@pytest.mark.parametrize('i', range(len(kr.FIXTURES)))
def test_fixture_precondition_and_shape(i):
    """Asserted on the reference alone: over every iteration the smallest relative gap between a row's two nearest centroids is at
    least 1e-6, so no rounding of a distance can move a label and every comparison of labels is exact, with no case excluded.  Also the
    sizes, the iteration counts (6, 15, 4, 4) and the fourth fixture's empty cluster, which the device tests rely on."""
    X, C0, ref = kr.fixture_run(i)
    seed, K, per, D, extra = kr.FIXTURES[i]
    assert X.shape == (K * per + extra, D) == ((493, 3), (533, 2), (301, 8), (607, 9))[i] and C0.shape == (K, D)
    print('fixture %d: min gap %.2e, n_iter %d, empty %d' % (i, ref['min_gap'], ref['n_iter'], int(np.count_nonzero(ref['counts'] == 0))))
    assert ref['min_gap'] >= kr.MIN_GAP
    assert ref['n_iter'] == (6, 15, 4, 4)[i] and ref['changed'][0] == X.shape[0] and ref['changed'][-1] == 0
    assert int(np.count_nonzero(ref['counts'] == 0)) == (0, 0, 0, 1)[i]
    assert int(ref['counts'].sum()) == X.shape[0]


@pytest.mark.parametrize('i', range(len(kr.FIXTURES)))
def test_kmeans_np_against_the_long_double_reference(i):
    """Labels, counts, changed and n_iter equal the reference exactly (the precondition makes that well defined).  Centroids: a float64
    sum of n terms in ANY order is within (n - 1) u sum |x| of the exact one (u = eps / 2), the division and the reference's own rounding
    add u |mean| each, so err <= (n + 1) u S per entry with S = sum |x| / n -- the a-priori bound, nothing measured.  Inertia: a distance
    of D squares carries at most (D + 2) u relative error, the sum of N of them (N - 1) u: err <= (N + D + 2) u inertia.  An empty
    cluster keeps its start row bit for bit."""
    X, C0, ref = kr.fixture_run(i)
    Cm, info = inducing.kmeans_np(X, C0, 100)
    assert info['n_iter'] == ref['n_iter']
    assert np.array_equal(info['labels'], ref['labels']) and info['labels'].dtype == np.int32
    assert np.array_equal(info['counts'], ref['counts']) and info['counts'].dtype == np.int64
    assert np.array_equal(info['changed'], ref['changed'])
    assert info['n_empty'] == int(np.count_nonzero(ref['counts'] == 0))
    u, (N, D) = kr.EPS / 2, X.shape
    assert np.all(np.abs(Cm - ref['C']) <= (ref['n_made'][:, None] + 1) * u * ref['S'])      # n, S of the update that made the centroid
    assert np.all(np.abs(info['inertia'] - ref['inertia']) <= (N + D + 2) * u * ref['inertia'])
    for j in np.nonzero(ref['counts'] == 0)[0]:
        # the fourth fixture's cluster 4 holds 13 rows in iteration 1 (its start is a data row) and none from iteration 2 on: it keeps,
        # bit for bit, the centroid of the last iteration that gave it rows
        runs = [inducing.kmeans_np(X, C0, k) for k in range(1, info['n_iter'] + 1)]
        last = max(k for k, (_, q) in enumerate(runs) if q['counts'][j] > 0)
        assert last < info['n_iter'] - 1 and np.array_equal(Cm[j], runs[last][0][j]) and not np.array_equal(Cm[j], C0[j])
    # max_iter cuts the run short without changing what came before
    C2, info2 = inducing.kmeans_np(X, C0, 2)
    assert info2['n_iter'] == 2 and np.array_equal(info2['changed'], ref['changed'][:2]) and np.array_equal(info2['inertia'], info['inertia'][:2])


def test_kmeans_np_ties_and_empty_clusters():
    """the lowest index wins a tie; of two identical centroids the second ends empty and unchanged"""
    X = np.array([[0.0], [2.0], [1.0], [1.0], [4.0]])               # rows 2 and 3 sit midway between centroids 0 and 1
    Cm, info = inducing.kmeans_np(X, np.array([[0.0], [2.0], [2.0]]), 1)
    assert info['labels'].tolist() == [0, 1, 0, 0, 1] and info['counts'].tolist() == [3, 2, 0] and info['n_empty'] == 1
    assert Cm.tolist() == [[2.0 / 3.0], [3.0], [2.0]] and info['inertia'].tolist() == [6.0] and info['changed'].tolist() == [5]


def test_sample_rows():
    idx = inducing.sample_rows(50, 7, 3)
    assert idx.dtype == np.int64 and idx.shape == (7,) and len(set(idx.tolist())) == 7 and idx.min() >= 0 and idx.max() < 50
    assert np.array_equal(idx, inducing.sample_rows(50, 7, 3))
    assert np.array_equal(idx, np.random.RandomState(3).choice(50, 7, replace=False))
    assert sorted(inducing.sample_rows(5, 5, 0).tolist()) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match='M = 6'):
        inducing.sample_rows(5, 6, 0)


def test_boundary_null_context_and_signatures():
    """each entry point is bound with as many arguments as include/zigp.h declares and returns ZIGP_EARG on a NULL context before it
    looks at anything else, its outputs untouched; the header's cap is the Python side's"""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name, nargs in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert decl, name
        assert len(args) == decl.group(1).count(',') + 1 == len(getattr(lib, name).argtypes) == nargs, name
        assert res is C.c_int
        sentinel = np.full(8, 7.0)
        n_iter = C.c_int32(-5)
        call = [1 if t in (C.c_int32, C.c_int64) else sentinel.ctypes.data for t in args]     # every array pointer: the sentinel block
        call[0], call[-1] = None, C.byref(n_iter)
        assert getattr(lib, name)(*call) == _lib.ZIGP_EARG, name
        assert np.all(sentinel == 7.0) and n_iter.value == -5
    assert inducing.KMEANS_MAX_M == int(re.search(r'#define ZIGP_KMEANS_MAX_M (\d+)', hdr).group(1)) == 4096
    assert inducing.MAX_D == _lib.MAX_D
    for cite in ('scripts/onoff.py:67', 'svgp.py:64'):
        assert cite in hdr


def test_python_side_refusals():
    """sizes, columns and the start are refused with a ValueError that names the argument, before the library is touched"""
    from zigp.engine import DenseEngine
    e = DenseEngine.__new__(DenseEngine)          # no context: a refusal that reached the library would fail on the missing attribute
    rs = np.random.RandomState(0)
    X = rs.rand(20, 3)
    for kw, match in ((dict(M=0), 'M must be >= 1'), (dict(M=21), 'M must be <= N'), (dict(M=3, max_iter=0), 'max_iter'),
                      (dict(M=3, cols=(-1, 2)), 'cols'), (dict(M=3, cols=(2, 2)), 'cols'), (dict(M=3, cols=(0, 0)), 'cols'),
                      (dict(M=3, cols=5), 'cols'), (dict(M=3, init=rs.rand(3, 2)), 'init'), (dict(M=3, init=rs.rand(4, 3)), 'init'),
                      (dict(M=3, cols=(1, 2), init=rs.rand(3, 3)), 'init')):
        with pytest.raises(ValueError, match=match):
            e.kmeans(X, **kw)
    with pytest.raises(ValueError, match='M must be <= 4096'):
        e.kmeans(np.zeros((5000, 1)), 4097)
    with pytest.raises(ValueError, match=r'D must be in \[1, 64\]'):
        e.kmeans(np.zeros((5, 65)), 2)
    with pytest.raises(ValueError, match='X must be'):
        e.kmeans(np.zeros(5), 2)
    e._full_N, e.D = 0, 0
    with pytest.raises(ValueError, match='no resident data'):
        e.kmeans_resident(3, init=rs.rand(3, 3))
    e._full_N, e.D = 20, 3
    with pytest.raises(ValueError, match='init must be'):
        e.kmeans_resident(3)
    with pytest.raises(ValueError, match='M must be <= N'):
        e.kmeans_resident(21, init=rs.rand(21, 3))
    with pytest.raises(ValueError, match='cols'):
        e.kmeans_resident(3, init=rs.rand(3, 3), cols=(1, 3))
    for f in (inducing.kmeans_np,):
        with pytest.raises(ValueError, match='M must be <= N'):
            f(rs.rand(2, 2), rs.rand(3, 2), 5)


def _same(a, b):
    return set(a.params) == set(b.params) and all(np.array_equal(a.params[k].value, b.params[k].value) for k in a.params)


def test_init_params_default_path_unchanged():
    """kmeans='scipy' is the default and gives, under the same seeds, the arrays of a call without the argument -- for the OnOff
    parameter set and for the heads; an unknown value is refused"""
    from onofftf.model import init_params
    from onofftf.heads import init_head_params
    rs = np.random.RandomState(4)
    X = np.column_stack([rs.rand(300) * 10, rs.rand(300) * 10, rs.rand(300)])

    def both(f, *a, **kw):
        return f(*a, rng=np.random.RandomState(1), kmeans_seed=5, **kw), f(*a, rng=np.random.RandomState(1), kmeans_seed=5, kmeans='scipy', **kw)
    a, b = both(init_params, X, (10, 4), (12, 3))
    assert _same(a, b) and a.params['f_ind/z_0'].value.shape == (10, 2) and a.params['g_ind/z_0'].value.shape == (12, 2)
    a, b = both(init_head_params, X, (10, 4), 'gaussian')
    assert _same(a, b)
    with pytest.raises(ValueError, match='kmeans'):
        init_params(X, (10, 4), (12, 3), kmeans='gpu')
    with pytest.raises(ValueError, match='kmeans'):
        init_head_params(X, (10, 4), 'gaussian', kmeans='gpu')
