"""GPU tests of the row calls' shared host layer (csrc/zigp_rows.h): calls of different kinds and sizes on one context do not see each
other's leftovers.  Every row call lays its device regions out from the start of the context's buffers (scratch, scratch2, out9,
path_tab, path_out), so a call runs inside whatever an earlier, larger or different call left there.  The property: each call's outputs
are the same bits in a forward run of the list, in the reverse run on the same engine, and alone on a fresh engine; and a call repeated
after a smaller one of its kind gives its first result again."""
import functools

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu
M, D, S = 16, 2, 17
LEVELS = (0.05, 0.5, 0.95)


def _rows(N, seed):
    """fm, fv, gm, gv, y of N OnOff rows"""
    rs = np.random.RandomState(seed)
    return rs.randn(N), 0.05 + rs.rand(N), 1.5 * rs.randn(N), 0.05 + 2.0 * rs.rand(N), rs.randn(N) * (rs.rand(N) > 0.3)


def _path_latent(rs, kind, Mh, R, var):
    ell = 0.4 + 0.1 * np.arange(D)
    return dict(kind=kind, Z=rs.rand(Mh, D), ell=ell, var=var, V=rs.randn(Mh, S), omega=rs.randn(R, D) / ell, phase=rs.uniform(0, 2 * np.pi, R),
                amp=rs.randn(R, S) * np.sqrt(2.0 * var / R), shift=-0.3)


@functools.lru_cache(maxsize=None)
def _inputs():
    """the dense model (M = 16, D = 2) with its rows, the two path latents and the fixed draws: made once, never changed"""
    from zigp import pathwise
    X, Y, p = make_problem(300, M, D, seed=5)
    rs = np.random.RandomState(21)
    lats = [_path_latent(rs, 'rbf', 7, 9, 1.0), _path_latent(rs, 'matern32', 12, 5, 2.0)]
    draws = {t: pathwise.draw('rbf', 11, D, M, S, rs) for t in 'fg'}
    return dict(X=X, Y=Y.reshape(-1), p=p, lats=lats, draws=draws, noise=float(p['noise']))


def IN(k):
    return _inputs()[k]


def _scores(r):
    return {k: v for k, v in r.items() if v is not None}


def _density(r):
    return dict(zip(('out3', 'sum', 'centre2'), r))


def _paths(r):
    return {k: r[k] for k in ('f', 'g', 'gf')}


# the list of the issue, in its order: name, call
CALLS = [
    ('predict_scores N=300 n_quad=20', lambda e: _scores(e.predict_scores(IN('p'), IN('X'), IN('Y'), n_quad=20, levels=LEVELS))),
    ('density_rows mode N=257 n_quad=256', lambda e: _density(e.density_rows('onoff', *_rows(257, 1), IN('noise'), n_quad=256, centre='mode',
                                                                             return_centre=True))),
    ('score_rows N=5 n_quad=40', lambda e: _scores(e.score_rows('onoff', *_rows(5, 2), IN('noise'), n_quad=40, levels=LEVELS))),      # a whole wave per row, 4 rows per block
    ('score_rows N=9 n_quad=20', lambda e: _scores(e.score_rows('onoff', *_rows(9, 3), IN('noise'), n_quad=20, levels=LEVELS))),      # half a wave per row, 8 rows per block
    ('predict_density N=9', lambda e: _density(e.predict_density(IN('p'), IN('X')[:9], IN('Y')[:9], n_quad=20))),
    ('path_rows N=33 S=17', lambda e: dict(out=e.path_rows(IN('lats'), IN('X')[:33], S))),
    ('sample_paths N=33 S=17', lambda e: _paths(e.sample_paths(IN('p'), IN('X')[:33], n_samples=S, draws=IN('draws')))),
    ('predict N=40', lambda e: dict(out9=e.predict(IN('p'), IN('X')[:40]))),
    ('density_rows gaussian N=1', lambda e: _density(e.density_rows('gaussian', _rows(1, 4)[0], _rows(1, 4)[1], None, None, _rows(1, 4)[4], IN('noise')))),
]


def _run(e, k):
    """the outputs of call k as arrays, each a copy of its own (a sum becomes a 0-d array: array_equal on it is equality of the floats)"""
    out = {name: np.array(v, dtype=np.float64, copy=True) for name, v in CALLS[k][1](e).items()}
    assert out and all(np.all(np.isfinite(v)) for v in out.values()), CALLS[k][0]
    return out


@pytest.fixture(scope='module')
def both_orders():
    """the list forward, then in reverse, on one engine"""
    import zigp
    e = zigp.DenseEngine(0)
    forward = [_run(e, k) for k in range(len(CALLS))]
    reverse = {k: _run(e, k) for k in reversed(range(len(CALLS)))}
    e.close()
    return forward, reverse


def _same(tag, a, b):
    assert sorted(a) == sorted(b), tag
    for name in a:
        assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), (tag, name)


@pytest.mark.parametrize('k', range(len(CALLS)), ids=[c[0].replace(' ', '_') for c in CALLS])
def test_a_call_gives_the_same_bits_in_either_order_and_alone(both_orders, k):
    import zigp
    forward, reverse = both_orders
    e = zigp.DenseEngine(0)
    alone = _run(e, k)
    e.close()
    _same(CALLS[k][0] + ': forward against reverse', forward[k], reverse[k])
    _same(CALLS[k][0] + ': forward against a fresh engine', forward[k], alone)


def test_the_shapes_the_list_is_meant_to_have(both_orders):
    """what the comparison above rests on: the outputs exist in the sizes named, the centre is a searched one, the sums are floats"""
    forward, _ = both_orders
    assert forward[0]['quantiles'].shape == (3, 300) and forward[0]['cdf'].shape == forward[0]['crps'].shape == (300,)
    assert forward[1]['out3'].shape == (3, 257) and forward[1]['centre2'].shape == (2, 257) and np.any(forward[1]['centre2'][0] != 0.0)
    assert forward[2]['crps'].shape == (5,) and forward[3]['crps'].shape == (9,) and forward[4]['out3'].shape == (3, 9)
    assert forward[5]['out'].shape == (2, S, 33) and forward[6]['gf'].shape == (S, 33) and forward[7]['out9'].shape == (9, 40)
    assert forward[8]['out3'].shape == (3, 1)
    for k, total, rows in [(k, 'crps_sum', forward[k]['crps']) for k in (0, 2, 3)] + [(k, 'sum', forward[k]['out3'][0]) for k in (1, 4, 8)]:
        # two orders of adding N numbers differ by at most N eps sum |x|
        assert forward[k][total].shape == () and abs(forward[k][total] - rows.sum()) <= rows.size * np.finfo(float).eps * np.abs(rows).sum()


def test_a_large_call_repeated_after_a_small_one_of_its_kind():
    """predict_scores_device at N = 300 with the CRPS, at N = 7 with one level and neither CDF nor CRPS, at N = 300 again: the buffers
    keep the larger size, so the second call runs inside the first one's contents and the third inside both."""
    import torch
    import zigp
    e = zigp.DenseEngine(0)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(IN('X'))).cuda(), torch.from_numpy(np.ascontiguousarray(IN('Y'))).cuda()

    def big():
        r = e.predict_scores_device(IN('p'), Xd, Yd, n_quad=20, levels=LEVELS)
        return {k: (np.float64(v) if isinstance(v, float) else v.cpu().numpy()) for k, v in r.items()}
    first = big()
    small = e.predict_scores_device(IN('p'), Xd[:7].contiguous(), Yd[:7].contiguous(), n_quad=20, levels=(0.5,), cdf=False, crps=False)
    assert small['cdf'] is None and small['crps'] is None and small['crps_sum'] is None and tuple(small['quantiles'].shape) == (1, 7)
    again = big()
    e.close()
    assert sorted(first) == ['cdf', 'crps', 'crps_sum', 'quantiles', 'sf'] and first['crps'].shape == (300,)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
