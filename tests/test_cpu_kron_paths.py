"""CPU side of the Kronecker sample paths (include/zigp_kronpaths.h): the factored weights and
the factored sum are the dense ones on the expanded grid, zero draws collapse onto the oracle's predictive means, the float64
restatement stands well inside the project's path bound, and the Python-side refusals come before the library is touched (no GPU)."""
import os
import re

import numpy as np
import pytest

import kron_nd
import kronpaths_ref as kr
import paths_ref as pr
from zigp import pathwise, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kron_weights_equal_dense_weights_on_the_kronecker_product():
    """kron_weights_np (per-factor Cholesky) against pathwise.weights_np on np.kron(K0, K1): two backward-stable solves of the same
    system, so they differ by at most ~cond eps of the solution.  M0 x M1 = 5 x 7, cond(K0) cond(K1) printed; the bound is
    64 eps cond relative to the largest weight."""
    rs = np.random.RandomState(11)
    M0, M1, S = 5, 7, 6
    Z0, Z1 = rs.rand(M0, 2), rs.rand(M1, 1)
    K0 = kr.rbf(Z0, [0.4, 0.5], 1.3) + 1e-6 * np.eye(M0)
    K1 = kr.rbf(Z1, [0.2], 0.8) + 1e-6 * np.eye(M1)
    u, s, eps, fZ = rs.randn(M0 * M1), 0.5 + rs.rand(M0 * M1), rs.randn(M0 * M1, S), rs.randn(M0 * M1, S)
    Vk = pathwise.kron_weights_np(K0, K1, u, s, eps, fZ)
    Vd = pathwise.weights_np(np.kron(K0, K1), u, s, eps, fZ)
    cond = np.linalg.cond(K0) * np.linalg.cond(K1)
    err = np.max(np.abs(Vk - Vd)) / np.max(np.abs(Vd))
    print('cond %.2e, relative difference %.2e, bound %.2e' % (cond, err, 64 * kr.EPS * cond))
    assert Vk.shape == (M0 * M1, S)
    assert err <= 64 * kr.EPS * cond
    with pytest.raises(ValueError, match='eps and fZ'):
        pathwise.kron_weights_np(K0, K1, u, s, eps[:, :2], fZ)


@pytest.mark.parametrize('dims,grid', [((2, 1), (3, 7)), ((1, 2), (5, 1)), ((4, 4), (6, 5))])
def test_factored_sum_equals_dense_sum_on_the_expanded_grid(dims, grid):
    """kron_path_sum_np against paths_ref.path_sum_np on the expanded grid with var0 var1: the same sum, another association; they
    agree within 8 eps of the point-wise magnitude (the two restatements' own roundings), and so do the magnitudes to 1e-12."""
    rs = np.random.RandomState(5)
    lat = kr.random_latent(rs, grid[0], grid[1], dims[0], dims[1], 7, 5)
    X = rs.rand(33, dims[0] + dims[1])
    a, ma = kr.kron_path_sum_np(lat, X)
    b, mb = pr.path_sum_np(kr.expand(lat), X)
    assert a.shape == (5, 33)
    assert np.all(np.abs(a - b) <= 8 * kr.EPS * ma)
    assert np.max(np.abs(ma - mb) / mb) < 1e-12
    got_mp = kr.kron_path_sum_mp(lat, X, [0, 32], [0, 4])
    assert np.all(np.abs(a[np.ix_([0, 4], [0, 32])] - got_mp) <= 8 * kr.EPS * ma[np.ix_([0, 4], [0, 32])])


@pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)
@pytest.mark.parametrize('name', ['d21-12', 'd21-mix'])
def test_zero_draws_collapse_onto_the_oracle_means(name):
    """a = 0 and eps = 0: a path is k(x, Z) K^-1 u, the oracle's fmean / gmean (kron_build_predict rows 3 and 5; jitter 1e-5 as the
    oracle fixture).  Bound: the project's path bound for the case."""
    X, Y, p = kron_nd.problem(name)
    z = pr.zero_draws(kr.model_draws(name))
    got = kr.kron_sample_paths_np(p, X, z, kron_nd.JITTER, 0.0)
    ref = kron_nd.oracle_predict(name, 0.0)
    bound, c = kr.path_bound(p, ('f', 'g'), kron_nd.JITTER)
    ef = max(kr.plane_err(got['f'][s], ref[3]) for s in (0, kr.MODEL_S - 1))
    eg = max(kr.plane_err(got['g'][s], ref[5]) for s in (0, kr.MODEL_S - 1))
    print('%s: cond product %.2e, bound %.2e, f %.2e, g %.2e' % (name, c, bound, ef, eg))
    assert ef <= bound and eg <= bound
    assert np.array_equal(got['f'][0], got['f'][-1])


@pytest.mark.parametrize('name', ['d21-12', 'd21-mix', 'd31', 'L32'])
def test_float64_restatement_is_inside_an_eighth_of_the_bound(name):
    """Floor pin: kron_sample_paths_np in float64 against the same statement in long double (Cholesky, solves, kernel, cosines), each of
    the planes f, g, gf normalised by its largest entry, stays at or below 1/8 of min(max(1e-9, 1e-13 c), 1e-6), c = cond(K0) cond(K1):
    the GPU tests' reference alone is well inside the bound they apply."""
    X, Y, p = kron_nd.problem(name)
    d = kr.model_draws(name)
    a = kr.model_ref(name)
    b = kr.kron_sample_paths_np(p, X, d, kr.MODEL_JITTER, 0.0, 0.0, dt=np.longdouble)
    bound, c = kr.path_bound(p, ('f', 'g'), kr.MODEL_JITTER)
    err = max(kr.plane_err(a[k], b[k]) for k in ('f', 'g', 'gf'))
    print('%s: cond product %.2e, bound %.2e, float64 against long double %.2e' % (name, c, bound, err))
    assert err <= bound / 8


def test_python_side_refusals():
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError, match='D0 \\+ D1 <= 8'):
        pathwise.check_kron_sizes(5, 4, 3, 3, 4)
    with pytest.raises(ValueError, match='D0, D1 >= 1'):
        pathwise.check_kron_sizes(0, 2, 3, 3, 4)
    with pytest.raises(ValueError, match='inducing points per factor'):
        pathwise.check_kron_sizes(2, 1, 129, 3, 4)
    with pytest.raises(ValueError, match='inducing points per factor'):
        pathwise.check_kron_sizes(2, 1, 3, 0, 4)
    with pytest.raises(ValueError, match='ZIGP_PATH_MAX_S'):
        pathwise.check_kron_sizes(2, 1, 3, 3, 257)
    pathwise.check_kron_sizes(7, 1, 128, 128, 256)
    from zigp.engine import DenseEngine
    lat = kr.random_latent(rs, 3, 4, 2, 1, 5, 2)
    recs, keep = DenseEngine._kron_path_latents([lat], (2, 1), 2)
    assert (recs[0].M0, recs[0].M1, recs[0].R) == (3, 4, 5)
    with pytest.raises(ValueError, match='V must be'):
        DenseEngine._kron_path_latents([dict(lat, V=lat['V'][:, :1])], (2, 1), 2)
    with pytest.raises(ValueError, match='Z must be'):
        DenseEngine._kron_path_latents([lat], (1, 2), 2)
    with pytest.raises(ValueError, match='one or two latents'):
        DenseEngine._kron_path_latents([lat, lat, lat], (2, 1), 2)
    with pytest.raises(ValueError, match='omega must be'):
        DenseEngine._kron_path_latents([dict(lat, omega=lat['omega'][:, :2])], (2, 1), 2)
    X, Y, p = kron_nd.problem('d21-12')
    s, keep, dims = DenseEngine._pack_kron(p)
    d = kr.model_draws('d21-12')
    draws, recs, keepd = DenseEngine._kron_path_draws(s, dims, ('f', 'g'), kr.MODEL_S, 0, None, d)
    assert recs['f'].R == kr.MODEL_R and draws is d
    with pytest.raises(ValueError, match='draw_f.eps must be'):
        DenseEngine._kron_path_draws(s, dims, ('f', 'g'), kr.MODEL_S, 0, None, dict(d, f=dict(d['f'], eps=d['f']['eps'][:5])))
    new, _, _ = DenseEngine._kron_path_draws(s, dims, ('f',), 3, 9, 5, None)
    assert new['f']['omega0'].shape == (9, 3) and new['f']['eps'].shape == (200, 3)
    assert np.array_equal(pathwise.kron_grid(np.array([[1.0], [2.0]]), np.array([[5.0], [6.0], [7.0]])),
                          np.array([[1, 5], [1, 6], [1, 7], [2, 5], [2, 6], [2, 7.0]]))


def test_binding_matches_the_header():
    """The new record's fields, in order, and the new entry points' argument counts are those of include/zigp_kronpaths.h, the header
    include/zigp.h includes; every function it declares is bound (zigp._lib.KRON_PATH_SIGNATURES) and nothing else is."""
    hdr = open(os.path.join(ROOT, 'include', 'zigp_kronpaths.h')).read()
    main = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    assert '#include "zigp_kronpaths.h"' in main and 'have no sample paths' not in main
    body = re.search(r'typedef struct \{([^}]*)\} zigp_kron_path_latent;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip().lstrip('*').strip() for decl in body.split(';') if decl.strip()
             for n in decl.replace('const double', '').replace('int32_t', '').replace('double', '').split(',')]
    assert names == [f[0] for f in _lib.zigp_kron_path_latent._fields_]
    assert names == ['M0', 'M1', 'R', 'reserved', 'Z0', 'Z1', 'ell0', 'ell1', 'var0', 'var1', 'V', 'omega', 'phase', 'amp', 'shift']
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\bint (zigp_[a-z_]+)\(', code))
    assert declared == set(_lib.KRON_PATH_SIGNATURES) == {
        'zigp_kron_path_rows', 'zigp_kron_path_rows_device', 'zigp_kron_sample_paths', 'zigp_kron_sample_paths_device',
        'zigp_kron_head_sample_paths', 'zigp_kron_head_sample_paths_device'}
    for fn in declared:
        m = re.search(r'\bint %s\(([^;]*)\);' % fn, code)
        assert len(m.group(1).split(',')) == len(_lib.KRON_PATH_SIGNATURES[fn][1]), fn
    assert _lib.KRON_PATH_MAX_M == 128


def test_entry_points_resolve_and_reject_a_null_context():
    """Every new entry point resolves in the built library and returns ZIGP_EARG for a NULL context before it reads an argument"""
    import ctypes as C
    lib = _lib.load()
    for fn, (res, args) in _lib.KRON_PATH_SIGNATURES.items():
        assert args[0] is C.c_void_p, fn
        blank = [0.0 if t is C.c_double else 0 if t in (C.c_int32, C.c_int64) else None for t in args[1:]]
        assert getattr(lib, fn)(None, *blank) == _lib.ZIGP_EARG, fn
