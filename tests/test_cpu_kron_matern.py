"""CPU side of the Matern factors of the Kronecker path: the restatement kron_matern_ref.py against the oracle, what the REFERENCE
alone does on the fixtures of tests/test_gpu_kron_matern.py (op-order floor, conditioning), the spectral draws of a product kernel
(zigp.pathwise.kron_draw), and the engine's argument checks that need no GPU.

Fixtures: the cases d11, d21-12, d21-mix, d31, d17, p88, p43, L32 of kron_nd.CASES with the kinds of kron_matern_ref.FIXTURES.  A GPU
result is judged at the project's 1e-6 only because the floor (factored float64 algebra against the literal dense order) is <= 1e-8 and
cond(K_p + 1e-5 I) <= 1e5 here, the conditions tests/test_cpu_kron_nd.py pins for the RBF fixtures.  Measured (profiles/
kron_matern_parity.log): cond 8.7e1 .. 6.1e3 for the Matern kinds, at most 2.2e4 for RBF."""
import numpy as np
import pytest

import kron_nd
import kron_matern_ref as kmr

pytestmark = pytest.mark.filterwarnings(kron_nd.READ_ONLY_NOTE)


def test_all_rbf_equals_the_oracle_bit_for_bit():
    """with every kind 'rbf' the restatement IS oracle/zigp_oracle_torch.py: values and every gradient block, both heads, predictions"""
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    name = 'd21-12'
    X, Y, p = kron_nd.problem(name)
    sc = kron_nd.case_scale(name)
    a = ot.kron_elbo_and_grad(X, Y, p, kron_nd.JITTER, scale=sc, g_offset=-0.3, f_mu=0.2)
    for q in (p, kmr.with_kinds(p, 'rbf', ('rbf', 'rbf'))):
        b = kmr.kron_elbo_and_grad(X, Y, q, kron_nd.JITTER, scale=sc, g_offset=-0.3, f_mu=0.2)
        assert a[:3] == b[:3]
        for k in a[3]:
            if isinstance(a[3][k], list):
                assert all(np.array_equal(u, v) for u, v in zip(a[3][k], b[3][k])), k
            else:
                assert np.array_equal(a[3][k], b[3][k]), k
    hp = kron_nd.head_params(p)
    for lik in ('gaussian', 'bernoulli'):
        Yh = (Y > 0).astype(np.float64) if lik == 'bernoulli' else Y
        a = ot.kron_head_elbo_and_grad(X, Yh, hp, lik, kron_nd.JITTER, scale=sc, f_mu=0.1)
        b = kmr.kron_head_elbo_and_grad(X, Yh, hp, lik, kron_nd.JITTER, scale=sc, f_mu=0.1)
        assert a[:3] == b[:3]
        for k in a[3]:
            assert all(np.array_equal(u, v) for u, v in zip(a[3][k], b[3][k])) if isinstance(a[3][k], list) else np.array_equal(a[3][k], b[3][k]), k
    # the predictions agree with the NumPy oracle (LAPACK inverse against torch's: the same LU, not the same bits)
    ref = np.stack([np.asarray(r).reshape(-1) for r in o.kron_build_predict(X, p, kron_nd.JITTER, -1.0)])
    got = kmr.kron_build_predict(X, p, kron_nd.JITTER, -1.0)
    assert max(kron_nd._relerr(got[i], ref[i]) for i in range(9)) <= 1e-9


def test_fixture_table_covers_every_pair():
    pairs = {k for v in kmr.FIXTURES.values() for k in v}
    assert pairs == set(kmr.PAIRS), set(kmr.PAIRS) - pairs
    assert sum(1 for kf, kg in kmr.FIXTURES.values() if kf != kg) >= 2
    assert list(kmr.FIXTURES) == ['d11', 'd21-12', 'd21-mix', 'd31', 'd17', 'p88', 'p43', 'L32']


@pytest.mark.parametrize('name', list(kmr.FIXTURES))
def test_fixture_floor_and_conditioning(name):
    X, Y, p = kmr.fixture(name)
    floor, cond = kmr.fixture_floor_and_cond(X, p, kron_nd.JITTER)
    print('%-8s f %s g %s: op-order floor %.2e, max cond(K_p + jitter) %s'
          % (name, p['kern_f'], p['kern_g'], floor, ', '.join('%s %.2e' % kv for kv in sorted(cond.items()))))
    assert floor <= 1e-8, floor
    assert max(cond.values()) <= 1e5, cond


def test_matern_factor_moves_the_prediction():
    """a Matern-3/2 time factor on d21-12 is no small change: what the GPU test of the same name relies on"""
    X, Y, p = kron_nd.problem('d21-12')
    a = kmr.kron_build_predict(X, p, kron_nd.JITTER, 0.0)[3]
    b = kmr.kron_build_predict(X, kmr.with_kinds(p, ('rbf', 'matern32')), kron_nd.JITTER, 0.0)[3]
    assert np.max(np.abs(a - b)) > 1e-3 * np.max(np.abs(a))


def test_kron_draw_with_rbf_kinds_is_draw():
    from zigp import pathwise
    for kinds in ('rbf', ('rbf', 'rbf'), (0, 0)):
        a = pathwise.draw('rbf', 37, 3, 6 * 5, 4, np.random.RandomState(11))
        r = np.random.RandomState(11)
        b = pathwise.kron_draw(kinds, 37, 2, 1, 6, 5, 4, r)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    pathwise.draw('rbf', 9, 3, 30, 2, r1)
    pathwise.kron_draw('rbf', 9, 2, 1, 6, 5, 2, r2)
    assert r1.standard_normal() == r2.standard_normal()      # the generator was consumed alike
    with pytest.raises(ValueError):
        pathwise.kron_draw(('rbf', 'matern12'), 9, 2, 1, 6, 5, 2, np.random.RandomState(0))
    with pytest.raises(ValueError):
        pathwise.kron_draw(('rbf', 'rbf', 'rbf'), 9, 2, 1, 6, 5, 2, np.random.RandomState(0))


@pytest.mark.parametrize('kinds', [('rbf', 'matern32'), ('matern52', 'rbf'), ('matern32', 'matern52'), ('matern52', 'matern52')])
def test_kron_draw_prior_covariance_is_the_product_kernel(kinds):
    """R = 4096 features, a fixed seed: with f_prior = sqrt(2 var / R) sum_r a_r cos(w_r . x + b_r), E_a[f(x) f(x')] is the feature mean
    (2 var / R) sum_r cos(w_r . x + b_r) cos(w_r . x' + b_r), whose expectation over (w, b) is k0 k1.  The standard error is the feature
    sample's own: std of the R terms / sqrt(R).  20 point pairs, 5 standard errors."""
    from zigp import pathwise
    D0, D1, R = 2, 1, 4096
    rs = np.random.RandomState(123)
    d = pathwise.kron_draw(kinds, R, D0, D1, 3, 3, 1, np.random.RandomState(2024))
    ell, var = np.array([0.9, 1.3, 0.6]), (1.7, 0.8)
    Xa = rs.rand(20, 3) * 2.0
    Xb = Xa + rs.randn(20, 3) * np.array([0.8, 0.8, 0.5]) * rs.rand(20, 1)
    om = d['omega0'] / ell[None, :]
    ca, cb = pathwise.features_np(Xa, om, d['phase']), pathwise.features_np(Xb, om, d['phase'])      # (20, R)
    terms = 2.0 * var[0] * var[1] * ca * cb
    emp, se = terms.mean(1), terms.std(1, ddof=1) / np.sqrt(R)
    k0 = np.array([kmr.factor_K_np(kinds[0], Xa[i:i + 1, :D0], Xb[i:i + 1, :D0], ell[:D0], var[0])[0, 0] for i in range(20)])
    k1 = np.array([kmr.factor_K_np(kinds[1], Xa[i:i + 1, D0:], Xb[i:i + 1, D0:], ell[D0:], var[1])[0, 0] for i in range(20)])
    z = (emp - k0 * k1) / se
    print(kinds, 'max |z| %.2f' % np.max(np.abs(z)))
    assert np.all(np.abs(z) <= 5.0), z
    # and the cosines of prior_np are these features
    pr = pathwise.prior_np(Xa, ell, var[0] * var[1], d)
    assert pr.shape == (1, 20)


def test_engine_kind_parsing_and_refusals_without_a_gpu():
    from zigp import _lib
    from zigp.engine import kron_kernel_kinds, kron_matern_factor, DenseEngine
    from zigp import pathwise
    assert kron_kernel_kinds({}) == {'f': (0, 0), 'g': (0, 0)}
    assert kron_kernel_kinds(dict(kern_f='Matern52', kern_g=('rbf', 'matern32'))) == {'f': (2, 2), 'g': (0, 1)}
    assert kron_kernel_kinds(dict(kern_f=['matern32', 'rbf']), ('f',)) == {'f': (1, 0)}
    for bad in ('matern12', ('rbf',), ('rbf', 'rbf', 'rbf'), 3, ('rbf', 1), None):
        with pytest.raises(ValueError, match='kern_g'):
            kron_kernel_kinds(dict(kern_g=bad))
    assert kron_matern_factor(kron_kernel_kinds({})) is None
    assert kron_matern_factor(kron_kernel_kinds(dict(kern_f=('rbf', 'matern52')))) == 'Matern52 kernel on factor 1 of latent f'
    assert kron_matern_factor(kron_kernel_kinds(dict(kern_g='matern32'))) == 'Matern32 kernel on factor 0 of latent g'

    class NoLibrary(DenseEngine):      # the fit-step refusals come before the library is touched: an engine without one shows it
        def __init__(self):
            pass

        def __del__(self):
            pass
    eng = NoLibrary()
    shape = dict(M0f=6, M1f=5, M0g=6, M1g=5, D0=2, D1=1, kern_f=('rbf', 'matern52'))
    z = np.zeros(4)
    with pytest.raises(ValueError, match='kron_fit_steps: a Matern52 kernel on factor 1 of latent f'):
        eng.kron_fit_steps(shape, z, z, z, [0.0] * 17, [0] * 17, 0, [0], 10)
    with pytest.raises(ValueError, match='kron_head_fit_steps: a Matern52 kernel on factor 1 of latent f'):
        eng.kron_head_fit_steps(shape, 'gaussian', z, z, z, [0.0] * 10, [0] * 10, [1] * 10, 0, [0], 10)
    # the path records carry the kinds in their fourth word
    import kronpaths_ref as kr
    lat = kr.random_latent(np.random.RandomState(0), 3, 4, 2, 1, 5, 2)
    recs, keep = DenseEngine._kron_path_latents([lat, dict(lat, kinds=('matern32', 'matern52'))], (2, 1), 2)
    assert (recs[0].reserved, recs[1].reserved) == (0, 1 + 4 * 2)
    with pytest.raises(ValueError):
        DenseEngine._kron_path_latents([dict(lat, kinds='matern12')], (2, 1), 2)
    assert pathwise.kron_kinds('matern32') == (1, 1) and pathwise.kron_kinds(('rbf', 2)) == (0, 2)
    assert {'zigp_set_kron_kernel', 'zigp_get_kron_kernel', 'zigp_test_kron_kbuild_kind', 'zigp_test_kron_kgrad_kind'} <= set(_lib.SIGNATURES)
