"""Stage-level checks of the Matern kernels of the dense path (zigp_set_kernel) through their own hooks: the Kuf panel k_kuf_build_matern
with its derivative panel K' (zigp_test_kuf_kind) against the formula in extended precision, the Kuf-cotangent reductions k_kgrad_matern
(zigp_test_kgrad_kind) against a NumPy restatement bit for bit on integer operands, and the RBF path left as it was."""
import numpy as np
import pytest

from conftest import make_problem
import matern_ref as mr

pytestmark = pytest.mark.gpu
MATERN = ('matern32', 'matern52')
KG_SPLIT = 4


def _panel_inputs(D):
    """N = 1500 (no multiple of the 512-column block), M = 50 (no multiple of 16), ARD lengthscales a factor 100 apart, inducing inputs
    taken from the data rows (r2 = 0 exactly) and one row 1e4 lengthscales away from all of them"""
    rs = np.random.RandomState(50 + D)
    N, M = 1500, 50
    X = rs.randn(N, D)
    ell = np.array([0.5]) if D == 1 else np.logspace(-1.0, 1.0, D)
    Z = X[:M].copy()
    X[N - 1] = 1.0e4 * ell
    return X, Z, ell, 1.7


@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('kind', MATERN)
def test_panel_and_derivative_panel_against_extended_precision(engine, kind, D):
    """K and K' against numpy.longdouble (64-bit mantissa: its own error, 5e-20, is nothing next to either side's).  The bar is not
    fixed in advance: the float64 NumPy formula's largest relative error against the same yardstick on the same inputs, times 8 -- the
    device has a table exp2 within 2 ulp where libm has < 1, a square root within 1 ulp and the polynomial factor, and forms the
    differences from pre-scaled inputs."""
    X, Z, ell, var = _panel_inputs(D)
    N, M = X.shape[0], Z.shape[0]
    assert np.finfo(np.longdouble).nmant >= 63, 'numpy.longdouble is not an extended type here'
    K, Kd = engine.test_kuf_kind(kind, X, Z, ell, var)
    Kv, none = engine.test_kuf_kind(kind, X, Z, ell, var, grad=False)
    assert none is None and np.array_equal(Kv, K), 'the value-only launch writes the same K'
    assert K.shape == (64, N) and Kd.shape == (64, N)
    assert not K[M:].any() and not Kd[M:].any(), 'padded rows m >= M are zeros'
    ref, refd = mr.panel_formula(kind, X, Z, ell, var, np.longdouble)
    f64, f64d = mr.panel_formula(kind, X, Z, ell, var, np.float64)
    far = N - 1
    assert np.all(np.isfinite(K)) and np.all(np.isfinite(Kd)) and np.all(K >= 0) and np.all(Kd >= 0)
    assert not K[:M, far].any() and not Kd[:M, far].any(), 'far pairs are exact zeros'
    assert not ref[:, far].any() and not refd[:, far].any()
    near = np.ones(N, dtype=bool)
    near[far] = False
    assert float(ref[:, near].min()) > 1e-280, 'the compared entries are normal numbers'
    rel = lambda a, b: float(np.max(np.abs(a[:, near].astype(np.longdouble) - b[:, near]) / b[:, near]))
    e_np, e_npd = rel(f64, ref), rel(f64d, refd)
    e_gpu, e_gpud = rel(K[:M], ref), rel(Kd[:M], refd)
    print('MATERN-PANEL %s D=%d: K  device %.3e  float64 NumPy %.3e  ratio %.2f;  K\' device %.3e  float64 NumPy %.3e  ratio %.2f  (bar 8)'
          % (kind, D, e_gpu, e_np, e_gpu / e_np, e_gpud, e_npd, e_gpud / e_npd))
    assert e_gpu <= 8.0 * e_np and e_gpud <= 8.0 * e_npd
    # coincident pairs (Z = X[:M]): the r = 1e-6 value, not var
    k0, kd0 = mr.panel_formula(kind, Z[:1], Z[:1], ell, var, np.longdouble)
    d = np.arange(M)
    eps = np.finfo(np.float64).eps      # e within 2 ulp, then one (K) or two (K') more roundings of products next to it, and the constants'
    assert np.all(np.abs(K[d, d] - float(k0[0, 0])) <= 4 * eps * var) and np.all(np.abs(Kd[d, d] - float(kd0[0, 0])) <= 5 * eps * float(kd0[0, 0]))
    assert np.all(K[d, d] < var)


def test_panel_hook_rbf_is_the_rbf_panel(engine):
    X, Z, ell, var = _panel_inputs(3)
    K, Kd = engine.test_kuf_kind('rbf', X, Z, ell, var)
    assert np.array_equal(K[:50], engine.test_kuf(X, Z, ell, var)) and np.array_equal(Kd, K) and not K[50:].any()


def _kgrad_numpy(Jp, K, Kd, alpha, gm, gv, X, Z, n0, N):
    """The four column groups of krow in float64 NumPy, per KG_SPLIT slab: 0: sum F K; 1 + d: sum F K' (x_d - z_d); 1 + D + d:
    sum F K' (x_d - z_d)^2; 1 + 2 D: sum K gm -- F = alpha gm^T + 2 J' diag(gv), columns n0 + n < N only."""
    M, Nc = K.shape
    D = Z.shape[1]
    out = np.zeros((KG_SPLIT, M, 2 + 2 * D))
    F = alpha[:, None] * gm[None, :] + 2.0 * gv[None, :] * Jp
    span = Nc // KG_SPLIT
    for sp in range(KG_SPLIT):
        cols = np.arange(sp * span, min((sp + 1) * span, N - n0))
        if cols.size == 0:
            continue
        f, k, kd = F[:, cols], K[:, cols], Kd[:, cols]
        df = X[n0 + cols][None, :, :] - Z[:, None, :]
        out[sp, :, 0] = np.sum(f * k, 1)
        out[sp, :, 1:1 + D] = np.sum((f * kd)[:, :, None] * df, 1)
        out[sp, :, 1 + D:1 + 2 * D] = np.sum((f * kd)[:, :, None] * df * df, 1)
        out[sp, :, 1 + 2 * D] = np.sum(k * gm[None, cols], 1)
    return out


@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('kind', MATERN)
def test_kgrad_hook_bit_for_bit_on_integer_operands(engine, kind, D):
    """M = 50, Nc = 1024 with 1000 valid rows: small integers, so that every product and every partial sum is an integer below 2^53 and
    exact in any order -- the comparison is bit-equality, and an indexing mistake (a wrong panel, row, column range or slab) cannot hide
    behind rounding.  K and K' differ everywhere, and the columns beyond the valid rows hold numbers that must not be read."""
    rs = np.random.RandomState(7 * D + len(kind))
    M, Nc, N = 50, 1024, 1000
    ri = lambda lo, hi, *shape: rs.randint(lo, hi + 1, size=shape).astype(np.float64)
    K, Kd, Jp = ri(0, 3, M, Nc), ri(4, 7, M, Nc), ri(-2, 2, M, Nc)
    alpha, gm, gv = ri(-2, 2, M), ri(-2, 2, Nc), ri(-1, 1, Nc)
    X, Z = ri(-3, 3, N, D), ri(-3, 3, M, D)
    want = _kgrad_numpy(Jp, K, Kd, alpha, gm, gv, X, Z, 0, N)
    assert np.max(np.abs(want)) < 2.0 ** 40 and np.all(want == np.round(want))
    got = engine.test_kgrad_kind(kind, Jp, K, Kd, alpha, gm, gv, X, Z)
    assert got.shape == want.shape
    for name, sl in (('sum F K', slice(0, 1)), ('sum F K\' dx', slice(1, 1 + D)), ('sum F K\' dx^2', slice(1 + D, 1 + 2 * D)), ('K gm', slice(1 + 2 * D, 2 + 2 * D))):
        assert np.array_equal(got[:, :, sl], want[:, :, sl]), (kind, D, name)
    assert want[3, :, 0].any() and want[:, :, 1:1 + 2 * D].any()
    # a second chunk accumulates onto the first, and a start row inside the data moves the window
    n0 = 300
    want2 = want + _kgrad_numpy(Jp, K, Kd, alpha, gm, gv, X, Z, n0, N)
    got2 = engine.test_kgrad_kind(kind, Jp, K, Kd, alpha, gm, gv, X, Z, n0=n0, krow=got)
    assert np.array_equal(got2, want2)
    # with K' = K the Matern reduction is the RBF one (the per-row form of k_kgrad)
    assert np.array_equal(engine.test_kgrad_kind(kind, Jp, K, K, alpha, gm, gv, X, Z), engine.test_kgrad_kind('rbf', Jp, K, K, alpha, gm, gv, X, Z))


def test_rbf_is_unchanged_and_the_setting_round_trips(engine):
    """set_kernel(., 'rbf') set explicitly gives the default's elbo bit for bit; after a Matern call, going back to RBF gives the earlier
    numbers bit for bit; get_kernel reports what was set."""
    X, Y, p = make_problem(1500, 50, 3, seed=5, Mg=37)
    engine.set_chunk(1024)
    engine.set_data(X, Y)

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(np.asarray(a[2][k]), np.asarray(b[2][k])) for k in a[2])

    base = engine.elbo(p, jitter=1e-6, scale=1.3)
    base_v = engine.elbo(p, jitter=1e-6, scale=1.3, need_grad=False)
    base_p = engine.predict(p, X[:300])
    assert engine.get_kernel('f') == 'rbf' and engine.get_kernel('g') == 'rbf'
    engine.set_kernel('f', 'rbf'); engine.set_kernel(1, 'rbf')
    assert same(engine.elbo(dict(p, kern_f='rbf', kern_g='rbf'), jitter=1e-6, scale=1.3), base)
    for kf, kg in (('matern52', 'matern32'), ('matern32', 'rbf'), ('rbf', 'matern52')):
        q = dict(p, kern_f=kf, kern_g=kg)
        m = engine.elbo(q, jitter=1e-6, scale=1.3)
        assert engine.get_kernel('f') == kf and engine.get_kernel(1) == kg
        assert np.isfinite(m[0]) and m[0] != base[0]
        engine.predict(q, X[:300])
        assert same(engine.elbo(p, jitter=1e-6, scale=1.3), base)
        assert engine.get_kernel(0) == 'rbf' and engine.get_kernel('g') == 'rbf'
        assert engine.elbo(p, jitter=1e-6, scale=1.3, need_grad=False)[:2] == base_v[:2]
        assert np.array_equal(engine.predict(p, X[:300]), base_p)
    engine.set_kernel('g', 'matern52')
    assert engine.get_kernel('g') == 'matern52' and engine.get_kernel('f') == 'rbf'
    engine.set_kernel('g', 'rbf')
    with pytest.raises(ValueError):
        engine.set_kernel('g', 'matern12')
    with pytest.raises(ValueError):
        engine.get_kernel(2)
    assert engine.get_kernel('g') == 'rbf'
    engine.set_chunk(16384)
