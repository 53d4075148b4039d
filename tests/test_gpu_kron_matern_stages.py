"""Stage-level parity of the Matern factor kernels of the Kronecker panel path (csrc/zigp_kron.hip): ONE launch of
k_kron_kbuild_matern<KIND, GRAD> (zigp_test_kron_kbuild_kind) or k_kron_kgrad_matern (zigp_test_kron_kgrad_kind) on caller-supplied operands.

The build kernel follows the project's rule, err_gpu <= 4 err_np + 16 eps S per element, against numpy.longdouble on the GPU's own inputs:
  truth   the formula in 64-bit-mantissa arithmetic from the differences (z - x) / ell;
  numpy   the kernel's arithmetic restated in float64: inputs times 1 / ell, r2 summed from 0 in ascending d of (z / ell - x / ell)^2,
          r = sqrt(r2 + 1e-12), then matern_k / matern_kd's expressions;
  S       the element's magnitude plus its first-order sensitivity to the roundings of r2.  Forming t_d = z_d / ell_d - x_d / ell_d in
          float64 costs up to ~2 eps (|z_d| + |x_d|) / ell_d each, so r2 moves by c eps with c = r2 + 2 sum_d |t_d| (|z_d| + |x_d|) / ell_d,
          and an element f(r2) by |df / d(r2 / 2)| c eps / 2:  S_K = K + K' c / 2,  S_K' = K' + K'' c / 2  with K'' = -dK' / d(r2 / 2) =
          3 sqrt3 var exp(-sqrt3 r) / r (Matern32: the cusp of the 3/2 kernel -- K' really is that sensitive next to r = 0) and
          (25 / 3) var exp(-sqrt5 r) (Matern52);
  plus the gradual-underflow term 2 P 2^-1074, P the factor that multiplies exp(-a r): the exponential is rounded to the subnormal grid
  before that product (for a result that is itself below the grid the term is the whole bound: far pairs must come out as +0, not NaN).
The cotangent kernel is bit-equal to its NumPy restatement on small-integer operands and inside the restatement's summed bound on random
ones.  Every test prints STAGE-LOG lines (profiles/kron_matern_parity.log keeps a run's)."""
import numpy as np
import pytest

import stage_ref as sr
from test_gpu_stages import _assert_exact_premise, _compare, sr_sentinel

pytestmark = pytest.mark.gpu
MATERN = ('matern32', 'matern52')
L = np.longdouble
BUILD_M, BUILD_N, BUILD_D = (5, 16, 33, 130), (1, 255, 257, 1025), (1, 3, 8)
KGRAD_M, KGRAD_D, KGRAD_N, KGRAD_NC = (5, 16, 33), (1, 3, 8), (1, 257, 1000), 1024


def _elements(kind, r2, var, dtype):
    """(K, K', K'', P) from r2 in `dtype` arithmetic, the expressions of matern_k / matern_kd"""
    one, r = dtype(1.0), np.sqrt(r2 + dtype(1e-12))
    if kind == 'matern32':
        t = np.sqrt(dtype(3.0)) * r if dtype is L else dtype(np.sqrt(3.0)) * r
        e = np.exp(-t)
        P = var * (one + t)
        return P * e, dtype(3.0) * var * e, dtype(3.0) * np.sqrt(dtype(3.0)) * var * e / r, P
    t = np.sqrt(dtype(5.0)) * r if dtype is L else dtype(np.sqrt(5.0)) * r
    e = np.exp(-t)
    P = var * (one + t + (dtype(5.0) / dtype(3.0)) * (r * r))
    return P * e, (dtype(5.0) / dtype(3.0)) * var * (one + t) * e, (dtype(25.0) / dtype(3.0)) * var * e, P


def _build_refs(kind, X, col0, Z, ell, var, Nc):
    """truth (K, K'), numpy (K, K'), S (K, K') and the underflow term, (M, Nc) each; columns n >= N are the kernel at x = 0"""
    M, D = Z.shape
    xs = np.zeros((Nc, D))
    xs[:X.shape[0]] = X[:, col0:col0 + D]
    d = (Z.astype(L)[:, None, :] - xs.astype(L)[None, :, :]) / ell.astype(L)
    r2 = (d * d).sum(-1)
    tK, tKd, tKdd, P = _elements(kind, r2, L(var), L)
    inv = 1.0 / ell                                                       # make_hyp: 1 / ell rounded once
    t64 = Z[:, None, :] * inv - (xs * inv)[None, :, :]
    r2_64 = np.zeros((M, Nc))
    for k in range(D):
        r2_64 = t64[:, :, k] * t64[:, :, k] + r2_64
    nK, nKd, _, _ = _elements(kind, r2_64, np.float64(var), np.float64)
    c = np.asarray(r2 + 2 * (np.abs(d) * (np.abs(Z)[:, None, :] + np.abs(xs)[None, :, :]) / ell).sum(-1), dtype=np.float64)
    tK64, tKd64, tKdd64 = (np.asarray(a, dtype=np.float64) for a in (tK, tKd, tKdd))
    under = 2.0 * np.asarray(P, dtype=np.float64) * 2.0 ** -1074
    return (tK, tKd), (nK, nKd), (tK64 + 0.5 * tKd64 * c, tKd64 + 0.5 * tKdd64 * c), under


def _rule(stage, name, gpu, ref64, truth, S, under):
    e_g = np.asarray(np.abs(gpu.astype(L) - truth), dtype=np.float64)
    e_n = np.asarray(np.abs(ref64.astype(L) - truth), dtype=np.float64)
    bound = 4 * e_n + 16 * sr.EPS * S + under
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(e_g == 0, 0.0, e_g / (sr.EPS * S + under))
        rn = np.where(e_n == 0, 0.0, e_n / (sr.EPS * S + under))
    print('STAGE-LOG %-12s %-34s max err_gpu / (eps S) = %.4g (numpy: %.4g)' % (stage, name, float(np.max(r)), float(np.max(rn))))
    bad = e_g > bound
    if bad.any():
        i, j = np.unravel_index(int(np.argmax(np.where(bad, r, 0))), e_g.shape)
        pytest.fail('%s, %s: row %d col %d: gpu %.17g truth %.17g err_gpu %.3g > 4 * %.3g + 16 eps * %.3g; %d of %d elements off' % (
            stage, name, i, j, gpu[i, j], float(truth[i, j]), e_g[i, j], e_n[i, j], S[i, j], int(bad.sum()), bad.size))


@pytest.mark.parametrize('D', BUILD_D)
@pytest.mark.parametrize('M', BUILD_M)
@pytest.mark.parametrize('kind', MATERN)
def test_build_panels_follow_the_rule(engine, kind, M, D):
    """K and K' of every N per (kind, M, D), col0 = 2 and ldx = D + 3.  The inputs hold, where N allows, rows that ARE inducing inputs
    (x = z exactly: r2 = 0, K the formula at r = 1e-6 -- below var -- and K' finite) and a row 1e3 lengthscales away from everything
    (exp underflows: exact +0 in both panels, no NaN); the rest lies 0.3 to 30 lengthscales out.  Rows m >= M are exact zeros in both
    panels, the padding columns n >= N hold the kernel at x = 0 bit for bit, and the value-only launch writes the same K."""
    assert np.finfo(L).nmant >= 63, 'numpy.longdouble is not an extended type here'
    col0 = 2
    for N in BUILD_N:
        Nc = sr.round_up(N, 256)
        rng = np.random.RandomState(1000 * M + 10 * D + N % 5 + len(kind))
        ell, var = 0.5 + rng.rand(D), 1.7
        Z = rng.randn(M, D)
        X = rng.randn(N, col0 + D + 1) * rng.choice([0.3, 3.0, 30.0], size=(N, 1))
        ncoin = min(M, N // 2)
        X[:ncoin, col0:col0 + D] = Z[:ncoin]
        far = N - 1 if N > 1 else None
        if far is not None:
            X[far, col0:col0 + D] = 1.0e3 * ell
        stage = 'kron-kbuild/%s M=%d D=%d N=%d' % (kind, M, D, N)
        K, Kd = engine.test_kron_panel_kbuild_kind(kind, X, col0, Z, ell, var, Nc)
        Kv, none = engine.test_kron_panel_kbuild_kind(kind, X, col0, Z, ell, var, Nc, grad=False)
        Mq = sr.round_up(M, 128)
        assert none is None and np.array_equal(Kv, K), '%s: the value-only launch writes another K' % stage
        assert K.shape == (Mq, Nc) and Kd.shape == (Mq, Nc)
        assert np.all(np.isfinite(K)) and np.all(np.isfinite(Kd)) and np.all(K >= 0) and np.all(Kd >= 0), '%s: a non-finite or negative element' % stage
        assert not K[M:].any() and not Kd[M:].any(), '%s: a row m >= M is not exactly 0' % stage
        (tK, tKd), (nK, nKd), (SK, SKd), under = _build_refs(kind, X, col0, Z, ell, var, Nc)
        _rule(stage, 'K', K[:M], nK, tK, SK, under)
        _rule(stage, "K'", Kd[:M], nKd, tKd, SKd, under)
        i = np.arange(ncoin)
        if ncoin:
            k1 = float(_elements(kind, L(0.0), L(var), L)[0])
            assert np.all(K[i, i] < var) and np.all(np.abs(K[i, i] - k1) <= 4 * np.finfo(np.float64).eps * var), '%s: x = z is not the r = 1e-6 value' % stage
            assert np.all(Kd[i, i] > 0)
        if far is not None:
            assert not K[:M, far].any() and not Kd[:M, far].any(), '%s: the far row did not underflow to +0' % stage
            assert not np.signbit(K[:M, far]).any() and not np.signbit(Kd[:M, far]).any()
        at0, atd0 = engine.test_kron_panel_kbuild_kind(kind, np.zeros((1, col0 + D + 1)), col0, Z, ell, var, 256)
        assert at0[:M, 0].all()
        assert np.array_equal(K[:, N:], np.repeat(at0[:, :1], Nc - N, 1)) and np.array_equal(Kd[:, N:], np.repeat(atd0[:, :1], Nc - N, 1)), \
            '%s: a padding column is not the kernel at x = 0' % stage


def test_build_hook_rbf_is_the_rbf_panel(engine):
    rng = np.random.RandomState(3)
    X, Z, ell = rng.randn(300, 6), rng.randn(33, 3), 0.5 + rng.rand(3)
    K, Kd = engine.test_kron_panel_kbuild_kind('rbf', X, 2, Z, ell, 1.7, 512)
    assert np.array_equal(K, engine.test_kron_panel_kbuild(X, 2, Z, ell, 1.7, 512)) and np.array_equal(Kd, K)


def _kgrad_ref(B, A, PdA, K, Kd, gm, dq, X, col0, Z, krow0, dtype=np.float64):
    """k_kron_kgrad_matern restated (stage_ref.kron_kgrad with the derivative panel): dK = gm B + 2 dq A + PdA; krow[m] += [sum dK K,
    sum dK K' (x_d - z_md), sum dK K' (x_d - z_md)^2] over the N = len(X) valid columns; the last column is not touched.  Bound of the GPU side
    alone, as there: gamma_(N+9) (sum_n T |x - z|^p + |krow0|), T = (|gm B| + 2 |dq A| + |PdA|) |K or K'|."""
    f = lambda a: np.asarray(a, dtype=dtype)
    M, D = Z.shape
    N = X.shape[0]
    B, A, PdA, K, Kd, gm, dq, Xc, Zc = f(B)[:, :N], f(A)[:, :N], f(PdA)[:, :N], f(K)[:, :N], f(Kd)[:, :N], f(gm)[None, :N], f(dq)[None, :N], \
        f(X)[:, col0:col0 + D], f(Z)
    dk = gm * B + 2 * dq * A + PdA
    adk = np.abs(gm * B) + 2 * np.abs(dq * A) + np.abs(PdA)
    t, T = dk * Kd, adk * np.abs(Kd)
    out = f(krow0).copy()
    bnd = np.abs(out)
    bnd[:, 1 + 2 * D] = 0
    out[:, 0] += (dk * K).sum(1)
    bnd[:, 0] += (adk * np.abs(K)).sum(1)
    for d in range(D):
        df = Xc[None, :, d] - Zc[:, None, d]
        out[:, 1 + d] += (t * df).sum(1)
        out[:, 1 + D + d] += (t * df * df).sum(1)
        bnd[:, 1 + d] += (T * np.abs(df)).sum(1)
        bnd[:, 1 + D + d] += (T * df * df).sum(1)
    return out, np.asarray(sr.gamma(N + 9) * bnd, dtype=np.float64)


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('D', KGRAD_D)
@pytest.mark.parametrize('M', KGRAD_M)
def test_kgrad_matern(engine, M, D, kind):
    """Every N per (M, D): K and K' differ everywhere, accumulation onto non-zero initial krow, col0 = 2 and ldx = D + 3, and the columns
    n >= N of every operand (both panels included) hold the stage sentinel's double: a read of one of them wrecks the sums.  Both Matern
    kinds launch the one kernel; with K' = K it is the RBF reduction."""
    sent = sr_sentinel()
    for N in KGRAD_N:
        o = sr.kron_panel_operands(kind, M, D, N, KGRAD_NC, seed=100 * M + 10 * D + N % 7)
        rs = np.random.RandomState(9000 + 100 * M + 10 * D + N % 7)
        o['Kd'] = rs.randint(4, 8, (M, KGRAD_NC)).astype(np.float64) if kind == 'int' else 3.0 * rs.rand(M, KGRAD_NC)
        ops = {k: o[k].copy() for k in ('B', 'A', 'PdA', 'K', 'Kd', 'gm', 'dq')}
        for a in ops.values():
            a[..., N:] = sent
        args = (ops['B'], ops['A'], ops['PdA'], ops['K'], ops['Kd'], ops['gm'], ops['dq'], o['X'], o['col0'], o['Z'])
        got = engine.test_kron_panel_kgrad_kind('matern32', *args, krow=o['krow0'])
        stage = 'kron-kgrad-matern/%s M=%d D=%d N=%d' % (kind, M, D, N)
        assert np.array_equal(got[:, 1 + 2 * D], o['krow0'][:, 1 + 2 * D]), '%s: the last column of krow was touched' % stage
        assert np.array_equal(got, engine.test_kron_panel_kgrad_kind('matern52', *args, krow=o['krow0']))
        if kind == 'int':
            ref, bnd = _kgrad_ref(*args, krow0=o['krow0'])
            _assert_exact_premise(bnd / sr.gamma(N + 9) + 1)
            _compare(stage, 'krow', got, ref, None, True)
            same = (ops['B'], ops['A'], ops['PdA'], ops['K'], ops['K'], ops['gm'], ops['dq'], o['X'], o['col0'], o['Z'])
            assert np.array_equal(engine.test_kron_panel_kgrad_kind('matern32', *same, krow=o['krow0']),
                                  engine.test_kron_panel_kgrad_kind('rbf', *same, krow=o['krow0'])), '%s: with K\' = K it is not the RBF reduction' % stage
        else:
            ref, bnd = _kgrad_ref(*args, krow0=o['krow0'], dtype=L)
            _compare(stage, 'krow', got, np.asarray(ref, dtype=np.float64), bnd * (1 + 2.0 ** -11), False)
    if kind == 'int':
        print('STAGE-LOG %-12s %-34s bit-equal for N in %s' % ('kron-kgrad-m', 'int M=%d D=%d' % (M, D), list(KGRAD_N)))


def test_kind_hooks_validate_and_leave_the_context_usable(engine):
    from zigp import _lib
    from test_gpu_kron import make_kron_problem
    lib = engine.lib
    assert lib.zigp_test_kron_kbuild_kind(None, 1, 1, 256, 1, 0, 1, 1, None, None, None, 1.0, None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_kbuild_kind(engine.ctx, 3, 1, 256, 1, 0, 1, 1, None, None, None, 1.0, None, None) == _lib.ZIGP_EARG
    assert b'unknown kernel kind' in lib.zigp_last_error(engine.ctx)
    assert lib.zigp_test_kron_kgrad_kind(engine.ctx, 1, 1, 9, 1, 256, 9, 0, *([None] * 10)) == _lib.ZIGP_EARG
    with pytest.raises(ValueError):
        engine.test_kron_panel_kbuild_kind('matern32', np.zeros((4, 2)), 1, np.zeros((3, 2)), 1.0, 1.0, 256)      # col0 + D > ldx
    X, Y, p = make_kron_problem(200, 6, 5, seed=1)
    a = engine.kron_elbo(p, X, Y, jitter=1e-5, need_grad=False)
    engine.test_kron_panel_kbuild_kind('matern52', np.zeros((4, 3)), 1, np.zeros((3, 2)), 1.0, 1.0, 256)
    b = engine.kron_elbo(p, X, Y, jitter=1e-5, need_grad=False)
    assert a[:2] == b[:2]
