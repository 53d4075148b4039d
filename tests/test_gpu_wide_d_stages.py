"""Stage-level checks of the run-time-D ("wide") kernels of the dense path, input dimensions 9 .. 64, through the stage hooks the D <= 8
kernels are checked with (tests/test_gpu_blocks.py, tests/test_gpu_stages.py): the Kuf panel k_kuf_build_wide against an 80-bit
evaluation with the bound of the D <= 8 kernel, and the sliced Kuf-cotangent reductions k_kgrad_slice against tests/stage_ref.py --
bit for bit on integer operands (sums below 2^53 are exact in any order: every indexing mistake shows, no rounding does) and within
the reference's own bound on random ones.  The wide path has ONE form of the reductions, the per-row one, whatever `exact` says."""
import numpy as np
import pytest

import stage_ref as sr
from test_gpu_stages import _kgrad_operands, _kgrad_check, _assert_exact_premise, sr_sentinel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('D', [9, 15, 16, 17, 24, 33, 64])
def test_kuf_panel_wide(engine, D):
    """Slice remainders 1, 7 and 0, one past a multiple of 16, and the limit; N odd and no multiple of 512, M no multiple of 16.  The bound
    is test_kuf_panel_kernel_golden_kernse_np_and_ulp's: the wide kernel keeps the direct-difference form, so the argument's error stays
    proportional to eps * y (D more additions of terms of one sign)."""
    rng = np.random.RandomState(11 + D)
    eps = np.finfo(np.float64).eps
    N, M = 3001, 70 + D
    X = rng.randn(N, D) * rng.choice([0.3, 3.0, 30.0], size=(N, 1))
    Z = rng.randn(M, D)
    ell = 0.5 + rng.rand(D)
    var = 1.7
    K = engine.test_kuf(X, Z, ell, var)
    L = np.longdouble
    y = np.zeros((M, N), dtype=L)
    for d in range(D):
        t = (Z.astype(L)[:, None, d] - X.astype(L)[None, :, d]) / L(ell[d])
        y += L(0.5) * t * t
    ref = L(var) * np.exp(-y)
    tol = (4.0 + 8.0 * y) * eps * ref + L(5e-324)
    err = np.abs(K.astype(L) - ref)
    print('KUF-WIDE D=%d worst error / bound = %.3g (y in [%.3g, %.3g], %d of %d entries non-zero)'
          % (D, float(np.max(err / tol)), float(y.min()), float(y.max()), int(np.count_nonzero(K)), K.size))
    assert not (err > tol).any(), (D, int((err > tol).sum()))
    assert (K[np.asarray(y > 760)] == 0.0).all() and (K >= 0).all() and np.isfinite(K).all()
    assert float(y.max()) > 800 and float(y.min()) < 100        # the sweep covers ordinary values and reaches past the underflow threshold


def _slices(M, Nc):
    import ctypes as C
    out = (C.c_int64 * 3)()
    from zigp import _lib
    assert _lib.load().zigp_test_kgmom_list(M, Nc, 3, out) == 0
    return int(out[0])


@pytest.mark.parametrize('D', [9, 16, 17, 33, 64])
def test_kgrad_wide_exact(engine, D):
    """Integer operands; the valid columns end inside the chunk (Nc = 1024, 900 valid) and fill it (Nc = 4096: 16 split-K planes).  The
    centred form (integer centre), the sliced per-row form and the reference agree bit for bit."""
    for M in (1, 3, 5, 130):
        for Nc, Nrows, n0 in ((1024, 1500, 600), (4096, 4096, 0)):
            Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, Nrows, 'int', seed=D)
            gm[Nrows - n0:] = 0.0
            gv[Nrows - n0:] = 0.0
            ref, bnd = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=np.ones(D))
            _assert_exact_premise(bnd / sr.gamma(min(Nc, Nrows - n0) + 8))
            S = _slices(M, Nc)
            print('KGRAD-WIDE D=%d M=%d Nc=%d: %d split-K planes' % (D, M, Nc, S))
            assert S > 1
            centred = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, centre=np.ones(D), exact=False)
            per_row = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, exact=True)
            _kgrad_check('kgrad-wide/int D=%d M=%d Nc=%d centred' % (D, M, Nc), centred, ref, None, True)
            _kgrad_check('kgrad-wide/int D=%d M=%d Nc=%d per-row' % (D, M, Nc), per_row, ref, None, True)
            assert not centred[1:, :, 1:1 + 2 * D].any(), 'the centred form adds its moments into slab 0 alone'


@pytest.mark.parametrize('exact', [0, 1], ids=['centred', 'per_row'])
@pytest.mark.parametrize('D', [9, 17, 64])
def test_kgrad_wide_bound(engine, D, exact):
    """Random operands against the extended-precision reference within its own bound; the host's own centre and rule (exact=None) give
    the centred form at this spread, bit for bit."""
    M, Nc, Nrows, n0 = 130, 2048, 2500, 700
    Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, Nrows, 'normal', seed=D)
    gm[Nrows - n0:] = 0.0
    gv[Nrows - n0:] = 0.0
    c = Z.mean(0)
    ref, bnd = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=None if exact else c, dtype=np.longdouble)
    got = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, exact=bool(exact), ell=np.ones(D))
    _kgrad_check('kgrad-wide/normal D=%d %s' % (D, 'per-row' if exact else 'centred'), got, ref, bnd * (1 + 2.0 ** -11), False)
    if not exact:
        auto = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, ell=np.ones(D))
        assert np.array_equal(auto, got), "the host's centre is not the mean inducing input, or its rule chose the per-row form"


@pytest.mark.parametrize('exact', [False, True], ids=['centred', 'per_row'])
def test_kgrad_wide_row_end_inside_the_splits(engine, exact):
    """The last valid column inside the first KG_SPLIT span: three splits have no valid column and add nothing."""
    M, D, Nc, row_end = 7, 19, 1024, 100
    Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, row_end, 'int', seed=4)
    gm[row_end:] = 0.0
    gv[row_end:] = 0.0
    ref, _ = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, 0, centre=np.ones(D))
    got = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, centre=np.ones(D), exact=exact)
    _kgrad_check('kgrad-wide/int row_end=100', got, ref, None, True)
    assert not got[1:].any()


@pytest.mark.parametrize('exact', [False, True], ids=['centred', 'per_row'])
def test_kgrad_wide_sentinel_in_padded_rows_and_masked_columns(engine, exact):
    """For D > 8 the hook fills the padded rows [M, 128 k) of the J' panel with the stage sentinel (1.38e306) in every test of this file;
    here the masked columns of the real rows carry it too, in J' and in K (gm = gv = 0 there, as the point-wise stage leaves them).
    Neither is read and sentinel x 0 is never formed: the result is finite and equals, bit for bit, the run with ordinary numbers in the
    masked columns and the reference."""
    M, D, Nc, Nrows, n0 = 5, 12, 1024, 1500, 600
    Jp, K, alpha, gm, gv, X, Z = _kgrad_operands(M, D, Nc, Nrows, 'int', seed=2)
    gm[Nrows - n0:] = 0.0
    gv[Nrows - n0:] = 0.0
    clean = engine.test_kgrad(Jp, K, alpha, gm, gv, X, Z, n0=n0, centre=np.ones(D), exact=exact)
    Jp2, K2 = Jp.copy(), K.copy()
    Jp2[:, Nrows - n0:] = sr_sentinel()
    K2[:, Nrows - n0:] = sr_sentinel()
    dirty = engine.test_kgrad(Jp2, K2, alpha, gm, gv, X, Z, n0=n0, centre=np.ones(D), exact=exact)
    assert np.all(np.isfinite(dirty)) and np.array_equal(dirty, clean)
    ref, _ = sr.kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=np.ones(D))
    _kgrad_check('kgrad-wide/int sentinel', dirty, ref, None, True)


@pytest.mark.parametrize('exact', [False, True], ids=['centred', 'per_row'])
def test_kgrad_wide_second_call_accumulates(engine, exact):
    M, D, Nc = 5, 11, 1024
    a = _kgrad_operands(M, D, Nc, Nc, 'int', seed=1)
    b = _kgrad_operands(M, D, Nc, Nc, 'int', seed=2)
    first = engine.test_kgrad(*a[:5], a[5], a[6], centre=np.ones(D), exact=exact)
    both = engine.test_kgrad(*b[:5], b[5], b[6], centre=np.ones(D), exact=exact, krow=first)
    ra, _ = sr.kgrad(*a[:5], a[5], a[6], 0, centre=np.ones(D))
    rb, _ = sr.kgrad(*b[:5], b[5], b[6], 0, centre=np.ones(D))
    _kgrad_check('kgrad-wide/int accumulate', both, ra + rb, None, True)
