"""CPU side of the predictive density (include/zigp.h "predictive density"): the references of tests/density_ref.py pin each other, the
quadrature rule, the degenerate rows, and the boundary of the three entry points.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import density_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = R.EPS


def test_numpy_reference_is_within_4_eps_S_of_the_50_digit_sum():
    """The condition that gives the GPU rule (err_gpu <= 4 err_np + 16 eps S) its meaning: float64 NumPy alone stays under 4 eps S on the
    full grid at 20 nodes (measured: 1.33 at worst), and on the subset at 1, 64 and 256 nodes (0.39, 0.49, 0.50)."""
    for n, full in ((20, True), (1, False), (64, False), (256, False)):
        rows, _, _, err, S = R.onoff_case(n, full)
        r = err / (EPS * S)
        print('n_quad %3d, %3d rows: NumPy err / (eps S) max %.3f' % (n, len(S), r.max()))
        assert len(S) == (675 if full else 60)
        assert r.max() < 4.0
    for lik in ('gaussian', 'bernoulli'):
        _, _, err, S = R.head_case(lik)
        print('%s head, %d rows: NumPy err / (eps S) max %.3f' % (lik, len(S), (err / (EPS * S)).max()))
        assert (err / (EPS * S)).max() < 4.0


def test_subset_covers_every_axis_value():
    for full, sub, k in zip(R.grid(), R.subset(), ('fm', 'fv', 'gm', 'gv', 'y')):
        assert set(sub) == set(full) == set(R.GRID_AXES[k]), k


@pytest.mark.parametrize('n', list(range(1, 65)))
def test_rule_moments(n):
    """sum w = 1, E[x^2] = 1 (n >= 2), E[x^4] = 3 (n >= 3), within 4 n eps (measured: at most 2 eps up to n = 64); the package's rule is
    the reference's, bit for bit"""
    from zigp.quadrature import gauss_hermite
    x, w = gauss_hermite(n)
    xr, wr = R.rule(n)
    assert np.array_equal(x, xr) and np.array_equal(w, wr) and np.all(w > 0)
    tol = 4 * n * EPS
    assert abs(w.sum() - 1.0) <= tol
    if n >= 2:
        assert abs(np.sum(w * x ** 2) - 1.0) <= tol
    if n >= 3:
        assert abs(np.sum(w * x ** 4) - 3.0) <= 3 * tol
    with pytest.raises(ValueError):
        gauss_hermite(0)


def test_rule_of_256_nodes_has_only_positive_weights():
    from zigp.quadrature import gauss_hermite
    x, w = gauss_hermite(256)
    assert x.size == w.size == 256 and np.all(w > 0) and np.all(np.isfinite(np.log(w)))


def test_degenerate_rows():
    """gv = 0: every node sits on gm, so logp is the closed form at link(gm); fv = gv = 0: the plain Gaussian in the noise variance.
    Both within 8 eps S."""
    fm, fv, gm, gv, y = R.grid()
    x, w = R.rule(20)
    z = np.zeros_like(gv)
    S = R.scales(fm, fv, gm, z, y, R.NOISE, x, w)
    ph = R.link_np(gm)
    s = R.NOISE + ph * ph * fv
    closed = -0.5 * (R.LOG_2PI + np.log(s)) - 0.5 * np.square(y - ph * fm) / s
    assert np.all(np.abs(R.logp_np(fm, fv, gm, z, y, R.NOISE, x, w) - closed) <= 8 * EPS * S)
    S0 = R.scales(fm, z, gm, z, y, R.NOISE, x, w)
    plain = -0.5 * (R.LOG_2PI + np.log(R.NOISE)) - 0.5 * np.square(y - ph * fm) / R.NOISE
    assert np.all(np.abs(R.logp_np(fm, z, gm, z, y, R.NOISE, x, w) - plain) <= 8 * EPS * S0)
    # slightly negative variances count as zero
    neg = np.full_like(gv, -1e-18)
    assert np.array_equal(R.logp_np(fm, neg, gm, neg, y, R.NOISE, x, w), R.logp_np(fm, z, gm, z, y, R.NOISE, x, w))


NEW = ('zigp_density_rows', 'zigp_predict_density', 'zigp_predict_density_device')


def test_boundary_null_context_and_signatures():
    """every new entry point returns ZIGP_EARG on a NULL context (before it looks at anything else), and its binding has as many
    arguments as the declaration in include/zigp.h"""
    from zigp import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert decl, name
        assert len(args) == decl.group(1).count(',') + 1 == len(getattr(lib, name).argtypes), name
        assert res is C.c_int
        sentinel = np.full(4, 7.0)
        call = [None] * len(args)
        for i, t in enumerate(args):
            if t in (C.c_int32, C.c_int64):
                call[i] = 1
            elif t is C.c_double:
                call[i] = 1.0
        call[-1], call[-2] = sentinel.ctypes.data, sentinel.ctypes.data
        assert getattr(lib, name)(*call) == _lib.ZIGP_EARG, name
        assert np.all(sentinel == 7.0)
    assert _lib.DENSITY_MAX_QUAD == int(re.search(r'#define ZIGP_DENSITY_MAX_QUAD (\d+)', hdr).group(1)) == 256


def test_predict_y_composes_on_a_stubbed_engine():
    """ymean = gfmean and yvar = (gfvar + gfmeanu) + noise, the two additions in that order: rows chosen so that the other association
    rounds differently"""
    from onoffgpf.OnOffSVGP import OnOffSVGP, JITTER
    from onoffgpf.param import Param
    rs = np.random.RandomState(3)
    rows = rs.rand(9, 200)
    noise = 0.0123456789
    a, b = (rows[1] + rows[2]) + noise, rows[1] + (rows[2] + noise)
    assert np.any(a != b)
    seen = {}

    class Engine:
        def predict(self, p, Xnew, jitter):
            seen.update(p=p, X=Xnew, jitter=jitter)
            return rows

    class Lik:
        variance = Param(np.array([noise]))

    m = OnOffSVGP.__new__(OnOffSVGP)
    m._engine, m.likelihood, m._values = Engine(), Lik(), lambda: 'values'
    Xnew = rs.rand(200, 2)
    ymean, yvar = m.predict_y(Xnew)
    assert seen['p'] == 'values' and seen['X'] is not None and seen['jitter'] == JITTER
    assert ymean.shape == yvar.shape == (200, 1)
    assert np.array_equal(ymean[:, 0], rows[0]) and np.array_equal(yvar[:, 0], a)
