"""CPU side of the mode-centred predictive density (include/zigp.h "centred"): the references of
tests/density_centred_ref.py pin each other and the integral, the degenerate rows, the boundary of the three entry points and the
Python-side refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import density_ref as R
import density_centred_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = R.EPS

# max |error| (nats) of the mode-centred NumPy sum against integral_mp on the 162 stress rows, as tools/density_centred_accuracy.py
# logged them (profiles/density_centred_accuracy.log: 4.35e-02, 9.93e-03, 3.55e-03), rounded up in the third digit; no margin on top
LOGGED_MAX = {20: 4.36e-2, 32: 9.94e-3, 64: 3.56e-3}


def _closed(fm, fv, gm, y, noise):
    ph = R.link_np(gm)
    s = noise + ph * ph * np.maximum(fv, 0.0)
    return -0.5 * (R.LOG_2PI + np.log(s)) - 0.5 * np.square(y - ph * fm) / s


def test_numpy_sum_is_within_4_eps_S_of_the_50_digit_sum():
    """What gives the GPU rule (err_gpu <= 4 err_np + 16 eps S) its meaning: float64 NumPy alone, at centre_np's own (zhat, tau), stays
    under 4 eps S_centred on the 675-row grid at 20 nodes (measured: 0.47 at worst) and on the 60-row subset at 1, 64 and 256 nodes
    (1.67, 0.25, 0.24)."""
    for kind, n in (('grid', 20), ('subset', 1), ('subset', 64), ('subset', 256)):
        rows, z, t, ru, truth, err, S = Q.sum_case(kind, n)
        r = err / (EPS * S)
        print('centred n_quad %3d, %3d rows: NumPy err / (eps S) max %.3f' % (n, len(S), r.max()))
        assert len(S) == (675 if kind == 'grid' else 60)
        assert np.all(np.isfinite(z)) and np.all(t > 0) and np.all(t <= Q.TAU_MAX)
        assert r.max() < 4.0


def test_degenerate_rows():
    """gv = 0 and gv = -1e-18: zhat = 0 and tau = 1 EXACTLY, logp within 8 eps S of the closed form at link(gm); fv = gv = 0: within
    8 eps S of the plain Gaussian in the noise variance"""
    fm, fv, gm, gv, y = R.grid()
    ru = Q.rule(20)
    for g0 in (np.zeros_like(gv), np.full_like(gv, -1e-18)):
        for f0 in (fv, np.zeros_like(fv), np.full_like(fv, -1e-18)):
            rows = (fm, f0, gm, g0, y)
            z, t = Q.centre_np(*rows, Q.NOISE)
            assert np.all(z == 0.0) and np.all(t == 1.0)
            S = Q.scales_centred(rows, z, t, ru)
            lp = Q.logp_centred_np(rows, z, t, ru)
            assert np.all(np.abs(lp - _closed(fm, f0, gm, y, Q.NOISE)) <= 8 * EPS * S)
            if not np.any(f0 > 0):
                ph = R.link_np(gm)
                plain = -0.5 * (R.LOG_2PI + np.log(Q.NOISE)) - 0.5 * np.square(y - ph * fm) / Q.NOISE
                assert np.all(np.abs(lp - plain) <= 8 * EPS * S)


def test_rows_with_fm_zero_are_finite():
    fm, fv, gm, gv, y = R.grid()
    keep = fm == 0.0
    assert keep.sum() == 135
    rows = tuple(a[keep] for a in (fm, fv, gm, gv, y))
    z, t = Q.centre_np(*rows, Q.NOISE)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(t)) and np.all(t > 0)
    for n in (1, 20):
        assert np.all(np.isfinite(Q.logp_centred_np(rows, z, t, Q.rule(n))))


def test_one_node_is_the_laplace_approximation():
    """x = (0), w = (1): the sum is log tau + F(zhat), within 8 eps S"""
    rows = R.grid()
    fm, fv, gm, gv, y = rows
    z, t = Q.centre_np(*rows, Q.NOISE)
    ru = Q.rule(1)
    assert ru[0].size == 1 and ru[0][0] == 0.0 and abs(ru[1][0] - 1.0) <= 2 * EPS
    F = Q._eval(z, fm, np.maximum(fv, 0.0), gm, np.sqrt(np.maximum(gv, 0.0)), y, Q.NOISE)[0]
    S = Q.scales_centred(rows, z, t, ru)
    assert np.all(np.abs(Q.logp_centred_np(rows, z, t, ru) - (np.log(t) + F)) <= 8 * EPS * S)


def test_search_ends_at_a_local_maximum_on_the_grids():
    """F'(zhat) vanishes to rounding in units of 1 / tau wherever the curvature is negative, and no row hits the iteration cap with a
    long step left"""
    for kind in ('grid', 'stress'):
        rows, z, t = Q.centre_case(kind)
        fm, fv, gm, gv, y = rows
        F, F1, F2 = Q._eval(z, fm, np.maximum(fv, 0.0), gm, np.sqrt(np.maximum(gv, 0.0)), y, Q.NOISE)
        curved = F2 < 0
        assert curved.all(), kind
        assert np.max(np.abs(F1 / -F2) * np.sqrt(-F2)) <= 1e-6, kind      # the Newton step that is left, in units of 1 / sqrt(-F'')


def test_stress_integrals_in_golden_are_integral_mp():
    """tests/golden/density_centred_stress_integral.txt holds what integral_mp gives: a sample of rows recomputed (every 23rd: all three
    gv, the far-tail row fm = 10, gm = 1.5, gv = 1e-3, y = 0 among them)"""
    import mpmath as mp
    rows, z, t = Q.centre_case('stress')
    gold = Q.stress_integral()
    idx = list(range(0, 162, 23)) + [int(np.nonzero((rows[0] == 10) & (rows[1] == 1e-4) & (rows[2] == 1.5) & (rows[3] == 1e-3) & (rows[4] == 0))[0][0])]
    again = Q.integral_mp(tuple(a[idx] for a in rows), z[idx], t[idx])
    with mp.workdps(30):
        for i, v in zip(idx, again):
            assert abs(v - gold[i]) <= mp.mpf(10) ** -20 * (1 + abs(v)), i
    # the documented far-tail row: the window gm +- 12 sg of tools/density_accuracy.py gave -3814, the integral is far above it
    assert float(gold[idx[-1]]) > -3000


@pytest.mark.parametrize('n', [20, 32, 64])
def test_reference_against_the_integral_on_the_stress_grid(n):
    """max |error| of the mode-centred sum on the 162 stress rows is no worse than what tools/density_centred_accuracy.py logged, and
    on every row where the gm-centred sum is more than 1 nat off, the centred sum is closer"""
    rows, z, t = Q.centre_case('stress')
    truth = Q.stress_integral()
    ru = Q.rule(n)
    e1 = R.err_to(truth, Q.logp_centred_np(rows, z, t, ru))
    e0 = R.err_to(truth, R.logp_np(*rows, Q.NOISE, *ru))
    print('n_quad %d: mode-centred median %.2e max %.2e, gm-centred median %.2e max %.2e, %d rows more than 1 nat off'
          % (n, np.median(e1), e1.max(), np.median(e0), e0.max(), int(np.sum(e0 > 1.0))))
    assert e1.max() <= LOGGED_MAX[n]
    far = e0 > 1.0
    assert far.sum() >= 10 and np.all(e1[far] < e0[far])


NEW = ('zigp_density_rows_centred', 'zigp_predict_density_centred', 'zigp_predict_density_centred_device')


def test_boundary_null_context_and_signatures():
    """every new entry point returns ZIGP_EARG on a NULL context (before it looks at anything else), its binding has as many arguments
    as the declaration in include/zigp.h -- those of its counterpart plus centre2 -- and there is no lik argument"""
    from zigp import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert decl, name
        assert len(args) == decl.group(1).count(',') + 1 == len(getattr(lib, name).argtypes), name
        assert res is C.c_int and 'centre2' in decl.group(1).split(',')[-1] and 'lik' not in decl.group(1)
        old = _lib.SIGNATURES[name.replace('_centred', '')][1]
        if name == 'zigp_density_rows_centred':
            old = old[:1] + old[2:]                      # no lik
        assert list(args[:-1]) == list(old), name
        sentinel = np.full(4, 7.0)
        call = [None] * len(args)
        for i, t in enumerate(args):
            if t in (C.c_int32, C.c_int64):
                call[i] = 1
            elif t is C.c_double:
                call[i] = 1.0
        call[-1] = call[-2] = call[-3] = sentinel.ctypes.data
        assert getattr(lib, name)(*call) == _lib.ZIGP_EARG, name
        assert np.all(sentinel == 7.0)


def test_python_side_refusals():
    """an unknown centre names both choices; centre='mode' on a closed-form head is refused; both before the library is touched"""
    from zigp.engine import DenseEngine
    e = DenseEngine.__new__(DenseEngine)          # no context: a refusal that reached the library would fail on the missing attribute
    z = np.zeros(4)
    for call in (lambda c: e.density_rows('onoff', z, z, z, z, z, 0.01, centre=c),
                 lambda c: e.predict_density({}, z.reshape(4, 1), z, centre=c),
                 lambda c: e.predict_density_device({}, None, None, centre=c)):
        with pytest.raises(ValueError, match="'mean'.*'mode'"):
            call('median')
        with pytest.raises(ValueError, match="'mean'.*'mode'"):
            call(None)
    for lik in ('gaussian', 'bernoulli'):
        with pytest.raises(ValueError, match='closed form'):
            e.density_rows(lik, z, z, None, None, z, 0.01, centre='mode')


def test_model_passes_centre_on_only_when_it_is_not_the_default():
    from onoffgpf.OnOffSVGP import OnOffSVGP, JITTER
    seen = []

    class Engine:
        def predict_density(self, p, Xnew, Ynew, **kw):
            seen.append(kw)
            return np.arange(12.0).reshape(3, 4), 0.0

    m = OnOffSVGP.__new__(OnOffSVGP)
    m._engine, m._values = Engine(), lambda: 'values'
    X, Y = np.zeros((4, 1)), np.zeros((4, 1))
    assert m.predict_density(X, Y).shape == (4, 1)
    m.predict_density(X, Y, n_quad=20, centre='mean')
    m.predict_density(X, Y, centre='mode')
    assert seen == [dict(jitter=JITTER, n_quad=64), dict(jitter=JITTER, n_quad=20), dict(jitter=JITTER, n_quad=64, centre='mode')]
