"""CPU side of the predictive scores (include/zigp.h "predictive scores"): the references of tests/score_ref.py pin each other and their
own floors, the closed form of the CRPS is checked against its defining integral, the degenerate rows, the boundary of the three entry
points and the model methods on a stubbed engine.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import density_ref as R
import score_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = R.EPS


def test_numpy_references_stay_under_their_floors():
    """What gives the GPU rule (err_gpu <= 4 err_np + 16 eps S) its meaning, on density_ref.subset() at 20 nodes with t = y: float64 NumPy
    alone is within 8 eps S_F of the 50-digit CDF in either tail and within 8 eps S_C of the 50-digit CRPS, the bisection's residual is within
    8 (eps S_F + ulp pdf) at every level, and the starting bracket holds the root.  The measured maxima are printed
    (profiles/score_parity.log)."""
    rows, (x, w), truth, err, scale = S.cdf_case(20, 'subset')
    for k, tail in enumerate(('F', 'SF')):
        ok = scale[k] > 0
        r = err[k][ok] / (EPS * scale[k][ok])
        print('CDF %-2s, %d rows: NumPy err / (eps S_F) max %.3f' % (tail, len(err[k]), r.max()))
        assert r.max() <= S.FLOOR
        assert np.all(err[k][~ok] == 0.0)          # a tail that underflows to 0 is an exact 0
    _, _, _, err_c, S_C = S.crps_case(20, 'subset')
    crps = S.crps_np(*rows, S.NOISE, x, w)
    print('CRPS, %d rows: NumPy err / (eps S_C) max %.3f, S_C / CRPS max %.2f' % (len(S_C), (err_c / (EPS * S_C)).max(), (S_C / crps).max()))
    assert (err_c / (EPS * S_C)).max() <= S.FLOOR and np.all(crps > 0)
    for p in S.FLOOR_LEVELS:
        t, res, unit = S.quantile_case(20, 'subset', p)
        lo, hi = S.bracket(*rows[:4], S.NOISE, x, w, p)
        print('quantile p = %-12.10g: residual / (eps S_F + ulp pdf) max %.3f' % (p, (res / unit).max()))
        assert (res / unit).max() <= S.FLOOR
        assert np.all((lo <= t) & (t <= hi))


def test_crps_closed_form_is_the_integral_of_the_squared_cdf_error():
    """CRPS = int (F(t) - 1[t >= y])^2 dt, by mpmath.quad on three rows (a bulk row, a zero spike, gv = 9): this checks the formula, not the
    arithmetic.  1e-10 relative."""
    import mpmath as mp
    x, w = R.rule(20)
    cases = [(0.5, 0.1, 1.5, 0.3, 0.4), (3.0, 0.1, -6.0, 1e-3, 0.0), (3.0, 4.0, 0.0, 9.0, 3.0)]
    for fm, fv, gm, gv, y in cases:
        row = tuple(np.array([v]) for v in (fm, fv, gm, gv, y))
        closed = S.crps_mp(*row, S.NOISE, x, w)[0]
        with mp.workdps(20):
            mu, s = S._mp_table(mp, fm, fv, gm, gv, S.NOISE, [mp.mpf(float(v)) for v in x])
            ws, sds = [mp.mpf(float(v)) for v in w], [mp.sqrt(v) for v in s]

            def F(t):
                return mp.fsum(wk * mp.ncdf((t - m) / d) for wk, m, d in zip(ws, mu, sds))
            sd = max(sds)          # the integrand is below exp(-15^2) outside [min mu - 15 sd, max mu + 15 sd]; the components' centres break it up
            pts = sorted(set([min(mu + [mp.mpf(y)]) - 15 * sd, mp.mpf(y), max(mu + [mp.mpf(y)]) + 15 * sd] + mu))
            below = [t for t in pts if t <= y]
            above = [t for t in pts if t >= y]
            integral = mp.quad(lambda t: F(t) ** 2, below) + mp.quad(lambda t: (1 - F(t)) ** 2, above)
            rel = abs(integral - closed) / closed
        print('row %s: closed form %.15g, integral %.15g, rel %.2e' % ((fm, fv, gm, gv, y), float(closed), float(integral), float(rel)))
        assert rel < 1e-10


def test_degenerate_rows():
    """gv = 0: one Gaussian at link(gm); fv = gv = 0: one Gaussian in the noise variance.  Variances of -1e-18 count as 0: equal bits."""
    fm, fv, gm, gv, y = R.subset()
    x, w = R.rule(20)
    z, neg = np.zeros_like(gv), np.full_like(gv, -1e-18)
    for fvv in (fv, z):
        ph = R.link_np(gm)
        mu, s = ph * fm, S.NOISE + ph * ph * fvv
        zz = (y - mu) / np.sqrt(s)
        F, SF = S.cdf_np(fm, fvv, gm, z, y, S.NOISE, x, w)
        SFl, SFu = S.cdf_scales(fm, fvv, gm, z, y, S.NOISE, x, w)
        assert np.all(np.abs(F - S.Phi(zz)) <= 8 * EPS * SFl) and np.all(np.abs(SF - S.Phi(-zz)) <= 8 * EPS * SFu)
        closed = S.A(y - mu, s) - np.sqrt(s / np.pi)
        SC = S.crps_scale(fm, fvv, gm, z, y, S.NOISE, x, w)
        assert np.all(np.abs(S.crps_np(fm, fvv, gm, z, y, S.NOISE, x, w) - closed) <= 8 * EPS * SC)
        lo, hi = S.bracket(fm, fvv, gm, z, S.NOISE, x, w, 0.05)
        assert np.array_equal(lo, hi)          # every component is the same one: the bracket is the quantile
    for a, b in (((fm, z, gm, gv), (fm, neg, gm, gv)), ((fm, fv, gm, z), (fm, fv, gm, neg)), ((fm, z, gm, z), (fm, neg, gm, neg))):
        assert np.array_equal(S.cdf_np(*a, y, S.NOISE, x, w), S.cdf_np(*b, y, S.NOISE, x, w))
        assert np.array_equal(S.crps_np(*a, y, S.NOISE, x, w), S.crps_np(*b, y, S.NOISE, x, w))
        assert np.array_equal(S.quantile_np(*a, S.NOISE, x, w, 0.05), S.quantile_np(*b, S.NOISE, x, w, 0.05))


NEW = ('zigp_score_rows', 'zigp_predict_scores', 'zigp_predict_scores_device')


def test_boundary_null_context_and_signatures():
    """every new entry point returns ZIGP_EARG on a NULL context (before it looks at anything else) with its outputs untouched, and its
    binding has as many arguments as the declaration in include/zigp.h"""
    from zigp import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert decl, name
        assert len(args) == decl.group(1).count(',') + 1 == len(getattr(lib, name).argtypes) == (18 if name == 'zigp_score_rows' else 16), name
        assert res is C.c_int
        sentinel = np.full(8, 7.0)
        call = [None] * len(args)
        for i, t in enumerate(args):
            if t in (C.c_int32, C.c_int64):
                call[i] = 1
            elif t is C.c_double:
                call[i] = 1.0
        for k in range(1, 5):          # cdf2, quant, crps, crps_sum
            call[-k] = sentinel.ctypes.data
        assert getattr(lib, name)(*call) == _lib.ZIGP_EARG, name
        assert np.all(sentinel == 7.0)
    assert _lib.SCORE_MAX_LEVELS == int(re.search(r'#define ZIGP_SCORE_MAX_LEVELS (\d+)', hdr).group(1)) == 16


def test_model_methods_compose_on_a_stubbed_engine():
    """predict_cdf, predict_quantiles and predict_crps hand the model's values, the inputs and the jitter to predict_scores and reshape what
    comes back: (N,1) columns, and (N, L) quantiles from the engine's (L, N)"""
    from onoffgpf.OnOffSVGP import OnOffSVGP, JITTER
    rs = np.random.RandomState(5)
    N = 50
    res = {'cdf': rs.rand(N), 'sf': rs.rand(N), 'quantiles': rs.rand(3, N), 'crps': rs.rand(N), 'crps_sum': 1.0}
    seen = []

    class Engine:
        def predict_scores(self, p, Xnew, Ynew=None, **kw):
            seen.append((p, Xnew, Ynew, kw))
            out = dict(res)
            if Ynew is None or not kw.get('cdf', True):
                out['cdf'] = out['sf'] = None
            if Ynew is None or not kw.get('crps', True):
                out['crps'] = out['crps_sum'] = None
            if not len(kw.get('levels', ())):
                out['quantiles'] = None
            return out

    m = OnOffSVGP.__new__(OnOffSVGP)
    m._engine, m._values = Engine(), lambda: 'values'
    Xnew, Ynew = rs.rand(N, 2), rs.rand(N, 1)
    F, SF = m.predict_cdf(Xnew, Ynew, n_quad=20)
    assert F.shape == SF.shape == (N, 1) and np.array_equal(F[:, 0], res['cdf']) and np.array_equal(SF[:, 0], res['sf'])
    p, X, Y, kw = seen[-1]
    assert p == 'values' and np.array_equal(X, Xnew) and np.array_equal(Y, Ynew) and kw['jitter'] == JITTER and kw['n_quad'] == 20
    q = m.predict_quantiles(Xnew, (0.05, 0.5, 0.95))
    assert q.shape == (N, 3) and np.array_equal(q, res['quantiles'].T)
    assert seen[-1][2] is None and tuple(seen[-1][3]['levels']) == (0.05, 0.5, 0.95) and seen[-1][3]['n_quad'] == 64
    c = m.predict_crps(Xnew, Ynew)
    assert c.shape == (N, 1) and np.array_equal(c[:, 0], res['crps'])
    assert m.predict_quantiles(Xnew, ()).shape == (N, 0)
