"""References of the mode-centred predictive density (include/zigp.h "predictive density", centred), shared by
test_cpu_density_centred.py, test_gpu_density_centred.py and tools/density_centred_accuracy.py.

Per row, sg = sqrt(max(gv, 0)), z = (g - gm) / sg and
    F(z) = -z^2 / 2 + l(link(gm + sg z)),   l(u) = -0.5 log(2 pi s(u)) - 0.5 (y - u fm)^2 / s(u),   s(u) = noise + u^2 max(fv, 0).
* `centre_np`         (zhat, tau): the safeguarded Newton search for a local maximiser of F from z = 0, the formulas in the order the
                      kernel k_density_rows<ZIGP_LIK_ONOFF, true> writes them, and tau = 1 / sqrt(-F''(zhat)) clamped to TAU_MAX;
* `logp_centred_np`   logsumexp_i [ log w_i + x_i^2 / 2 + log tau - z_i^2 / 2 + l(link(gm + sg z_i)) ],  z_i = zhat + tau x_i, in float64;
* `logp_centred_mp`   the same finite sum on the same float64 inputs (zhat and tau included) at 50 digits;
* `scales_centred`    density_ref.scales extended by the new terms: per node, on top of |l_i|, the link, the node g_i = gm + sg z_i and
                      the quadratic form, the summands |log w_i|, x_i^2 / 2, |log tau|, z_i^2 / 2, the node z_i = zhat + tau x_i inside
                      z_i^2 / 2 (|z_i| (|zhat| + |tau x_i|)) and inside g_i (|dl_i/dg_i| sg (|zhat| + |tau x_i|));
* `integral_mp`       the integral itself, mpmath.quad at 30 digits over [min(gm - 12 sg, -9), max(gm + 12 sg, 9)] in g (wide enough
                      for mass that sits far from gm), broken at 65 even points and at zhat + m tau, m in {0, +-1, +-3, +-10, +-30}.
The stress grid of tools/density_accuracy.py and a cache of its integrals live here too.
"""
import functools
import itertools
import os

import numpy as np

import density_ref as R

EPS = R.EPS
C1 = R.C1
NOISE = R.NOISE
LOG_2PI = R.LOG_2PI
INV_SQRT_2PI = 0.39894228040143267794
MAX_ITER, MAX_HALVE, TAU_MAX = 60, 30, 1.5     # csrc/zigp_density.hip DC_MAX_ITER, DC_MAX_HALVE, DC_TAU_MAX
SG_FLOOR = 1e-3                                # a step is at most one unit of g: 1 / max(sg, SG_FLOOR) in z
FREE_STEP, STOP_STEP = 1e-4, 1e-9              # in units of 1 / sqrt(-F''): below FREE_STEP a Newton step is taken unchecked, at STOP_STEP the search ends
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _erf(v):
    from scipy.special import erf
    return erf(v)


def _eval(z, fm, fvp, gm, sg, y, noise, link=None):
    """F, F', F'' at z (arrays), the kernel's dc_eval; `link` replaces the link value (the +-1 ulp twin of the centre tier)"""
    g = gm + sg * z
    ph = 0.5 * (1.0 + _erf(g * 0.70710678118654752440)) * C1 + R.C0
    if link is not None:
        ph = link(ph)
    dph = C1 * INV_SQRT_2PI * np.exp(-0.5 * g * g)
    s = noise + ph * ph * fvp
    r = y - ph * fm
    q = ph * fvp
    with np.errstate(all='ignore'):
        F = -0.5 * z * z + (-0.5 * (LOG_2PI + np.log(s)) - 0.5 * (r * r) / s)
        l1 = (r * fm - q) / s + (r * r) * q / (s * s)
        l2 = -(fvp + fm * fm) / s + (2.0 * q * q - 4.0 * r * fm * q + (r * r) * fvp) / (s * s) - 4.0 * (r * r) * (q * q) / (s * s * s)
        F1 = -z + sg * l1 * dph
        F2 = -1.0 + sg * sg * (l2 * dph * dph - g * l1 * dph)
    return F, F1, F2


def centre_np(fm, fv, gm, gv, y, noise, link=None):
    """(zhat, tau) per row.  Vectorised over the rows; every row follows the scalar algorithm of the kernel:
         z = 0; repeat at most MAX_ITER times:
           h = -F''(z); step = F'(z) / h if h > 0 else sign(F') cap; step clamped to +-cap, cap = 1 / max(sg, SG_FLOOR)
           a Newton step (h > 0) of at most FREE_STEP / sqrt(h) is taken as it is, and the search ends when it is at most STOP_STEP / sqrt(h)
           any other step is halved (at most MAX_HALVE times) until F does not decrease; if it still does, or the step is 0, the search ends
         tau = min(1 / sqrt(h), TAU_MAX) if h > 0 else 1."""
    fm, fv, gm, gv, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (fm, fv, gm, gv, y))
    sg, fvp = np.sqrt(np.maximum(gv, 0.0)), np.maximum(fv, 0.0)
    cap = 1.0 / np.maximum(sg, SG_FLOOR)
    z = np.zeros_like(fm)
    F, F1, F2 = _eval(z, fm, fvp, gm, sg, y, noise, link)
    live = np.ones(z.shape, dtype=bool)
    for _ in range(MAX_ITER):
        if not live.any():
            break
        h = -F2
        newton = h > 0.0
        with np.errstate(all='ignore'):
            step = np.where(newton, F1 / h, np.where(F1 > 0.0, cap, np.where(F1 < 0.0, -cap, 0.0)))
            step = np.minimum(np.maximum(step, -cap), cap)
            unit = np.where(newton, 1.0 / np.sqrt(np.where(newton, h, 1.0)), 0.0)
        free = live & newton & (np.abs(step) <= FREE_STEP * unit)
        stop = free & (np.abs(step) <= STOP_STEP * unit)
        live = live & (step != 0.0) & ~np.isnan(step)
        accepted = free.copy()
        zn, Fn, F1n, F2n = z + step, F.copy(), F1.copy(), F2.copy()
        e = _eval(zn, fm, fvp, gm, sg, y, noise, link)
        Fn, F1n, F2n = (np.where(free, a, b) for a, b in zip(e, (Fn, F1n, F2n)))
        trying = live & ~free
        for _ in range(MAX_HALVE + 1):
            if not trying.any():
                break
            ok = trying & (e[0] >= F)
            Fn, F1n, F2n = (np.where(ok, a, b) for a, b in zip(e, (Fn, F1n, F2n)))
            accepted |= ok
            trying &= ~ok
            step = np.where(trying, 0.5 * step, step)
            zn = np.where(trying, z + step, zn)
            e = _eval(zn, fm, fvp, gm, sg, y, noise, link)
        move = live & accepted
        z, F, F1, F2 = np.where(move, zn, z), np.where(move, Fn, F), np.where(move, F1n, F1), np.where(move, F2n, F2)
        live = move & ~stop
    h = -F2
    with np.errstate(all='ignore'):
        tau = np.where(h > 0.0, np.minimum(1.0 / np.sqrt(np.where(h > 0.0, h, 1.0)), TAU_MAX), 1.0)
    return z, tau


def _terms_centred_np(fm, fv, gm, gv, y, noise, zhat, tau, x, w):
    """(N, n) arrays l, Phi, s, res, g, z of the definition"""
    fm, fv, gm, gv, y, zhat, tau = (np.asarray(a, dtype=np.float64).reshape(-1, 1) for a in (fm, fv, gm, gv, y, zhat, tau))
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    sg = np.sqrt(np.maximum(gv, 0.0))
    z = zhat + tau * x
    g = gm + sg * z
    ph = R.link_np(g)
    s = noise + ph * ph * np.maximum(fv, 0.0)
    res = y - ph * fm
    l = ((np.log(np.asarray(w, dtype=np.float64)).reshape(1, -1) + 0.5 * x * x) + np.log(tau)) - 0.5 * z * z \
        + (-0.5 * (LOG_2PI + np.log(s)) - 0.5 * res * res / s)
    return l, ph, s, res, g, z


def logp_centred_np(rows, zhat, tau, rule, noise=NOISE):
    from scipy.special import logsumexp
    return logsumexp(_terms_centred_np(*rows, noise, zhat, tau, *rule)[0], axis=1)


def scales_centred(rows, zhat, tau, rule, noise=NOISE):
    x, w = rule
    l, ph, s, res, g, z = _terms_centred_np(*rows, noise, zhat, tau, x, w)
    fm, fv, gm, gv = (np.asarray(a, dtype=np.float64).reshape(-1, 1) for a in rows[:4])
    zhat, tau = (np.asarray(a, dtype=np.float64).reshape(-1, 1) for a in (zhat, tau))
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    fvp, sg = np.maximum(fv, 0.0), np.sqrt(np.maximum(gv, 0.0))
    rho = np.exp(l - np.max(l, axis=1, keepdims=True))
    rho /= rho.sum(axis=1, keepdims=True)
    dl_dph = -ph * fvp / s + res * fm / s + res * res * ph * fvp / (s * s)
    dl_dg = dl_dph * C1 * np.exp(-0.5 * g * g) / np.sqrt(2.0 * np.pi)
    zparts = np.abs(zhat) + np.abs(tau * x)
    c = np.abs(l) + np.abs(ph * dl_dph) + np.abs(dl_dg) * (np.abs(gm) + np.abs(sg * z)) + res * res / s
    c = c + np.abs(np.log(np.asarray(w, dtype=np.float64))).reshape(1, -1) + 0.5 * x * x + np.abs(np.log(tau)) + 0.5 * z * z \
        + np.abs(z) * zparts + np.abs(dl_dg) * sg * zparts
    return 1.0 + np.sum(rho * c, axis=1)


def logp_centred_mp(rows, zhat, tau, rule, noise=NOISE, dps=50):
    """the finite sum on the same float64 numbers, every operation at `dps` digits; returns mpmath numbers"""
    import mpmath as mp
    x, w = rule
    with mp.workdps(dps):
        xs, lw = [mp.mpf(float(v)) for v in x], [mp.log(mp.mpf(float(v))) for v in w]
        half, l2pi = mp.mpf(1) / 2, mp.log(2 * mp.pi)
        c1, c0, r2 = mp.mpf(C1), mp.mpf(R.C0), mp.sqrt(2)
        out = []
        for a, b, c, d, e, zh, ta in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in tuple(rows) + (zhat, tau))):
            a, b, c, d, e = mp.mpf(float(a)), mp.mpf(max(float(b), 0.0)), mp.mpf(float(c)), mp.mpf(max(float(d), 0.0)), mp.mpf(float(e))
            zh, ta = mp.mpf(float(zh)), mp.mpf(float(ta))
            sg, lt = mp.sqrt(d), mp.log(ta)
            ls = []
            for xi, lwi in zip(xs, lw):
                z = zh + ta * xi
                ph = half * (1 + mp.erf((c + sg * z) / r2)) * c1 + c0
                s = mp.mpf(float(noise)) + ph * ph * b
                res = e - ph * a
                ls.append(lwi + half * xi * xi + lt - half * z * z - half * (l2pi + mp.log(s)) - half * res * res / s)
            m = max(ls)
            out.append(m + mp.log(mp.fsum(mp.exp(v - m) for v in ls)))
        return out


def integral_mp(rows, zhat, tau, noise=NOISE, dps=30, panels=64):
    """log of the integral over g, per row, as mpmath numbers; a row with gv <= 0 has no integral and gets the closed form at link(gm)"""
    import mpmath as mp
    out = []
    with mp.workdps(dps):
        c1, c0, r2 = mp.mpf(C1), mp.mpf(R.C0), mp.sqrt(2)
        for a, b, c, d, e, zh, ta in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in tuple(rows) + (zhat, tau))):
            a, b, c, d, e, s2 = (mp.mpf(float(v)) for v in (a, max(b, 0.0), c, max(d, 0.0), e, noise))
            sg = mp.sqrt(d)

            def lik(g):
                ph = (1 + mp.erf(g / r2)) / 2 * c1 + c0
                s = s2 + ph * ph * b
                return mp.exp(-(e - ph * a) ** 2 / (2 * s)) / mp.sqrt(2 * mp.pi * s)
            if d == 0:
                out.append(mp.log(lik(c)))
                continue
            lo, hi = min(c - 12 * sg, mp.mpf(-9)), max(c + 12 * sg, mp.mpf(9))
            pts = set(mp.linspace(lo, hi, panels + 1))
            for m in (0, 1, -1, 3, -3, 10, -10, 30, -30):
                g = c + sg * (mp.mpf(float(zh)) + m * mp.mpf(float(ta)))
                if lo < g < hi:
                    pts.add(g)
            out.append(mp.log(mp.quad(lambda g: mp.exp(-(g - c) ** 2 / (2 * d)) / mp.sqrt(2 * mp.pi * d) * lik(g), sorted(pts))))
    return out


def ulp_link(seed):
    """a link perturbed by a seeded -1 / 0 / +1 ulp per value (the device-fit tests' idiom): the centre tier's measure of how far
    rounding alone moves the search"""
    rs = np.random.RandomState(seed)

    def f(ph):
        k = rs.randint(-1, 2, size=np.shape(ph))
        return np.where(k > 0, np.nextafter(ph, np.inf), np.where(k < 0, np.nextafter(ph, -np.inf), ph))
    return f


# ---- grids and caches ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stress():
    """the 162 stress rows of tools/density_accuracy.py (noise 0.01) as five read-only arrays"""
    g = np.array(list(itertools.product((0.5, 3.0, 10.0), (1e-4, 0.1), (-2.0, 0.0, 1.5), (1e-3, 0.3, 9.0), (0.0, 0.4, 3.0))))
    cols = tuple(np.ascontiguousarray(g[:, i]) for i in range(5))
    for c in cols:
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def rule(n):
    x, w = R.rule(n)
    keep = w > 0
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(w[keep])


def case_rows(kind):
    return {'grid': R.grid, 'subset': R.subset, 'stress': stress}[kind]()


@functools.lru_cache(maxsize=None)
def centre_case(kind):
    """(rows, zhat, tau) of centre_np on a named row set"""
    rows = case_rows(kind)
    z, t = centre_np(*rows, NOISE)
    return rows, z, t


@functools.lru_cache(maxsize=None)
def sum_case(kind, n):
    """(rows, zhat, tau, rule, logp_mp, err_np, S) at centre_np's own centre; one 50-digit evaluation per session"""
    rows, z, t = centre_case(kind)
    ru = rule(n)
    truth = logp_centred_mp(rows, z, t, ru)
    return rows, z, t, ru, truth, R.err_to(truth, logp_centred_np(rows, z, t, ru)), scales_centred(rows, z, t, ru)


STRESS_TRUTH = os.path.join(GOLD, 'density_centred_stress_integral.txt')


@functools.lru_cache(maxsize=None)
def stress_integral():
    """the 162 integrals as mpmath numbers: read from tests/golden (30 digits each, written by tools/density_centred_accuracy.py, which
    computes them with integral_mp; test_cpu_density_centred.py recomputes a sample)"""
    import mpmath as mp
    with mp.workdps(50):
        vals = [mp.mpf(line.split()[-1]) for line in open(STRESS_TRUTH) if line.strip() and not line.startswith('#')]
    assert len(vals) == 162
    return vals
