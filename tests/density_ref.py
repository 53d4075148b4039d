"""References of the predictive density (include/zigp.h "predictive density"), shared by test_cpu_density.py and
test_gpu_density.py.

The OnOff density is DEFINED as a finite sum over a quadrature rule for N(0, 1) (nodes x_i, weights w_i):
    Phi_i = link(gm + sqrt(max(gv, 0)) x_i),  s_i = noise + Phi_i^2 max(fv, 0),
    l_i = log w_i - 0.5 log(2 pi s_i) - 0.5 (y - Phi_i fm)^2 / s_i,   logp = logsumexp_i l_i.
* `logp_np`  that sum in float64 NumPy (SciPy erf and logsumexp),
* `logp_mp`  the same sum on the same float64 table at 50 digits (mpmath): the truth the other two are measured against,
* `scales`   per row, S = 1 + sum_i rho_i c_i: rho_i the terms' responsibilities (softmax of l_i) and
             c_i = |l_i| + |Phi_i dl_i/dPhi_i| + |dl_i/dg_i| (|gm| + |g_i - gm|) + res_i^2 / s_i,  res_i = y - Phi_i fm,
             the sensitivity of the sum to one-ulp errors in the log-term, the link, the node g_i = gm + sg x_i (its two summands) and
             the quadratic form.  eps * S is the unit every error of this file's users is expressed in.
The heads have closed forms; `head_np`, `head_mp`, `head_scales` are the same three for them.  For the Bernoulli head the link term is
(p + 0.5 (1 - 2e-3)) |dl/dp| instead of p |dl/dp|: erf returns a value of magnitude up to 1, so one ulp of ITS result is an absolute
error of 0.5 (1 - 2e-3) eps in p however small p is (p >= 1e-3), on top of the rounding of p itself.
The grids and a cache of the 50-digit results (computed once per session, never written to) live here too.
"""
import functools
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps
C1, C0 = 1.0 - 2.e-3, 1.e-3
NOISE = 0.01
LOG_2PI = float(np.log(2.0 * np.pi))


def rule(n):
    """Gauss-Hermite for N(0, 1): hermegauss nodes, weights / sqrt(2 pi)"""
    x, w = np.polynomial.hermite_e.hermegauss(n)
    return x, w / np.sqrt(2.0 * np.pi)


def link_np(g):
    from scipy.special import erf
    return 0.5 * (1.0 + erf(g / np.sqrt(2.0))) * C1 + C0


def _terms_np(fm, fv, gm, gv, y, noise, x, w):
    """(N, n) arrays l, Phi, s, res, g of the definition"""
    fm, fv, gm, gv, y = (np.asarray(a, dtype=np.float64).reshape(-1, 1) for a in (fm, fv, gm, gv, y))
    g = gm + np.sqrt(np.maximum(gv, 0.0)) * np.asarray(x).reshape(1, -1)
    ph = link_np(g)
    s = noise + ph * ph * np.maximum(fv, 0.0)
    res = y - ph * fm
    l = np.log(np.asarray(w)).reshape(1, -1) - 0.5 * (LOG_2PI + np.log(s)) - 0.5 * res * res / s
    return l, ph, s, res, g


def logp_np(fm, fv, gm, gv, y, noise, x, w):
    from scipy.special import logsumexp
    return logsumexp(_terms_np(fm, fv, gm, gv, y, noise, x, w)[0], axis=1)


def scales(fm, fv, gm, gv, y, noise, x, w):
    l, ph, s, res, g = _terms_np(fm, fv, gm, gv, y, noise, x, w)
    fm, fv, gm = (np.asarray(a, dtype=np.float64).reshape(-1, 1) for a in (fm, fv, gm))
    fvp = np.maximum(fv, 0.0)
    rho = np.exp(l - np.max(l, axis=1, keepdims=True))
    rho /= rho.sum(axis=1, keepdims=True)
    dl_dph = -ph * fvp / s + res * fm / s + res * res * ph * fvp / (s * s)
    dl_dg = dl_dph * C1 * np.exp(-0.5 * g * g) / np.sqrt(2.0 * np.pi)
    c = np.abs(l) + np.abs(ph * dl_dph) + np.abs(dl_dg) * (np.abs(gm) + np.abs(g - gm)) + res * res / s
    return 1.0 + np.sum(rho * c, axis=1)


def logp_mp(fm, fv, gm, gv, y, noise, x, w, dps=50):
    """the same finite sum on the same float64 numbers, every operation at `dps` digits; returns mpmath numbers"""
    import mpmath as mp
    with mp.workdps(dps):
        xs, lw = [mp.mpf(float(v)) for v in x], [mp.log(mp.mpf(float(v))) for v in w]
        half, l2pi = mp.mpf(1) / 2, mp.log(2 * mp.pi)
        c1, c0 = mp.mpf(C1), mp.mpf(C0)        # the float64 constants the code holds
        r2 = mp.sqrt(2)
        out = []
        for a, b, c, d, e in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in (fm, fv, gm, gv, y))):
            a, b, c, d, e = mp.mpf(float(a)), mp.mpf(max(float(b), 0.0)), mp.mpf(float(c)), mp.mpf(max(float(d), 0.0)), mp.mpf(float(e))
            sg = mp.sqrt(d)
            ls = []
            for xi, lwi in zip(xs, lw):
                ph = half * (1 + mp.erf((c + sg * xi) / r2)) * c1 + c0
                s = mp.mpf(float(noise)) + ph * ph * b
                res = e - ph * a
                ls.append(lwi - half * (l2pi + mp.log(s)) - half * res * res / s)
            m = max(ls)
            out.append(m + mp.log(mp.fsum(mp.exp(v - m) for v in ls)))
        return out


def err_to(mp_vals, vals):
    """|vals - mp_vals| as float64, the difference taken at mpmath precision"""
    import mpmath as mp
    with mp.workdps(50):
        return np.array([float(abs(mp.mpf(float(v)) - t)) for v, t in zip(np.asarray(vals).reshape(-1), mp_vals)])


# ---- the heads -------------------------------------------------------------------------------------------------------------------
def head_np(lik, fm, fv, y, noise):
    """(logp, ymean, yvar) in float64"""
    fm, fv, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (fm, fv, y))
    if lik == 'gaussian':
        s = fv + noise
        return -0.5 * (LOG_2PI + np.log(s)) - 0.5 * np.square(y - fm) / s, fm, s
    p = link_np(fm / np.sqrt(1.0 + fv))
    return np.where(y == 1.0, np.log(p), np.log1p(-p)), p, p * (1.0 - p)


def head_mp(lik, fm, fv, y, noise, dps=50):
    import mpmath as mp
    with mp.workdps(dps):
        out = []
        for a, b, e in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in (fm, fv, y))):
            a, b = mp.mpf(float(a)), mp.mpf(float(b))
            if lik == 'gaussian':
                s = b + mp.mpf(float(noise))
                out.append(-(mp.log(2 * mp.pi) + mp.log(s)) / 2 - (mp.mpf(float(e)) - a) ** 2 / (2 * s))
            else:
                p = (1 + mp.erf(a / mp.sqrt(1 + b) / mp.sqrt(2))) / 2 * mp.mpf(C1) + mp.mpf(C0)
                out.append(mp.log(p) if float(e) == 1.0 else mp.log(1 - p))
        return out


def head_scales(lik, fm, fv, y, noise):
    fm, fv, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (fm, fv, y))
    l = head_np(lik, fm, fv, y, noise)[0]
    if lik == 'gaussian':
        return 1.0 + np.abs(l) + np.square(y - fm) / (fv + noise)
    z = fm / np.sqrt(1.0 + fv)
    p = link_np(z)
    dl_dp = np.where(y == 1.0, 1.0 / p, -1.0 / (1.0 - p))
    dl_dz = dl_dp * C1 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    return 1.0 + np.abs(l) + (p + 0.5 * C1) * np.abs(dl_dp) + 2.0 * np.abs(dl_dz * z)


# ---- grids -----------------------------------------------------------------------------------------------------------------------
GRID_AXES = dict(fm=(-3.0, 0.0, 0.5, 3.0, 10.0), fv=(1e-4, 0.1, 4.0), gm=(-6.0, -2.0, 0.0, 1.5, 6.0), gv=(1e-3, 0.3, 9.0), y=(0.0, 0.4, 3.0))


@functools.lru_cache(maxsize=None)
def grid():
    """the 675 rows fm x fv x gm x gv x y as five read-only arrays"""
    rows = np.array(list(itertools.product(*(GRID_AXES[k] for k in ('fm', 'fv', 'gm', 'gv', 'y')))))
    cols = tuple(np.ascontiguousarray(rows[:, i]) for i in range(5))
    for c in cols:
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def subset():
    """60 rows of the grid, every 11th starting at 5 (11 is coprime to every axis length, so all values of every axis occur)"""
    cols = tuple(np.ascontiguousarray(c[5::11][:60]) for c in grid())
    for c in cols:
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def onoff_case(n, full):
    """(rows, rule, logp_mp, err_np, S) of the full grid or the subset at an n-node rule; one 50-digit evaluation per session"""
    rows = grid() if full else subset()
    x, w = rule(n)
    keep = w > 0                                   # (every weight of the rules used here is positive; a zero one would be refused)
    x, w = np.ascontiguousarray(x[keep]), np.ascontiguousarray(w[keep])
    t = logp_mp(*rows, NOISE, x, w)
    return rows, (x, w), t, err_to(t, logp_np(*rows, NOISE, x, w)), scales(*rows, NOISE, x, w)


@functools.lru_cache(maxsize=None)
def head_grid(lik):
    """fm x fv x y; Bernoulli: z = fm / sqrt(1 + fv) reaches +-40 and y is a 0 / 1 label"""
    if lik == 'gaussian':
        axes = (GRID_AXES['fm'], (1e-4, 0.1, 4.0), GRID_AXES['y'])
    else:
        axes = ((-40.0, -8.0, -3.0, -1.0, -0.1, 0.0, 0.3, 1.0, 3.0, 8.0, 40.0), (0.0, 1e-4, 0.1, 4.0), (0.0, 1.0))
    rows = np.array(list(itertools.product(*axes)))
    cols = tuple(np.ascontiguousarray(rows[:, i]) for i in range(3))
    for c in cols:
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def head_case(lik):
    rows = head_grid(lik)
    t = head_mp(lik, *rows, NOISE)
    return rows, t, err_to(t, head_np(lik, *rows, NOISE)[0]), head_scales(lik, *rows, NOISE)
