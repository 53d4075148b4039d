"""References of the predictive scores (include/zigp.h "predictive scores"), shared by test_cpu_score.py and
test_gpu_score.py.  The grids, the rule and the link are density_ref's.

The predictive distribution of an OnOff row is DEFINED as the finite Gaussian mixture over a rule for N(0, 1) (nodes x_k, weights w_k):
    Phi_k = link(gm + sqrt(max(gv, 0)) x_k),  mu_k = Phi_k fm,  s_k = noise + Phi_k^2 max(fv, 0),  z_k(t) = (t - mu_k) / sqrt(s_k)
    F(t) = sum_k w_k Phi(z_k),  SF(t) = sum_k w_k Phi(-z_k),  Phi(z) = erfc(-z / sqrt 2) / 2,  pdf(t) = sum_k w_k phi(z_k) / sqrt(s_k)
    CRPS(y) = sum_i w_i A(y - mu_i, s_i) - 1/2 sum_ij w_i w_j A(mu_i - mu_j, s_i + s_j),  A(m, v) = 2 sqrt(v) phi(m / sqrt v) + m (2 Phi(m / sqrt v) - 1)
* `cdf_np`, `crps_np`, `pdf_np`   those sums in float64 NumPy (SciPy erf / erfc),
* `cdf_mp`, `crps_mp`             the same sums from the same float64 inputs, every operation at 50 digits (mpmath): the truth,
* `quantile_np`                   the root of F = p (p <= 1/2) or SF = 1 - p by bisection from the stated bracket, in float64,
* `cdf_scales`, `crps_scale`      the error scales S_F (either tail) and S_C; eps * S is the unit every error is expressed in:
      S_F = sum_k w_k [Phi(+-z_k) + phi(z_k) c_k],
      c_k = |z_k| + |t| / sqrt(s_k) + |mu_k| / sqrt(s_k) + |Phi_k dz_k/dPhi_k| + |dz_k/dPhi_k dPhi_k/dg| (|gm| + |g_k - gm|),
      dz_k/dPhi_k = -fm / sqrt(s_k) - z_k Phi_k fv / s_k;
      S_C = sum_i w_i |A_i| + 1/2 sum_ij w_i w_j |A_ij|.
The Gaussian head is the one-component case mu = fm, s = fv + noise: `head_*` are the same for it.
A cache of the 50-digit results (computed once per session, never written to) lives here too.
"""
import functools

import numpy as np

import density_ref as R

EPS = R.EPS
NOISE = R.NOISE
SQRT2, SQRT_2PI, SQRT_PI = np.sqrt(2.0), np.sqrt(2.0 * np.pi), np.sqrt(np.pi)
LEVELS = (1e-9, 0.05, 0.5, 0.95, 1.0 - 1e-9)                          # the GPU tests' levels
FLOOR_LEVELS = (1e-9, 1e-3, 0.05, 0.5, 0.95, 1.0 - 1e-3, 1.0 - 1e-9)  # the levels the quantile floor is pinned at
FLOOR = 8.0                                                           # the bar test_cpu_score.py asserts for NumPy alone, in eps S (or eps S + ulp pdf)


def _col(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, 1)


def table(fm, fv, gm, gv, noise, x, w):
    """(N, n) arrays Phi, mu, s, g and the (1, n) weights of the definition"""
    fm, fv, gm, gv = (_col(a) for a in (fm, fv, gm, gv))
    g = gm + np.sqrt(np.maximum(gv, 0.0)) * np.asarray(x, dtype=np.float64).reshape(1, -1)
    ph = R.link_np(g)
    return ph, ph * fm, noise + ph * ph * np.maximum(fv, 0.0), g, np.asarray(w, dtype=np.float64).reshape(1, -1)


def Phi(z):
    from scipy.special import erfc
    return 0.5 * erfc(-z / SQRT2)


def phi(z):
    return np.exp(-0.5 * z * z) / SQRT_2PI


def A(m, v):
    from scipy.special import erf
    sd = np.sqrt(v)
    x = m / sd
    return sd * (2.0 * phi(x) + x * erf(x / SQRT2))


def cdf_np(fm, fv, gm, gv, t, noise, x, w):
    """(F(t), SF(t)) per row, each its own sum"""
    _, mu, s, _, w = table(fm, fv, gm, gv, noise, x, w)
    z = (_col(t) - mu) / np.sqrt(s)
    return np.sum(w * Phi(z), axis=1), np.sum(w * Phi(-z), axis=1)


def pdf_np(fm, fv, gm, gv, t, noise, x, w):
    _, mu, s, _, w = table(fm, fv, gm, gv, noise, x, w)
    sd = np.sqrt(s)
    return np.sum(w * phi((_col(t) - mu) / sd) / sd, axis=1)


def cdf_scales(fm, fv, gm, gv, t, noise, x, w):
    """(S_F of the lower tail, S_F of the upper tail) per row"""
    ph, mu, s, g, w = table(fm, fv, gm, gv, noise, x, w)
    fm, fv, gm, t = _col(fm), np.maximum(_col(fv), 0.0), _col(gm), _col(t)
    sd = np.sqrt(s)
    z = (t - mu) / sd
    dz_dph = -fm / sd - z * ph * fv / s
    dph_dg = R.C1 * phi(g)
    c = np.abs(z) + np.abs(t) / sd + np.abs(mu) / sd + np.abs(ph * dz_dph) + np.abs(dz_dph * dph_dg) * (np.abs(gm) + np.abs(g - gm))
    return np.sum(w * (Phi(z) + phi(z) * c), axis=1), np.sum(w * (Phi(-z) + phi(z) * c), axis=1)


def _crps_parts(fm, fv, gm, gv, y, noise, x, w):
    _, mu, s, _, w = table(fm, fv, gm, gv, noise, x, w)
    a1 = w * A(_col(y) - mu, s)                                                                  # (N, n)
    a2 = w[:, :, None] * w[:, None, :] * A(mu[:, :, None] - mu[:, None, :], s[:, :, None] + s[:, None, :])   # (N, n, n)
    return a1, a2


def crps_np(fm, fv, gm, gv, y, noise, x, w):
    a1, a2 = _crps_parts(fm, fv, gm, gv, y, noise, x, w)
    return a1.sum(axis=1) - 0.5 * a2.sum(axis=(1, 2))


def crps_scale(fm, fv, gm, gv, y, noise, x, w):
    a1, a2 = _crps_parts(fm, fv, gm, gv, y, noise, x, w)
    return np.abs(a1).sum(axis=1) + 0.5 * np.abs(a2).sum(axis=(1, 2))


def bracket(fm, fv, gm, gv, noise, x, w, p):
    """[min_k, max_k] of mu_k + sqrt(s_k) Phi^-1(p) per row"""
    from scipy.special import ndtri
    _, mu, s, _, _ = table(fm, fv, gm, gv, noise, x, w)
    zp = ndtri(p) if p <= 0.5 else -ndtri(1.0 - p)
    c = mu + np.sqrt(s) * zp
    return c.min(axis=1), c.max(axis=1)


def quantile_np(fm, fv, gm, gv, noise, x, w, p):
    """bisection on r(t) = F(t) - p (p <= 1/2) or (1 - p) - SF(t), from the stated bracket until it is one ulp wide; of the two ends, the one
    with the smaller |r|"""
    rows = (fm, fv, gm, gv)
    lower, q = p <= 0.5, (p if p <= 0.5 else 1.0 - p)

    def r(t):
        F, SF = cdf_np(*rows, t, noise, x, w)
        return F - q if lower else q - SF
    lo, hi = bracket(*rows, noise, x, w, p)
    lo, hi = lo.copy(), hi.copy()
    for _ in range(1200):
        mid = lo + 0.5 * (hi - lo)
        live = (lo < mid) & (mid < hi)
        if not live.any():
            break
        neg = r(mid) < 0.0
        lo = np.where(live & neg, mid, lo)
        hi = np.where(live & ~neg, mid, hi)
    return np.where(np.abs(r(lo)) <= np.abs(r(hi)), lo, hi)


# ---- 50 digits -------------------------------------------------------------------------------------------------------------------
def _mp_table(mp, a, b, c, d, noise, xs):
    """mu_k, s_k of one row at the working precision, from the float64 inputs"""
    a, b, c, d = mp.mpf(float(a)), mp.mpf(max(float(b), 0.0)), mp.mpf(float(c)), mp.mpf(max(float(d), 0.0))
    sg, half, c1, c0, r2 = mp.sqrt(d), mp.mpf(1) / 2, mp.mpf(R.C1), mp.mpf(R.C0), mp.sqrt(2)
    mu, s = [], []
    for xi in xs:
        ph = half * (1 + mp.erf((c + sg * xi) / r2)) * c1 + c0
        mu.append(ph * a)
        s.append(mp.mpf(float(noise)) + ph * ph * b)
    return mu, s


def _mp_A(mp, m, v):
    sd = mp.sqrt(v)
    x = m / sd
    return sd * (2 * mp.npdf(x) + x * mp.erf(x / mp.sqrt(2)))


def cdf_mp(fm, fv, gm, gv, t, noise, x, w, dps=50):
    """([F], [SF]) as mpmath numbers"""
    import mpmath as mp
    with mp.workdps(dps):
        xs, ws, r2 = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in w], mp.sqrt(2)
        F, SF = [], []
        for a, b, c, d, e in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in (fm, fv, gm, gv, t))):
            mu, s = _mp_table(mp, a, b, c, d, noise, xs)
            z = [(mp.mpf(float(e)) - m) / mp.sqrt(v) for m, v in zip(mu, s)]
            F.append(mp.fsum(wk * mp.erfc(-zk / r2) / 2 for wk, zk in zip(ws, z)))
            SF.append(mp.fsum(wk * mp.erfc(zk / r2) / 2 for wk, zk in zip(ws, z)))
        return F, SF


def crps_mp(fm, fv, gm, gv, y, noise, x, w, dps=50):
    import mpmath as mp
    with mp.workdps(dps):
        xs, ws = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in w]
        n, out = len(xs), []
        for a, b, c, d, e in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in (fm, fv, gm, gv, y))):
            mu, s = _mp_table(mp, a, b, c, d, noise, xs)
            t1 = mp.fsum(ws[i] * _mp_A(mp, mp.mpf(float(e)) - mu[i], s[i]) for i in range(n))
            off = mp.fsum(ws[i] * ws[j] * _mp_A(mp, mu[i] - mu[j], s[i] + s[j]) for i in range(n) for j in range(i + 1, n))   # i < j: half of the off-diagonal
            diag = mp.fsum(ws[i] * ws[i] * mp.sqrt(s[i] / mp.pi) for i in range(n))                                             # 1/2 w_i^2 A(0, 2 s_i)
            out.append(t1 - off - diag)
        return out


def quantile_residual(fm, fv, gm, gv, noise, x, w, p, t):
    """|G(t) - q| at 50 digits as float64: G = F, q = p for p <= 1/2, else G = SF, q = 1 - p"""
    import mpmath as mp
    F, SF = cdf_mp(fm, fv, gm, gv, t, noise, x, w)
    with mp.workdps(50):
        if p <= 0.5:
            return np.array([float(abs(v - mp.mpf(float(p)))) for v in F])
        return np.array([float(abs(v - (1 - mp.mpf(float(p))))) for v in SF])


def quantile_scale(fm, fv, gm, gv, noise, x, w, p, t):
    """eps S_F(t) + ulp(t) pdf(t): the unit of the quantile's residual in probability"""
    S = cdf_scales(fm, fv, gm, gv, t, noise, x, w)[0 if p <= 0.5 else 1]
    return EPS * S + np.spacing(np.abs(t)) * pdf_np(fm, fv, gm, gv, t, noise, x, w)


err_to = R.err_to


# ---- the Gaussian head -----------------------------------------------------------------------------------------------------------
def head_np(fm, fv, y, noise, levels=()):
    """(F, SF, CRPS, quantiles (L, N)) in float64"""
    from scipy.special import ndtri
    fm, fv, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (fm, fv, y))
    s = fv + noise
    z = (y - fm) / np.sqrt(s)
    zp = np.array([ndtri(p) if p <= 0.5 else -ndtri(1.0 - p) for p in levels]).reshape(-1, 1)
    return Phi(z), Phi(-z), A(y - fm, s) - np.sqrt(s / np.pi), fm + np.sqrt(s) * zp


def head_mp(fm, fv, y, noise, dps=50):
    import mpmath as mp
    with mp.workdps(dps):
        F, SF, Cr = [], [], []
        for a, b, e in zip(*(np.asarray(v, dtype=np.float64).reshape(-1) for v in (fm, fv, y))):
            a, s, e = mp.mpf(float(a)), mp.mpf(float(b)) + mp.mpf(float(noise)), mp.mpf(float(e))
            z = (e - a) / mp.sqrt(s)
            F.append(mp.erfc(-z / mp.sqrt(2)) / 2)
            SF.append(mp.erfc(z / mp.sqrt(2)) / 2)
            Cr.append(_mp_A(mp, e - a, s) - mp.sqrt(s / mp.pi))
        return F, SF, Cr


def head_scales(fm, fv, y, noise):
    """(S_F lower, S_F upper, S_C): the one-component case of the scales above (no link: c = |z| + |t| / sd + |mu| / sd)"""
    fm, fv, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (fm, fv, y))
    s = fv + noise
    sd = np.sqrt(s)
    z = (y - fm) / sd
    c = np.abs(z) + np.abs(y) / sd + np.abs(fm) / sd
    return Phi(z) + phi(z) * c, Phi(-z) + phi(z) * c, np.abs(A(y - fm, s)) + np.sqrt(s / np.pi)


def head_quantile_residual(fm, fv, noise, p, t):
    """(|G(t) - q| at 50 digits, eps S_F(t) + ulp(t) pdf(t)) of the Gaussian head"""
    F, SF, _ = head_mp(fm, fv, t, noise)
    import mpmath as mp
    with mp.workdps(50):
        res = np.array([float(abs(v - mp.mpf(float(p)))) for v in F]) if p <= 0.5 else np.array([float(abs(v - (1 - mp.mpf(float(p))))) for v in SF])
    S = head_scales(fm, fv, t, noise)[0 if p <= 0.5 else 1]
    s = np.asarray(fv, dtype=np.float64).reshape(-1) + noise
    z = (np.asarray(t).reshape(-1) - np.asarray(fm).reshape(-1)) / np.sqrt(s)
    return res, EPS * S + np.spacing(np.abs(t)) * phi(z) / np.sqrt(s)


# ---- cached cases ----------------------------------------------------------------------------------------------------------------
def _rule(n):
    x, w = R.rule(n)
    keep = w > 0
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(w[keep])


@functools.lru_cache(maxsize=None)
def fifth():
    """every fifth row of the subset (12 rows)"""
    cols = tuple(np.ascontiguousarray(c[::5]) for c in R.subset())
    for c in cols:
        c.setflags(write=False)
    return cols


def rows_of(which):
    return {'grid': R.grid, 'subset': R.subset, 'fifth': fifth}[which]()


@functools.lru_cache(maxsize=None)
def cdf_case(n, which):
    """(rows, rule, (F, SF) at 50 digits, (err_np of F, of SF), (S_F lower, upper)) at t = y; one 50-digit evaluation per session"""
    rows, (x, w) = rows_of(which), _rule(n)
    t = cdf_mp(*rows, NOISE, x, w)
    got = cdf_np(*rows, NOISE, x, w)
    return rows, (x, w), t, (err_to(t[0], got[0]), err_to(t[1], got[1])), cdf_scales(*rows, NOISE, x, w)


@functools.lru_cache(maxsize=None)
def crps_case(n, which):
    """(rows, rule, CRPS at 50 digits, err_np, S_C)"""
    rows, (x, w) = rows_of(which), _rule(n)
    t = crps_mp(*rows, NOISE, x, w)
    return rows, (x, w), t, err_to(t, crps_np(*rows, NOISE, x, w)), crps_scale(*rows, NOISE, x, w)


@functools.lru_cache(maxsize=None)
def quantile_case(n, which, p):
    """(t of the bisection, its residual at 50 digits, eps S_F + ulp pdf at that t)"""
    rows, (x, w) = rows_of(which), _rule(n)
    r4 = rows[:4]
    t = quantile_np(*r4, NOISE, x, w, p)
    return t, quantile_residual(*r4, NOISE, x, w, p, t), quantile_scale(*r4, NOISE, x, w, p, t)
