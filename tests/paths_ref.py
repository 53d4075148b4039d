"""References of the sample paths (include/zigp.h "sample paths"), shared by test_cpu_paths.py and
test_gpu_paths.py: the finite sum of zigp_path_rows in NumPy and in 50-digit mpmath, the magnitude S of the point-wise rule, and the
NumPy restatement of zigp_sample_paths for the three parametrisations (zigp.pathwise.weights_np: Cholesky and triangular solves)."""
import math

import numpy as np
from scipy.special import erf

from zigp import pathwise

FLOOR = 1e-12
EPS = 2.220446049250313e-16
SQ = {'matern32': math.sqrt(3.0), 'matern52': math.sqrt(5.0)}


def r2_np(X, Z, ell):
    """(N, M) scaled squared distances from direct differences"""
    A, B = np.asarray(X, dtype=np.float64) / ell, np.asarray(Z, dtype=np.float64) / ell
    return np.sum(np.square(A[:, None, :] - B[None, :, :]), 2)


def k_of_r2_np(kind, r2, var):
    if kind == 'rbf':
        return var * np.exp(-r2 / 2)
    r = np.sqrt(r2 + FLOOR)
    if kind == 'matern32':
        return var * (1.0 + SQ[kind] * r) * np.exp(-SQ[kind] * r)
    if kind == 'matern52':
        return var * (1.0 + SQ[kind] * r + 5.0 / 3.0 * np.square(r)) * np.exp(-SQ[kind] * r)
    raise ValueError(kind)


def kern_np(kind, X, Z, ell, var):
    return k_of_r2_np(kind, r2_np(X, Z, np.broadcast_to(np.asarray(ell, dtype=np.float64).reshape(-1), (np.shape(X)[1],))), float(var))


def _ell(lat, D):
    return np.broadcast_to(np.asarray(lat['ell'], dtype=np.float64).reshape(-1), (D,))


def path_sum_np(lat, X):
    """(out (S, N), mag (S, N)) of one latent dict (DenseEngine.path_rows): the sum in NumPy, and the magnitude S of the point-wise
    rule -- the sum of the terms' absolute values, each times one plus the magnitude of its argument: sum_d |omega x| + |b| for a
    cosine, the exponent (r^2 / 2, or sqrt(2 nu) r) for a kernel value; the mean part's terms count once."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    kind = lat.get('kind', 'rbf')
    ell = _ell(lat, D)
    r2 = r2_np(X, lat['Z'], ell)
    K = k_of_r2_np(kind, r2, float(lat['var']))                                   # (N, M)
    expo = r2 / 2 if kind == 'rbf' else SQ[kind] * np.sqrt(r2 + FLOOR)
    V = np.asarray(lat['V'], dtype=np.float64)
    out = K @ V
    mag = (np.abs(K) * (1.0 + expo)) @ np.abs(V)
    phase = np.asarray(lat['phase'], dtype=np.float64).reshape(-1)
    if phase.size:
        om, amp = np.asarray(lat['omega'], dtype=np.float64), np.asarray(lat['amp'], dtype=np.float64)
        arg = X @ om.T + phase[None, :]
        c = np.cos(arg)
        out = out + c @ amp
        mag = mag + (np.abs(c) * (1.0 + np.abs(X) @ np.abs(om).T + np.abs(phase)[None, :])) @ np.abs(amp)
    lin = lat.get('lin')
    shift = float(lat.get('shift', 0.0))
    if lin is not None:
        lin = np.asarray(lin, dtype=np.float64).reshape(-1)
        out = out + (X @ lin)[:, None]
        mag = mag + (np.abs(X) @ np.abs(lin))[:, None]
    return (out + shift).T, (mag + abs(shift)).T


def path_sum_mp(lat, X, rows, cols):
    """The sum at the elements rows x cols in 50-digit arithmetic from the doubles as given: float array (len(cols), len(rows)) of the
    correctly rounded values"""
    import mpmath as mp
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    kind = lat.get('kind', 'rbf')
    ell = [mp.mpf(float(v)) for v in _ell(lat, D)]
    Z, V = np.asarray(lat['Z'], dtype=np.float64), np.asarray(lat['V'], dtype=np.float64)
    phase = np.asarray(lat['phase'], dtype=np.float64).reshape(-1)
    R, M = phase.size, Z.shape[0]
    om = np.asarray(lat['omega'], dtype=np.float64).reshape(R, D) if R else None
    amp = np.asarray(lat['amp'], dtype=np.float64) if R else None
    lin = None if lat.get('lin') is None else np.asarray(lat['lin'], dtype=np.float64).reshape(-1)
    var, shift = mp.mpf(float(lat['var'])), mp.mpf(float(lat.get('shift', 0.0)))
    out = np.zeros((len(cols), len(rows)))
    with mp.workdps(50):
        for jn, n in enumerate(rows):
            x = [mp.mpf(float(v)) for v in X[n]]
            feat = []
            for m in range(M):
                r2 = mp.fsum(((x[d] - mp.mpf(float(Z[m, d]))) / ell[d]) ** 2 for d in range(D))
                if kind == 'rbf':
                    k = var * mp.exp(-r2 / 2)
                else:
                    r = mp.sqrt(r2 + mp.mpf(FLOOR))
                    a = mp.sqrt(3) if kind == 'matern32' else mp.sqrt(5)
                    poly = 1 + a * r if kind == 'matern32' else 1 + a * r + mp.mpf(5) / 3 * r * r
                    k = var * poly * mp.exp(-a * r)
                feat.append(k)
            for r_ in range(R):
                feat.append(mp.cos(mp.fsum(mp.mpf(float(om[r_, d])) * x[d] for d in range(D)) + mp.mpf(float(phase[r_]))))
            mean = shift + (mp.fsum(mp.mpf(float(lin[d])) * x[d] for d in range(D)) if lin is not None else 0)
            for js, s in enumerate(cols):
                w = [mp.mpf(float(V[m, s])) for m in range(M)] + [mp.mpf(float(amp[r_, s])) for r_ in range(R)]
                out[js, jn] = float(mean + mp.fdot(w, feat))
    return out


def pick(n, want):
    """Up to `want` indices of range(n): the ends, the 16-tile boundaries, then evenly spread"""
    idx = {0, n - 1}
    for b in (15, 16, 17, 31, 32, 63, 64, 127, 128):
        if b < n:
            idx.add(b)
    idx = sorted(idx)[:want]
    if len(idx) < min(want, n):
        for v in np.linspace(0, n - 1, want).astype(int):
            if len(idx) < want and int(v) not in idx:
                idx.append(int(v))
    return sorted(idx)


def link(g):
    """Phi~ (OnOffSVGP.py:178), as pointwise_eval and the predictive density write it"""
    return 0.5 * (1.0 + erf(np.asarray(g) * 0.70710678118654752440)) * (1.0 - 2.e-3) + 1.e-3


def link_times_mp(g, f):
    """Phi~(g) f at 50 digits from the doubles as given, rounded once"""
    import mpmath as mp
    with mp.workdps(50):
        return np.array([float(((1 + mp.erf(mp.mpf(float(a)) / mp.sqrt(2))) / 2 * (1 - mp.mpf('2e-3')) + mp.mpf('1e-3')) * mp.mpf(float(b)))
                         for a, b in zip(np.ravel(g), np.ravel(f))])


def latent_tables_np(p, tag, draw, jitter):
    """The latent dict of path_rows that zigp_sample_paths forms for latent `tag` of the parameter dict p (read as DenseEngine reads
    it): omega = omega0 / ell, amp = a sqrt(2 var / R), V = weights_np(...)"""
    Z = np.asarray(p['Z' + tag], dtype=np.float64)
    M, D = Z.shape
    ell = np.broadcast_to(np.asarray(p['ell_' + tag], dtype=np.float64).reshape(-1), (D,)).copy()
    var = float(np.squeeze(p['var_' + tag]))
    kind = p.get('kern_' + tag, 'rbf')
    R = int(draw['R'])
    S = np.shape(draw['eps'])[1]
    omega = np.asarray(draw['omega0'], dtype=np.float64).reshape(R, D) / ell[None, :]
    amp = np.asarray(draw['a'], dtype=np.float64).reshape(R, S) * (math.sqrt(2.0 * var / R) if R else 0.0)
    fZ = pathwise.prior_np(Z, ell, var, draw).T                                                         # (M, S)
    Kuu = kern_np(kind, Z, Z, ell, var) + jitter * np.eye(M)
    V = pathwise.weights_np(Kuu, p['u_%sm' % tag], p['u_%ss_sqrt' % tag], draw['eps'], fZ, whiten=p.get('whiten', False), q_diag=p.get('q_diag', True))
    return dict(kind=kind, Z=Z, ell=ell, var=var, V=V, omega=omega, phase=np.asarray(draw['phase'], dtype=np.float64), amp=amp)


def sample_paths_np(p, X, draws, jitter=1e-6, g_offset=0.0):
    """NumPy restatement of zigp_sample_paths: dict(f, g, gf), each (S, N)"""
    lf, lg = latent_tables_np(p, 'f', draws['f'], jitter), latent_tables_np(p, 'g', draws['g'], jitter)
    if p.get('mean_a') is not None:
        lf['lin'] = np.asarray(p['mean_a'], dtype=np.float64).reshape(-1)
    if p.get('mean_b') is not None:
        lf['shift'] = float(np.squeeze(p['mean_b']))
    lg['shift'] = float(g_offset)
    f, g = path_sum_np(lf, X)[0], path_sum_np(lg, X)[0]
    return dict(f=f, g=g, gf=link(g) * f)


def zero_draws(draws):
    """The draws with eps = 0 and a = 0: the paths collapse onto the posterior mean"""
    return {t: dict(d, a=np.zeros_like(d['a']), eps=np.zeros_like(d['eps'])) for t, d in draws.items()}
