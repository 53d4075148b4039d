"""References of the Kronecker sample paths (include/zigp_kronpaths.h), shared by
test_cpu_kron_paths.py and test_gpu_kron_paths.py: the finite sum of zigp_kron_path_rows in NumPy, in long double and in 50-digit mpmath,
the magnitude S of the point-wise rule, and the NumPy / long-double restatements of zigp_kron_sample_paths and of the heads
(zigp.pathwise.kron_weights_np: per-factor Cholesky and triangular solves).

A Kronecker latent is the dict of DenseEngine.kron_path_rows: Z = [Z0, Z1], ell = [ell0, ell1], var = [var0, var1], V (M0 M1, S)
factor-0-major, omega (R, D0 + D1), phase (R), amp (R, S), shift."""
import functools
import math

import numpy as np

import paths_ref
from zigp import pathwise

EPS = paths_ref.EPS
LD = np.longdouble


def _f(a, dt=np.float64):
    return np.asarray(a, dtype=dt)


def _ells(lat, dt=np.float64):
    Z0, Z1 = lat['Z']
    return [np.broadcast_to(_f(lat['ell'][q], dt).reshape(-1), (np.shape(Z)[1],)) for q, Z in ((0, Z0), (1, Z1))]


def _vars(lat):
    return float(np.squeeze(lat['var'][0])), float(np.squeeze(lat['var'][1]))


def factor_np(X, Z, ell, var, dt=np.float64):
    """(k (N, M), exponent r2 / 2 (N, M)) of one factor from direct differences"""
    d = (_f(Z, dt)[None, :, :] - _f(X, dt)[:, None, :]) / _f(ell, dt).reshape(1, 1, -1)
    a = np.sum(np.square(d), 2) / 2
    return dt(var) * np.exp(-a), a


def expand(lat):
    """The latent dict of DenseEngine.path_rows over the expanded grid: a product of two RBF factors is an RBF over the D0 + D1 columns"""
    e0, e1 = _ells(lat)
    v0, v1 = _vars(lat)
    out = dict(kind='rbf', Z=pathwise.kron_grid(lat['Z'][0], lat['Z'][1]), ell=np.concatenate([e0, e1]), var=v0 * v1, V=_f(lat['V']),
               omega=lat['omega'], phase=lat['phase'], amp=lat['amp'], shift=float(lat.get('shift', 0.0)))
    return out


def kron_path_sum_np(lat, X, dt=np.float64):
    """(out (S, N), mag (S, N)) of one Kronecker latent: the factored sum, and the magnitude S of the point-wise rule -- the sum of
    the terms' absolute values, each times one plus the magnitude of its argument: |a0| + |a1|, the two exponents, for a grid term;
    sum_d |omega x| + |b| for a cosine; the shift counts once.  dt = np.longdouble: the same statement in long double."""
    X = _f(X, dt)
    D0 = np.shape(lat['Z'][0])[1]
    e0, e1 = _ells(lat, dt)
    v0, v1 = _vars(lat)
    k0, a0 = factor_np(X[:, :D0], lat['Z'][0], e0, v0, dt)          # (N, M0)
    k1, a1 = factor_np(X[:, D0:], lat['Z'][1], e1, v1, dt)          # (N, M1)
    M0, M1 = k0.shape[1], k1.shape[1]
    V = _f(lat['V'], dt).reshape(M0, M1, -1)
    out = np.einsum('ni,nj,ijs->ns', k0, k1, V)
    Va = np.abs(V)
    mag = (np.einsum('ni,nj,ijs->ns', k0, k1, Va) + np.einsum('ni,nj,ijs->ns', k0 * a0, k1, Va) + np.einsum('ni,nj,ijs->ns', k0, k1 * a1, Va))
    phase = _f(lat['phase'], dt).reshape(-1)
    if phase.size:
        om, amp = _f(lat['omega'], dt), _f(lat['amp'], dt)
        c = np.cos(X @ om.T + phase[None, :])
        out = out + c @ amp
        mag = mag + (np.abs(c) * (1.0 + np.abs(X) @ np.abs(om).T + np.abs(phase)[None, :])) @ np.abs(amp)
    shift = dt(float(lat.get('shift', 0.0)))
    return (out + shift).T, (mag + abs(shift)).T


def kron_path_sum_mp(lat, X, rows, cols):
    """The sum at the elements rows x cols in 50-digit arithmetic from the doubles as given: float array (len(cols), len(rows)) of the
    correctly rounded values.  The product k0 k1 is not rounded here: this is the sum, not the kernel's arithmetic."""
    import mpmath as mp
    X = _f(X)
    Z0, Z1 = _f(lat['Z'][0]), _f(lat['Z'][1])
    D0, D1 = Z0.shape[1], Z1.shape[1]
    e0, e1 = _ells(lat)
    v0, v1 = _vars(lat)
    M0, M1 = Z0.shape[0], Z1.shape[0]
    V = _f(lat['V']).reshape(M0, M1, -1)
    phase = _f(lat['phase']).reshape(-1)
    R = phase.size
    om = _f(lat['omega']).reshape(R, D0 + D1) if R else None
    amp = _f(lat['amp']) if R else None
    out = np.zeros((len(cols), len(rows)))
    with mp.workdps(50):
        def fac(x, Z, ell, var):
            el = [mp.mpf(float(v)) for v in ell]
            return [mp.mpf(var) * mp.exp(-mp.fsum(((mp.mpf(float(z[d])) - x[d]) / el[d]) ** 2 for d in range(len(el))) / 2) for z in Z]
        for jn, n in enumerate(rows):
            x = [mp.mpf(float(v)) for v in X[n]]
            k0, k1 = fac(x[:D0], Z0, e0, v0), fac(x[D0:], Z1, e1, v1)
            cs = [mp.cos(mp.fsum(mp.mpf(float(om[r, d])) * x[d] for d in range(D0 + D1)) + mp.mpf(float(phase[r]))) for r in range(R)]
            for js, s in enumerate(cols):
                acc = mp.mpf(float(lat.get('shift', 0.0)))
                for i in range(M0):
                    acc += k0[i] * mp.fdot([mp.mpf(float(v)) for v in V[i, :, s]], k1)
                if R:
                    acc += mp.fdot([mp.mpf(float(v)) for v in amp[:, s]], cs)
                out[js, jn] = float(acc)
    return out


def pointwise_ratio(got, ref_np, ref_mp, mag):
    """(largest err / (eps S), largest err - (4 err_np + 16 eps S)) over the sampled elements of the rule err <= 4 err_np + 16 eps S"""
    err, err_np = np.abs(got - ref_mp), np.abs(ref_np - ref_mp)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(mag > 0, err / (EPS * mag), np.where(err == 0, 0.0, np.inf))
    return float(np.max(ratio)), float(np.max(err - (4 * err_np + 16 * EPS * mag)))


def random_latent(rs, M0, M1, D0, D1, R, S, zero=False, shift=0.3):
    """A Kronecker latent over rows on [0, 1]^(D0 + D1): lengthscales of about a third of the cube's diagonal per factor"""
    lat = dict(Z=[rs.rand(M0, D0), rs.rand(M1, D1)], ell=[(0.25 + 0.2 * rs.rand(D0)) * math.sqrt(D0), (0.25 + 0.2 * rs.rand(D1)) * math.sqrt(D1)],
               var=[1.0 + rs.rand(), 0.5 + rs.rand()], V=np.zeros((M0 * M1, S)) if zero else rs.randn(M0 * M1, S),
               omega=3.0 * rs.randn(R, D0 + D1), phase=rs.uniform(0, 2 * np.pi, R), amp=rs.randn(R, S) / math.sqrt(max(R, 1)), shift=shift)
    return lat


# ---- the model calls ------------------------------------------------------------------------------------------------------------------
def rbf(Z, ell, var, dt=np.float64):
    return factor_np(Z, Z, np.broadcast_to(_f(ell, dt).reshape(-1), (np.shape(Z)[1],)), float(np.squeeze(var)), dt)[0]


def factor_matrices(p, tag, jitter, dt=np.float64):
    Z = p['Z' + tag]
    return [rbf(Z[q], p['ell_' + tag][q], p['var_' + tag][q], dt) + dt(jitter) * np.eye(np.shape(Z[q])[0], dtype=dt) for q in range(2)]


def path_bound(p, tags, jitter):
    """The project's path bound min(max(1e-9, 1e-13 c), 1e-6) with c = cond(K0) cond(K1), the largest over the latents `tags`; (bound, c)"""
    c = 0.0
    for t in tags:
        K0, K1 = factor_matrices(p, t, jitter)
        c = max(c, float(np.linalg.cond(K0) * np.linalg.cond(K1)))
    return min(max(1e-9, 1e-13 * c), 1e-6), c


def _chol_ld(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def _solve_lower_ld(L, B, trans=False):
    """L^-1 B (or L^-T B) in long double by substitution, B a matrix"""
    n = L.shape[0]
    X = np.array(B, dtype=LD)
    if not trans:
        for i in range(n):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def kron_weights_ld(K0, K1, u_m, q_sqrt, eps, fZ):
    """pathwise.kron_weights_np in long double"""
    M0, M1 = K0.shape[0], K1.shape[0]
    M, S = M0 * M1, np.shape(eps)[1]
    rhs = _f(u_m, LD).reshape(M, 1) + _f(q_sqrt, LD).reshape(M, 1) * _f(eps, LD) - _f(fZ, LD)
    L0, L1 = _chol_ld(K0), _chol_ld(K1)
    R = _solve_lower_ld(L0, _solve_lower_ld(L0, rhs.reshape(M0, M1 * S)), trans=True).reshape(M0, M1, S)
    R = np.ascontiguousarray(R.transpose(1, 0, 2)).reshape(M1, M0 * S)
    R = _solve_lower_ld(L1, _solve_lower_ld(L1, R), trans=True).reshape(M1, M0, S)
    return np.ascontiguousarray(R.transpose(1, 0, 2)).reshape(M, S)


def kron_latent_tables(p, tag, draw, jitter, dt=np.float64):
    """The latent dict of kron_path_rows that zigp_kron_sample_paths forms for latent `tag` of the Kronecker parameter dict p:
    omega = omega0 / [ell0 | ell1], amp = a sqrt(2 var0 var1 / R), V = kron_weights_np(...) (dt = np.longdouble: in long double)"""
    Z = [_f(p['Z' + tag][0]), _f(p['Z' + tag][1])]
    D = [Z[0].shape[1], Z[1].shape[1]]
    ell = [np.broadcast_to(_f(p['ell_' + tag][q]).reshape(-1), (D[q],)).copy() for q in range(2)]
    var = [float(np.squeeze(p['var_' + tag][q])) for q in range(2)]
    R, S = int(draw['R']), np.shape(draw['eps'])[1]
    ellc = np.concatenate(ell)
    omega = _f(draw['omega0'], dt).reshape(R, D[0] + D[1]) / _f(ellc, dt)[None, :]
    knn = dt(var[0]) * dt(var[1])
    amp = _f(draw['a'], dt).reshape(R, S) * (np.sqrt(dt(2.0) * knn / R) if R else dt(0.0))
    G = pathwise.kron_grid(Z[0], Z[1])
    fZ = (np.cos(_f(G, dt) @ omega.T + _f(draw['phase'], dt)[None, :]) @ amp) if R else np.zeros((G.shape[0], S), dtype=dt)
    K0, K1 = factor_matrices(p, tag, jitter, dt)
    wfun = pathwise.kron_weights_np if dt is np.float64 else kron_weights_ld
    V = wfun(K0, K1, p['u_%sm' % tag], p['u_%ss_sqrt' % tag], draw['eps'], fZ)
    return dict(Z=Z, ell=ell, var=var, V=V, omega=omega, phase=_f(draw['phase'], dt), amp=amp)


def kron_sample_paths_np(p, X, draws, jitter=1e-6, g_offset=0.0, f_mu=0.0, dt=np.float64):
    """Restatement of zigp_kron_sample_paths: dict(f, g, gf), each (S, N)"""
    lf, lg = kron_latent_tables(p, 'f', draws['f'], jitter, dt), kron_latent_tables(p, 'g', draws['g'], jitter, dt)
    lf['shift'], lg['shift'] = float(f_mu), float(g_offset)
    f, g = kron_path_sum_np(lf, X, dt)[0], kron_path_sum_np(lg, X, dt)[0]
    return dict(f=f, g=g, gf=paths_ref.link(_f(g)) * _f(f) if dt is np.float64 else link_ld(g) * f)


def kron_head_sample_paths_np(p, X, lik, draw, jitter=1e-6, f_mu=0.0):
    """Restatement of zigp_kron_head_sample_paths: dict(f) and, for 'bernoulli', p = link(f)"""
    lf = kron_latent_tables(p, 'f', draw, jitter)
    lf['shift'] = float(f_mu)
    f = kron_path_sum_np(lf, X)[0]
    return dict(f=f, p=paths_ref.link(f)) if lik == 'bernoulli' else dict(f=f)


def link_ld(g):
    """Phi~ in long double through the float64 erf and its first-order correction (erf' is exact to long double here)"""
    from scipy.special import erf
    g = _f(g, LD)
    z = g * LD(0.70710678118654752440084436210485)
    z0 = _f(z)
    e = _f(erf(z0), LD) + (z - _f(z0, LD)) * LD(2.0) / np.sqrt(LD(np.pi)) * np.exp(-_f(z0, LD) ** 2)
    return LD(0.5) * (1 + e) * (LD(1.0) - LD(2.e-3)) + LD(1.e-3)


def plane_err(a, b):
    """max |a - b| / max |b| of one plane"""
    a, b = _f(a, LD), _f(b, LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


MODEL_JITTER = 1e-5       # kron_nd.JITTER: the jitter at which the cases' conditioning was tuned
MODEL_R, MODEL_S = 200, 20
MODEL_CASES = ('d21-12', 'd21-mix', 'd31', 'L32', 'p43')


@functools.lru_cache(maxsize=None)
def model_draws(name):
    """The seeded draws of a kron_nd case (R = 200, S = 20): computed once, shared, never written to"""
    import kron_nd
    X, Y, p = kron_nd.problem(name)
    D = p['Zf'][0].shape[1] + p['Zf'][1].shape[1]
    rs = np.random.RandomState(4000 + list(kron_nd.CASES).index(name))
    d = {t: pathwise.draw('rbf', MODEL_R, D, p['Z' + t][0].shape[0] * p['Z' + t][1].shape[0], MODEL_S, rs) for t in ('f', 'g')}
    for t in d:
        for a in d[t].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def model_ref(name, g_offset=0.0, f_mu=0.0):
    """kron_sample_paths_np of a case with its seeded draws"""
    import kron_nd
    X, Y, p = kron_nd.problem(name)
    r = kron_sample_paths_np(p, X, model_draws(name), MODEL_JITTER, g_offset, f_mu)
    for a in r.values():
        a.setflags(write=False)
    return r
