"""Host side of the sample paths (include/zigp.h "sample paths"): the parameter-free draw behind a set of
paths and the NumPy statement of the weights that zigp_sample_paths forms on the device.

A path is  f*(x) = f_prior(x) + k(x, Z) Kuu^-1 (u - f_prior(Z)),  u ~ q(u)  (Wilson et al., 2020), with
f_prior(x) = sqrt(2 var / R) sum_r a_r cos((omega0_r / ell) . x + phase_r) a random-feature draw of the prior."""
import numpy as np

from . import _lib
from ._lib import as_f64

KIND_NAMES = {v: k for k, v in _lib.KERNELS.items()}
MATERN_NU = {_lib.KERN_MATERN32: 1.5, _lib.KERN_MATERN52: 2.5}


def _kind(kind):
    if isinstance(kind, str):
        if kind.lower() not in _lib.KERNELS:
            raise ValueError("kernel %r: the dense path knows 'rbf', 'matern32' and 'matern52'" % (kind,))
        return _lib.KERNELS[kind.lower()]
    if kind not in KIND_NAMES:
        raise ValueError('kernel kind %r is not a ZIGP_KERN_* value' % (kind,))
    return int(kind)


def check_sizes(D, S):
    """The sizes every path call refuses, before the library is touched"""
    if not 1 <= D <= _lib.PATH_MAX_D:
        raise ValueError('D = %d: the sample paths cover input dimensions 1 .. %d' % (D, _lib.PATH_MAX_D))
    if not 1 <= S <= _lib.PATH_MAX_S:
        raise ValueError('S = %d: a call draws 1 .. %d sample paths (ZIGP_PATH_MAX_S)' % (S, _lib.PATH_MAX_S))


def draw(kind, R, D, M, S, rng):
    """The draw of one latent: dict(R, omega0 (R, D), phase (R), a (R, S), eps (M, S)).  rng: a numpy RandomState or Generator.
    omega0 are the spectral frequencies at unit lengthscales: z ~ N(0, I) for RBF, z sqrt(2 nu / chi2_{2 nu}) (a multivariate Student-t
    with 2 nu degrees of freedom) for Matern nu = 3/2, 5/2; the phase is uniform on [0, 2 pi)."""
    kind = _kind(kind)
    check_sizes(D, S)
    if R < 0 or M < 1:
        raise ValueError('R = %d, M = %d: R must be >= 0 and M >= 1' % (R, M))
    z = rng.standard_normal((R, D))
    if kind in MATERN_NU:
        nu = MATERN_NU[kind]
        z = z * np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=(R, 1)))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=R)
    return dict(R=int(R), omega0=as_f64(z), phase=as_f64(phase), a=as_f64(rng.standard_normal((R, S))), eps=as_f64(rng.standard_normal((M, S))))


def check_draw(d, tag, M, D, S):
    """Shapes of a draw against the model, by name; returns the four arrays as C-contiguous float64"""
    R = int(d['R'])
    if R < 0:
        raise ValueError('draw_%s: R is negative' % tag)
    out = {}
    for k, shape in (('omega0', (R, D)), ('phase', (R,)), ('a', (R, S)), ('eps', (M, S))):
        a = as_f64(d[k])
        if a.shape != shape:
            raise ValueError('draw_%s.%s must be %s, not %s' % (tag, k, shape, a.shape))
        out[k] = a
    return R, out


def features_np(X, omega, phase):
    """cos(X omega^T + phase), (N, R)"""
    return np.cos(as_f64(X) @ as_f64(omega).T + as_f64(phase)[None, :])


def prior_np(X, ell, var, d):
    """f_prior at the rows X for every sample of the draw d: (S, N)"""
    R = int(d['R'])
    if R == 0:
        return np.zeros((np.shape(d['a'])[1], np.shape(X)[0]))
    omega = as_f64(d['omega0']) / as_f64(ell).reshape(1, -1)
    amp = as_f64(d['a']) * np.sqrt(2.0 * float(var) / R)
    return (features_np(X, omega, d['phase']) @ amp).T


def weights_np(Kuu, u_m, q_sqrt, eps, fZ, whiten=False, q_diag=True):
    """V (M, S) with  k(x, Z) V = k(x, Z) Kuu^-1 (u - f_Z),  u = the draw of q(u) behind eps:  V = L^-T t  by Cholesky and triangular
    solves, Kuu = L L^T (jitter included by the caller), fZ (M, S) = f_prior(Z):
      unwhitened            t = L^-1 (u_m + s o eps - fZ)
      whitened, diagonal    t = u_m + s o eps - L^-1 fZ
      whitened, full        t = u_m + tril(L_q) eps - L^-1 fZ"""
    from scipy.linalg import solve_triangular
    Kuu, eps, fZ = as_f64(Kuu), as_f64(eps), as_f64(fZ)
    M = Kuu.shape[0]
    u_m = as_f64(u_m).reshape(M, 1)
    L = np.linalg.cholesky(Kuu)
    if not whiten:
        if not q_diag:
            raise ValueError('q_diag=False needs whiten=True')
        t = solve_triangular(L, u_m + as_f64(q_sqrt).reshape(M, 1) * eps - fZ, lower=True)
    elif q_diag:
        t = u_m + as_f64(q_sqrt).reshape(M, 1) * eps - solve_triangular(L, fZ, lower=True)
    else:
        t = u_m + np.tril(as_f64(q_sqrt).reshape(M, M)) @ eps - solve_triangular(L, fZ, lower=True)
    return solve_triangular(L.T, t, lower=False)


# ---- the Kronecker (space x time) model and its heads (include/zigp_kronpaths.h) ----
# draw() serves them with D = D0 + D1 and M = M0 M1: omega0 holds the frequencies of all the columns, eps the normals of the grid
# (factor-0-major, as u_fm).  prior_np serves them with ell = [ell0 | ell1] and var = var0 var1.

def check_kron_sizes(D0, D1, M0, M1, S):
    """The sizes every Kronecker path call refuses, before the library is touched"""
    if D0 < 1 or D1 < 1 or D0 + D1 > _lib.PATH_MAX_D:
        raise ValueError('D0 = %d, D1 = %d: the Kronecker sample paths cover D0, D1 >= 1 with D0 + D1 <= %d' % (D0, D1, _lib.PATH_MAX_D))
    if not (1 <= M0 <= _lib.KRON_PATH_MAX_M and 1 <= M1 <= _lib.KRON_PATH_MAX_M):
        raise ValueError('M0 = %d, M1 = %d: the Kronecker sample paths cover 1 .. %d inducing points per factor' % (M0, M1, _lib.KRON_PATH_MAX_M))
    if not 1 <= S <= _lib.PATH_MAX_S:
        raise ValueError('S = %d: a call draws 1 .. %d sample paths (ZIGP_PATH_MAX_S)' % (S, _lib.PATH_MAX_S))


def kron_kinds(kinds):
    """(kind0, kind1) as ZIGP_KERN_* values from a name or kind (both factors) or a pair of them"""
    if isinstance(kinds, (str, int, np.integer)):
        kinds = (kinds, kinds)
    if len(kinds) != 2:
        raise ValueError('the kinds of a Kronecker latent are a name or a pair (kind0, kind1), not %r' % (kinds,))
    return _kind(kinds[0]), _kind(kinds[1])


def kron_draw(kinds, R, D0, D1, M0, M1, S, rng):
    """The draw of one Kronecker latent whose factors have the kinds (kind0, kind1): the dict of draw() with omega0 (R, D0 + D1) and
    eps (M0 M1, S).  The spectral density of a product kernel is the product of the factors' densities, so the omega0 columns of factor
    q follow that factor's law: z ~ N(0, I) for RBF, z sqrt(2 nu / chi2_{2 nu}) with ONE chi2 per feature and per Matern factor (factor
    0 first).  With both kinds RBF the generator is consumed exactly as by draw('rbf', R, D0 + D1, M0 M1, S, rng)."""
    k = kron_kinds(kinds)
    check_kron_sizes(D0, D1, M0, M1, S)
    if R < 0:
        raise ValueError('R = %d must be >= 0' % R)
    z = rng.standard_normal((R, D0 + D1))
    for q, cols in ((0, slice(0, D0)), (1, slice(D0, D0 + D1))):
        if k[q] in MATERN_NU:
            nu = MATERN_NU[k[q]]
            z[:, cols] *= np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=(R, 1)))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=R)
    return dict(R=int(R), omega0=as_f64(z), phase=as_f64(phase), a=as_f64(rng.standard_normal((R, S))),
                eps=as_f64(rng.standard_normal((M0 * M1, S))))


def kron_weights_np(K0, K1, u_m, q_sqrt, eps, fZ):
    """V (M0 M1, S), factor-0-major, with  (k0(x, Z0) (x) k1(x, Z1)) V = k(x, Z) (K0 (x) K1)^-1 (u - f_Z),  u = u_m + s o eps the draw of
    q(u) behind eps:  V_s = K0^-1 (U + S o E_s - F_Z,s) K1^-1 as M0 x M1 matrices, by the Cholesky factor of each K_p (jitter included
    by the caller) and triangular solves -- nothing of size M0 M1 x M0 M1 is formed.  fZ (M0 M1, S) = f_prior at the grid points."""
    from scipy.linalg import solve_triangular
    K0, K1, eps, fZ = as_f64(K0), as_f64(K1), as_f64(eps), as_f64(fZ)
    M0, M1 = K0.shape[0], K1.shape[0]
    M, S = M0 * M1, eps.shape[1]
    if eps.shape != (M, S) or fZ.shape != (M, S):
        raise ValueError('eps and fZ must be (M0 M1, S) = (%d, %d)' % (M, S))
    rhs = as_f64(u_m).reshape(M, 1) + as_f64(q_sqrt).reshape(M, 1) * eps - fZ
    L0, L1 = np.linalg.cholesky(K0), np.linalg.cholesky(K1)
    R = rhs.reshape(M0, M1 * S)                                                     # K0^-1 from the left, every (j, s) column at once
    R = solve_triangular(L0.T, solve_triangular(L0, R, lower=True), lower=False).reshape(M0, M1, S)
    R = np.ascontiguousarray(R.transpose(1, 0, 2)).reshape(M1, M0 * S)              # K1^-1 from the right = from the left of the transpose
    R = solve_triangular(L1.T, solve_triangular(L1, R, lower=True), lower=False).reshape(M1, M0, S)
    return np.ascontiguousarray(R.transpose(1, 0, 2)).reshape(M, S)


def kron_grid(Z0, Z1):
    """The M0 M1 grid points (i, j) as rows [z0_i | z1_j], factor-0-major: (M0 M1, D0 + D1)"""
    Z0, Z1 = as_f64(Z0), as_f64(Z1)
    return np.hstack([np.repeat(Z0, Z1.shape[0], axis=0), np.tile(Z1, (Z0.shape[0], 1))])
