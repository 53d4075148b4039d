"""tests/kronf_ref.py with a kernel kind PER FACTOR: NumPy restatements of the per-point tile kernels of the fused Kronecker path in their
Matern form (csrc/zigp_kronf.hip k_kf_forward_kinds / k_kf_backward_kinds, csrc/zigp_kronl.h k_kfl_*_kinds), and the fixtures of the fused
Matern tests.  TEST INFRASTRUCTURE ONLY.

Conventions of kronf_ref.py: every function takes a `dtype` (np.float64 or np.longdouble) and returns (value, S), S the first-order error
weight of the sums behind the value.  With every kind 'rbf' each function returns kronf_ref's bits (the RBF tile IS kronf_ref.ktile and the
expressions around it are kronf_ref's, in its order): tests/test_cpu_kron_matern_fused.py pins that.

A Matern tile: r2 from z / ell - x / ell as kronf_ref.ktile forms it, r = sqrt(r2 + 1e-12), t = sqrt(3) r or sqrt(5) r,
    Matern32  K = var (1 + t) exp(-t)               K' = 3 var exp(-t)
    Matern52  K = var (1 + t + 5/3 r^2) exp(-t)     K' = 5/3 var (1 + t) exp(-t)
K' = -dK / d(r2 / 2).  Error weight of K: an absolute error w of r2 / 2 (kronf_ref.ktile's w) moves K by K' w, and sqrt, the product with
sqrt(3) / sqrt(5), the polynomial and exp add a few roundings plus t of them (exp turns the rounding of its argument into t eps of its
value): eK = |K| (6 + t) + K' w.  K' carries the same weight form with K'' <= K' (a 3 / 5 multiple of a decaying factor): eKd = |K'| (6 + t + 5 w).

The backward sums: everything of kronf_ref.backward, except that the moment columns 1 .. 2 D of a Matern factor take t' = dK . K' where an
RBF factor takes t = dK . K (column 0 keeps t), and that column 15 of the 16-column moment block of a Matern factor holds sum t' (the finish
kernels re-centre the t' moments with it); for an RBF factor column 15 is zero, as every column beyond 2 D."""
import numpy as np

import kronf_ref as R
from kronf_ref import _f, psi

KINDS = ('rbf', 'matern32', 'matern52')
FLOOR = 1e-12


def ktile(kind, Z, ell, var, Xp, dtype=np.float64, weight=False, grad=False):
    """(K[, eK]) as kronf_ref.ktile for 'rbf'; for a Matern kind the same from the formulas above.  grad: (K, eK, Kd, eKd) (weight implied)."""
    if kind == 'rbf':
        if not grad:
            return R.ktile(Z, ell, var, Xp, dtype, weight)
        K, eK = R.ktile(Z, ell, var, Xp, dtype, True)
        return K, eK, K, eK
    inv = 1 / _f(ell, dtype).reshape(-1)
    zs, xs = _f(Z, dtype) * inv, _f(Xp, dtype) * inv
    D = zs.shape[1]
    r2 = np.zeros((zs.shape[0], xs.shape[0]), dtype=dtype)
    w = np.zeros_like(r2)
    for d in range(D):
        t = zs[:, None, d] - xs[None, :, d]
        r2 = r2 + t * t
        w = w + np.abs(t) * (np.abs(zs[:, None, d]) + np.abs(xs[None, :, d]) + np.abs(t))
    w = w + (D + 1) * r2 / 2
    r = np.sqrt(r2 + dtype(FLOOR))
    v = _f(var, dtype).reshape(())
    if kind == 'matern32':
        t = np.sqrt(dtype(3)) * r
        e = np.exp(-t)
        K, Kd = v * (1 + t) * e, 3 * v * e
    else:
        t = np.sqrt(dtype(5)) * r
        e = np.exp(-t)
        K, Kd = v * (1 + t + dtype(5) / dtype(3) * (r * r)) * e, dtype(5) / dtype(3) * v * (1 + t) * e
    eK, eKd = np.abs(K) * (6 + t) + np.abs(Kd) * w, np.abs(Kd) * (6 + t + 5 * w)
    if grad:
        return K, eK, Kd, eKd
    return (K, eK) if weight else K


class _Tiles(R._Tiles):
    """kronf_ref._Tiles with the factor kinds: K, A = P K and, for the backward sums, K'"""
    def __init__(self, kinds, P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype):
        self.P = (_f(P0, dtype), _f(P1, dtype))
        D0 = np.asarray(Z0).shape[1]
        Xn = np.asarray(X)[:N]
        self.Xp = (Xn[:, :D0], Xn[:, D0:])
        kt = (ktile(kinds[0], Z0, ell0, var0, self.Xp[0], dtype, grad=True), ktile(kinds[1], Z1, ell1, var1, self.Xp[1], dtype, grad=True))
        self.K, self.eK = (kt[0][0], kt[1][0]), (kt[0][1], kt[1][1])
        self.Kd, self.eKd = (kt[0][2], kt[1][2]), (kt[0][3], kt[1][3])
        self.A = tuple(self.P[p] @ self.K[p] for p in range(2))
        self.eA = tuple(np.abs(self.P[p]) @ self.eK[p] for p in range(2))
        self.sq = tuple(a * a for a in self.A)
        self.esq = tuple(2 * np.abs(self.A[p]) * self.eA[p] + self.sq[p] for p in range(2))


def forward(kinds, P0, P1, Al, S2, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype=np.float64):
    """kronf_ref.forward with the factor kinds: (part, S), both (4, N)"""
    t = _Tiles(kinds, P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype)
    Al, S2 = _f(Al, dtype), _f(S2, dtype)
    K, eK, A, eA = t.K, t.eK, t.A, t.eA
    B0, eB0 = Al @ K[1], np.abs(Al) @ eK[1]
    C0, eC0 = S2 @ t.sq[1], np.abs(S2) @ t.esq[1]
    part = np.stack([(K[0] * A[0]).sum(0), (K[1] * A[1]).sum(0), (K[0] * B0).sum(0), (t.sq[0] * C0).sum(0)])
    S = np.stack([(eK[0] * np.abs(A[0]) + np.abs(K[0]) * eA[0]).sum(0), (eK[1] * np.abs(A[1]) + np.abs(K[1]) * eA[1]).sum(0),
                  (eK[0] * np.abs(B0) + np.abs(K[0]) * eB0).sum(0), (t.esq[0] * np.abs(C0) + t.sq[0] * eC0).sum(0)])
    return part, S


def backward(kinds, P0, P1, Al, S2, Z0, Z1, ell0, ell1, var0, var1, X, N, part, gm, gv, dq0, dq1, zc0, zc1, dtype=np.float64):
    """kronf_ref.backward with the factor kinds.  Kr_p [M_p][1 + 2 D_p] is the moment block as the finish kernels read it: column 0
    (dK_p . K_p) 1, columns >= 1 (dK_p . K'_p) Psi_p; 'Kd%d' [M_p] is sum_n (dK_p . K'_p), column 15 of the device block of a Matern
    factor (an RBF factor: the device column is zero and this entry is None)."""
    del part
    t = _Tiles(kinds, P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype)
    Al, S2 = _f(Al, dtype), _f(S2, dtype)
    K, eK, A, eA, P = t.K, t.eK, t.A, t.eA, t.P
    gm, gv, dq = _f(gm, dtype)[:N], _f(gv, dtype)[:N], (_f(dq0, dtype)[:N], _f(dq1, dtype)[:N])
    agm, agv = np.abs(gm), np.abs(gv)
    Ps = (psi(t.Xp[0], zc0, dtype), psi(t.Xp[1], zc1, dtype))
    B, eB = (Al @ K[1], Al.T @ K[0]), (np.abs(Al) @ eK[1], np.abs(Al).T @ eK[0])
    Cc, eC = (S2 @ t.sq[1], S2.T @ t.sq[0]), (np.abs(S2) @ t.esq[1], np.abs(S2).T @ t.esq[0])
    out = dict(dAl=((K[0] * gm) @ K[1].T, (eK[0] * agm) @ np.abs(K[1]).T + (np.abs(K[0]) * agm) @ eK[1].T),
               dS2=((t.sq[0] * gv) @ t.sq[1].T, (t.esq[0] * agv) @ t.sq[1].T + (t.sq[0] * agv) @ t.esq[1].T))
    for p in range(2):
        aA, aK, adq = np.abs(A[p]), np.abs(K[p]), np.abs(dq[p])
        dA = 2 * gv * A[p] * Cc[p]
        edA = 2 * agv * (eA[p] * np.abs(Cc[p]) + aA * eC[p] + aA * np.abs(Cc[p]))
        E, eE = dq[p] * K[p] + dA, adq * eK[p] + edA
        out['dP%d' % p] = (E @ K[p].T, eE @ aK.T + np.abs(E) @ eK[p].T)
        PdA, ePdA = P[p] @ dA, np.abs(P[p]) @ (edA + np.abs(dA))
        dK = gm * B[p] + 2 * dq[p] * A[p] + PdA
        edK = agm * (eB[p] + np.abs(B[p])) + 2 * adq * (eA[p] + aA) + ePdA + np.abs(PdA)
        tt, ett = dK * K[p], edK * aK + np.abs(dK) * eK[p]
        if kinds[p] == 'rbf':
            out['Kr%d' % p] = (tt @ Ps[p], (ett + 3 * np.abs(tt)) @ np.abs(Ps[p]))
            out['Kd%d' % p] = None
            continue
        td, etd = dK * t.Kd[p], edK * np.abs(t.Kd[p]) + np.abs(dK) * t.eKd[p]
        v0, s0 = tt @ Ps[p][:, :1], (ett + 3 * np.abs(tt)) @ np.abs(Ps[p][:, :1])
        v1, s1 = td @ Ps[p][:, 1:], (etd + 3 * np.abs(td)) @ np.abs(Ps[p][:, 1:])
        out['Kr%d' % p] = (np.concatenate([v0, v1], 1), np.concatenate([s0, s1], 1))
        out['Kd%d' % p] = (td.sum(1), (etd + 3 * np.abs(td)).sum(1))
    return out


def factor_K(kind, Z, ell, var, jitter, dtype=np.float64):
    """K_p (M, M) as k_kf_factor[_kinds] builds it: differences of the inducing inputs times 1 / ell, the kernel's formula (a Matern
    diagonal at r2 = 0: r = 1e-6), plus jitter on the diagonal."""
    Z = _f(Z, dtype)
    inv = 1 / _f(ell, dtype).reshape(-1)
    q = (Z[:, None, :] - Z[None, :, :]) * inv
    r2 = np.zeros(q.shape[:2], dtype=dtype)
    for d in range(q.shape[2]):
        r2 = r2 + q[:, :, d] * q[:, :, d]
    v = _f(var, dtype).reshape(())
    if kind == 'rbf':
        K = v * np.exp(-r2 / 2)
    else:
        r = np.sqrt(r2 + dtype(FLOOR))
        if kind == 'matern32':
            t = np.sqrt(dtype(3)) * r
            K = v * (1 + t) * np.exp(-t)
        else:
            t = np.sqrt(dtype(5)) * r
            K = v * (1 + t + dtype(5) / dtype(3) * (r * r)) * np.exp(-t)
    return K + dtype(jitter) * np.eye(Z.shape[0], dtype=dtype)


# ---- the fixtures of the fused Matern tests: the fused-eligible cases of kron_matern_ref.FIXTURES, with their kinds, and four more cases
# of kron_nd.CASES -- <2,1> blocks, <1,2> and <2,1> in one step, both factors at seven columns, a larger grid whose latents differ --
# with kinds chosen so that every one of the nine (kind0, kind1) pairs stands on some latent of the table. ----
NEW_KINDS = {
    'd21-21': (('matern52', 'rbf'), ('rbf', 'matern52')),
    'd21-mix2': (('matern32', 'matern52'), ('rbf', 'rbf')),
    'd77': (('matern52', 'matern32'), ('rbf', 'matern32')),
    'L51': (('rbf', 'matern32'), ('matern32', 'rbf')),
}
L77_KINDS = (('matern32', 'matern52'), ('matern52', 'rbf'))      # L77 is not in the table above: its kinds in the finish-stage tests
PINNED = ('d11', 'd21-12', 'd21-mix', 'd31', 'd17', 'L32')      # held to floor <= 1e-8, cond <= 1e5 by tests/test_cpu_kron_matern.py


def fixture_kinds():
    import kron_matern_ref as kmr
    out = {k: kmr.FIXTURES[k] for k in PINNED}
    out.update(NEW_KINDS)
    return out


def fixture(name):
    """(X, Y, p) of kron_nd.problem(name) with the table's kinds in p (arrays shared with kron_nd's cache, read-only)"""
    import kron_matern_ref as kmr
    import kron_nd
    X, Y, p = kron_nd.problem(name)
    kf, kg = fixture_kinds()[name]
    return X, Y, kmr.with_kinds(p, kf, kg)


def zz_kd(kind, Z, ell, var, dtype=np.float64):
    """(K', eK') (M, M) of a Matern factor at its own inducing inputs, as k_kf_kd_prepare / k_kfl_krow_kinds form it: the second pair of
    ktile(..., grad=True) with Xp = Z"""
    _, _, Kd, eKd = ktile(kind, Z, ell, var, Z, dtype, grad=True)
    return Kd, eKd


def finish(kinds, w, K0, K1, P0, P1, U, S2, T0, T1, Al, s, Z0, Z1, zc0, zc1, jitter, kl, ell, var, dtype=np.float64, Kd=(None, None), _mut=()):
    """kronf_ref.finish with the factor kinds.  A Matern factor differs in the moment columns 1 .. 2 D of its krow only: tt = G . K'_p(Z_p, Z_p)
    in place of G . (K_p - jitter I), and the re-centring with column 15 of its moment block (sum t') in place of column 0.  w['Kr%d' % p] is
    the device block of the factor, 16 columns.  Kd[p]: (K', eK') to use for factor p (a stage test passes the tapped image with a zero
    weight); None: formed here from Z_p, ell[p], var[p].  With every kind 'rbf' this IS kronf_ref.finish (same call, same bits)."""
    mom = []
    for p, (Z, Kr) in enumerate(((Z0, w['Kr0']), (Z1, w['Kr1']))):
        if kinds[p] == 'rbf':
            mom.append(None)
            continue
        kd = Kd[p] if Kd[p] is not None else zz_kd(kinds[p], Z, ell[p], var[p], dtype)
        mom.append((kd[0], kd[1], np.asarray(Kr)[:, 15]))
    return R.finish(w, K0, K1, P0, P1, U, S2, T0, T1, Al, s, Z0, Z1, zc0, zc1, jitter, kl, dtype, _mom=tuple(mom), _mut=_mut)
