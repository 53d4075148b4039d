"""Plain NumPy restatements of the per-point tile kernels of the fused Kronecker path (csrc/zigp_kronf.hip k_kf_forward / k_kf_backward /
k_kf_reduce / k_kf_latent and their larger-grid twins in csrc/zigp_kronl.h), written from the formulas in the kernels' header comments.
Every function takes a `dtype` (np.float64 or np.longdouble) and returns, per output, the pair (value, S) with S the sum of the absolute
values of the terms of the sums behind that output, each operand that is itself computed entering with its own error weight (below); the
convention of tests/stage_ref.py: an evaluation of the same sums in any order is within a small multiple of eps S of the exact value.
tests/test_cpu_kronf_ref.py pins them to torch autograd and to the oracle; tests/test_gpu_kronf_stages.py holds the kernels to them.
The finish stage (kl_scalars, finish, krow_from_G, assemble at the end of this file: k_kf_finish, k_kfl_finish<1..3> and the host chain rule
kron_assemble_grads) takes its inputs as given, so its S is the plain nested sum of absolute values; tests/test_cpu_kronf_finish_ref.py pins it.

S is a first-order error weight, built with the computation: an input counts with its magnitude, a K tile with eK = |K| (2 + w), w the error weight
of its exponent (ktile), a sum of products sum a_i b_i with sum (e(a_i) |b_i| + |a_i| e(b_i)), the
products' own roundings being covered because every weight is at least the magnitude of its value.  Where a sum has one level (dAl) this
is the sum of the absolute values of its terms; where operands are themselves cancelling sums (A_p = P_p K_p with P_p = K_p^-1, whose
terms are cond(K_p) times larger than A_p) it charges that cancellation once per operand and not once per factor of a product -- the
plain nested sum of absolute values |P||K| squared and multiplied through st = (a0^2)^T S2 (a1^2) allows errors of 1e-4 of the value at
cond(K_p) = 1e4, where this weight allows 1e-10.

Notation per latent: factor p in {0, 1} has M_p inducing points Z_p (M_p, D_p), lengthscales ell_p (D_p), variance var_p and
P_p = (K_p(Z_p, Z_p) + jitter I)^-1; X (N, D0 + D1) holds the columns of factor 0 first.  K_p (M_p, N) is the cross-covariance tile,
A_p = P_p K_p.
"""
import numpy as np

from stage_ref import EPS, round_up  # noqa: F401  (re-exported for the tests)


def _f(a, dtype):
    return np.asarray(a, dtype=dtype)


def ktile(Z, ell, var, Xp, dtype=np.float64, weight=False):
    """K (M, N) = var exp(-1/2 |z_m / ell - x_n / ell|^2) in the operand form of kf_ktile: both inputs are multiplied by 1 / ell first.
    weight: also eK = |K| (2 + w), w the error weight of the exponent y = -r2 / 2, since exp turns an absolute error of y into a relative
    one of K.  The kernel's operands are the ROUNDED products zs = z / ell and xs = x / ell, so t = zs - xs carries eps (|zs| + |xs| + |t|)
    -- what matters when the inputs lie far from the origin in units of the lengthscale -- and r2 = sum t^2 carries
    2 |t| times that per dimension plus D + 1 roundings of its own:  w = sum_d |t_d| (|zs_d| + |xs_d| + |t_d|) + (D + 1) r2 / 2."""
    inv = 1 / _f(ell, dtype).reshape(-1)
    zs, xs = _f(Z, dtype) * inv, _f(Xp, dtype) * inv
    D = zs.shape[1]
    r2 = np.zeros((zs.shape[0], xs.shape[0]), dtype=dtype)
    w = np.zeros_like(r2)
    for d in range(D):
        t = zs[:, None, d] - xs[None, :, d]
        r2 = r2 + t * t
        if weight:
            w = w + np.abs(t) * (np.abs(zs[:, None, d]) + np.abs(xs[None, :, d]) + np.abs(t))
    K = _f(var, dtype).reshape(()) * np.exp(-r2 / 2)
    return (K, np.abs(K) * (2 + w + (D + 1) * r2 / 2)) if weight else K


class _Tiles:
    """the K and A = P K tiles of one latent with their error weights (module docstring)"""
    def __init__(self, P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype):
        self.P = (_f(P0, dtype), _f(P1, dtype))
        D0 = np.asarray(Z0).shape[1]
        Xn = np.asarray(X)[:N]
        self.Xp = (Xn[:, :D0], Xn[:, D0:])
        kt = (ktile(Z0, ell0, var0, self.Xp[0], dtype, True), ktile(Z1, ell1, var1, self.Xp[1], dtype, True))
        self.K, self.eK = (kt[0][0], kt[1][0]), (kt[0][1], kt[1][1])
        self.A = tuple(self.P[p] @ self.K[p] for p in range(2))
        self.eA = tuple(np.abs(self.P[p]) @ self.eK[p] for p in range(2))
        self.sq = tuple(a * a for a in self.A)
        self.esq = tuple(2 * np.abs(self.A[p]) * self.eA[p] + self.sq[p] for p in range(2))


def forward(P0, P1, Al, S2, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype=np.float64):
    """part [4][N] of k_kf_forward: q0 = k0 . a0, q1 = k1 . a1, mean = k0^T Alpha k1, st = (a0^2)^T S2 (a1^2) per point.
    Returns (part, S), both (4, N)."""
    t = _Tiles(P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype)
    Al, S2 = _f(Al, dtype), _f(S2, dtype)
    K, eK, A, eA = t.K, t.eK, t.A, t.eA
    B0, eB0 = Al @ K[1], np.abs(Al) @ eK[1]
    C0, eC0 = S2 @ t.sq[1], np.abs(S2) @ t.esq[1]
    part = np.stack([(K[0] * A[0]).sum(0), (K[1] * A[1]).sum(0), (K[0] * B0).sum(0), (t.sq[0] * C0).sum(0)])
    S = np.stack([(eK[0] * np.abs(A[0]) + np.abs(K[0]) * eA[0]).sum(0), (eK[1] * np.abs(A[1]) + np.abs(K[1]) * eA[1]).sum(0),
                  (eK[0] * np.abs(B0) + np.abs(K[0]) * eB0).sum(0), (t.esq[0] * np.abs(C0) + t.sq[0] * eC0).sum(0)])
    return part, S


def psi(Xp, zc, dtype=np.float64):
    """Psi (N, 1 + 2 D): the moment columns 1, x_d - zc_d, (x_d - zc_d)^2 of a factor's input columns Xp (N, D)."""
    xc = _f(Xp, dtype) - _f(zc, dtype).reshape(1, -1)
    return np.concatenate([np.ones((xc.shape[0], 1), dtype=dtype), xc, xc * xc], 1)


def backward(P0, P1, Al, S2, Z0, Z1, ell0, ell1, var0, var1, X, N, part, gm, gv, dq0, dq1, zc0, zc1, dtype=np.float64):
    """The sums over points of k_kf_backward (+ k_kf_reduce; larger grids: k_kfl_backward + k_kfl_accum), from the comment block above
    k_kf_backward.  Per point, with gm / gv the cotangents of mean / var and dq_p the cotangent of q_p:
        B0 = Alpha K1, B1 = Alpha^T K0, C0 = S2 A1^2, C1 = S2^T A0^2;  dA_p = 2 gv A_p . C_p;  dK_p = gm B_p + 2 dq_p A_p + P_p dA_p;
        E_p = dq_p K_p + dA_p
        dAl = K0 diag(gm) K1^T;  dS2 = A0^2 diag(gv) (A1^2)^T;  dP_p = E_p K_p^T (unsymmetrised);  Kr_p = (dK_p . K_p) Psi_p  [M_p][1 + 2 D_p]
    `part` is what the forward kernel left; the backward kernel recomputes its tile and does not read it (the argument keeps the call
    of a stage test uniform: the stage's inputs as tapped).  Returns dict name -> (value, S)."""
    del part
    t = _Tiles(P0, P1, Z0, Z1, ell0, ell1, var0, var1, X, N, dtype)
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
        out['Kr%d' % p] = (tt @ Ps[p], (ett + 3 * np.abs(tt)) @ np.abs(Ps[p]))
    return out


def frag_image(A, transposed):
    """kf_write_frag: the A-operand image of v_mfma_f64_16x16x4 of a row-major matrix A (R, C), R and C multiples of 16 --
    F[(rb * ksn + ks) * 64 + lane] = B(16 rb + lane % 16, 4 ks + lane / 16) with B = A (ksn = C / 4) or, transposed, B = A^T (ksn = R / 4)."""
    A = np.asarray(A)
    R, Cc = A.shape
    rows, cols = (Cc, R) if transposed else (R, Cc)
    ksn = cols // 4
    idx = np.arange(rows * cols)
    lane, blk = idx & 63, idx >> 6
    ks, rb = blk % ksn, blk // ksn
    row, k = 16 * rb + (lane & 15), 4 * ks + (lane >> 4)
    return A[k, row] if transposed else A[row, k]


def latent(P0, P1, U, dtype=np.float64):
    """k_kf_latent / k_kfl_latent: T0 = U P1, T1 = P0 U, Alpha = P0 (U P1).  Returns dict name -> (value, S)."""
    P0, P1, U = _f(P0, dtype), _f(P1, dtype), _f(U, dtype)
    T0, aT0 = U @ P1, np.abs(U) @ np.abs(P1)
    return dict(T0=(T0, aT0), T1=(P0 @ U, np.abs(P0) @ np.abs(U)), Al=(P0 @ T0, np.abs(P0) @ aT0))


def work_image(b, M, D, cap):
    """The work block k_kf_reduce writes for one latent (kf_work_layout) from the values of backward(): capacity (nb0c, nb1c) 16-row blocks,
    R_p = 16 nb_pc, ldw = max(R0, R1): dAl [R0][ldw] | dS2 [R0][ldw] | dP0 [R0][ldw] | dP1 [R1][ldw] | Kr0 [R0][16] | Kr1 [R1][16], zero
    wherever the latent's own M0 x M1 grid (and the 1 + 2 D_p moment columns) ends."""
    R0, R1 = 16 * cap[0], 16 * cap[1]
    ldw = max(R0, R1)
    mats = [np.zeros((R0, ldw)), np.zeros((R0, ldw)), np.zeros((R0, ldw)), np.zeros((R1, ldw)), np.zeros((R0, 16)), np.zeros((R1, 16))]
    for m, k in zip(mats, ('dAl', 'dS2', 'dP0', 'dP1', 'Kr0', 'Kr1')):
        v = np.asarray(b[k][0], dtype=np.float64)
        m[:v.shape[0], :v.shape[1]] = v
    return np.concatenate([m.reshape(-1) for m in mats])


def work_split(work, cap):
    """The six matrices of a work block (inverse of work_image's concatenation)."""
    R0, R1 = 16 * cap[0], 16 * cap[1]
    ldw = max(R0, R1)
    shapes = [(R0, ldw), (R0, ldw), (R0, ldw), (R1, ldw), (R0, 16), (R1, 16)]
    out, o = {}, 0
    for k, (r, c) in zip(('dAl', 'dS2', 'dP0', 'dP1', 'Kr0', 'Kr1'), shapes):
        out[k] = np.asarray(work[o:o + r * c]).reshape(r, c)
        o += r * c
    assert o == len(work)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier: inputs with which every K tile is an exact selector and every sum over points is a sum of integers
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT_VAR = {0.0: ((4.0, 16.0), (1.0, 64.0)), 0.25: ((3.75, 0.75), (0.75, 15.75))}      # jitter -> per latent (var0, var1): var + jitter a power of 4


def exact_problem(grid_f, grid_g, D, N, jitter=0.0, seed=0):
    """Inputs of the exact tier and what the kernels must produce from them, bit for bit.

    Inducing inputs of factor p: the first M_p points of a lattice with spacing 64 ell_d in every dimension (digits of the point's index
    in base b_p = ceil(Mmax_p^(1 / D_p))), lengthscales powers of two >= 2^-5 (shared by the latents, so that one X serves both), variances
    EXACT_VAR[jitter].  Then K_p(Z_p, Z_p) + jitter I = c_p I exactly (exp(-2048) underflows to zero), c_p a power of 4, its Cholesky
    factor, inverse and P_p = I / c_p are exact.  Every point sits on one lattice point (i_n, j_n) < (Mmax0, Mmax1) -- outside the grid
    of a latent with fewer points, which then sees it at distance >= 64 lengthscales: a zero tile -- or, every 7th / 11th point, 1000
    lengthscales off the lattice in factor 0 / factor 1.  u in -3 .. 3, s in 1 .. 3, injected cotangents in -3 .. 3 (about a third zeros).
    With h_p = 1 where the point hits inducing point i (j) of factor p, r_p = var_p / c_p:
        part = (h0 var0 r0, h1 var1 r1, h0 h1 r0 r1 u_ij, h0 h1 r0^2 r1^2 s_ij^2)
        dAl_ij += h0 h1 gm var0 var1;  dS2_ij += h0 h1 gv r0^2 r1^2
        dP0_ii += h0 var0 (dq0 var0 + 2 h1 gv r0 r1^2 s_ij^2);  dP1_jj += h1 var1 (dq1 var1 + 2 h0 gv r1 r0^2 s_ij^2)
        Kr0_i. += h0 (h1 gm r0 r1 u_ij + 2 dq0 r0 var0 + 2 h1 gv r0^2 r1^2 s_ij^2) psi_0(x);  Kr1_j. likewise
    (one non-zero term per inner sum).  Returns dict(p, X, Y, lat=[per latent dict(stage, cot, zc, part, sums, U, S2, P, Zs, M)])."""
    rs = np.random.RandomState(seed)
    grids = [grid_f] if grid_g is None else [grid_f, grid_g]
    Mmax = [max(g[q] for g in grids) for q in range(2)]
    base = [int(np.ceil(Mmax[q] ** (1.0 / D[q]) - 1e-9)) for q in range(2)]
    ell = [np.array([2.0 ** (-5 + (d + q) % 3) for d in range(D[q])]) for q in range(2)]

    def lattice(idx, q):
        idx = np.asarray(idx)
        return np.stack([64.0 * ell[q][d] * ((idx // base[q] ** d) % base[q]) for d in range(D[q])], -1)

    ij = [rs.randint(0, Mmax[q], size=N) for q in range(2)]
    Xq = [lattice(ij[q], q) for q in range(2)]
    n = np.arange(N)
    far = [(n % 7 == 3), (n % 11 == 5)]
    for q in range(2):
        Xq[q][far[q], 0] = -1000.0 * ell[q][0]
    X = np.ascontiguousarray(np.hstack(Xq))
    Y = np.where(n % 3 == 0, 0.0, 1.0 + (n % 5))
    p = dict(noise=0.5)
    lat = []
    for h, g in enumerate(grids):
        tag = 'fg'[h]
        var = EXACT_VAR[jitter][h]
        M = tuple(g)
        Z = [lattice(np.arange(M[q]), q) for q in range(2)]
        u = rs.randint(-3, 4, size=M).astype(np.float64)
        s = rs.randint(1, 4, size=M).astype(np.float64)
        cot = rs.randint(-3, 4, size=(4, N)).astype(np.float64) * (rs.rand(4, N) > 0.25)
        p['Z' + tag], p['ell_' + tag], p['var_' + tag] = Z, [e.copy() for e in ell], [np.array([var[0]]), np.array([var[1]])]
        p['u_%sm' % tag], p['u_%ss_sqrt' % tag] = u.reshape(-1, 1), s.reshape(-1, 1)
        c = [var[q] + jitter for q in range(2)]
        r = [var[q] / c[q] for q in range(2)]
        hit = [(~far[q]) & (ij[q] < M[q]) for q in range(2)]
        i, j = np.where(hit[0], ij[0], 0), np.where(hit[1], ij[1], 0)
        h0, h1 = hit[0].astype(np.float64), hit[1].astype(np.float64)
        uij, s2ij = u[i, j], (s * s)[i, j]
        gm, gv, dq0, dq1 = cot
        part = np.stack([h0 * var[0] * r[0], h1 * var[1] * r[1], h0 * h1 * r[0] * r[1] * uij, h0 * h1 * r[0] ** 2 * r[1] ** 2 * s2ij])
        zc = [0.5 * (Z[q].min(0) + Z[q].max(0)) for q in range(2)]
        sums = dict(dAl=np.zeros(M), dS2=np.zeros(M), dP0=np.zeros((M[0], M[0])), dP1=np.zeros((M[1], M[1])),
                    Kr0=np.zeros((M[0], 1 + 2 * D[0])), Kr1=np.zeros((M[1], 1 + 2 * D[1])))
        both = h0 * h1
        np.add.at(sums['dAl'], (i, j), both * gm * var[0] * var[1])
        np.add.at(sums['dS2'], (i, j), both * gv * r[0] ** 2 * r[1] ** 2)
        np.add.at(sums['dP0'], (i, i), h0 * var[0] * (dq0 * var[0] + 2 * h1 * gv * r[0] * r[1] ** 2 * s2ij))
        np.add.at(sums['dP1'], (j, j), h1 * var[1] * (dq1 * var[1] + 2 * h0 * gv * r[1] * r[0] ** 2 * s2ij))
        common = both * (gm * r[0] * r[1] * uij + 2 * gv * r[0] ** 2 * r[1] ** 2 * s2ij)
        t = [h0 * (common + 2 * dq0 * r[0] * var[0]), h1 * (common + 2 * dq1 * r[1] * var[1])]
        for q, idx in enumerate((i, j)):
            np.add.at(sums['Kr%d' % q], idx, t[q][:, None] * psi(Xq[q], zc[q]))
        P = [np.eye(M[q]) / c[q] for q in range(2)]
        lat.append(dict(M=M, var=var, c=c, Z=Z, ell=ell, U=u, S2=s * s, P=P, zc=zc, cot=cot, part=part, sums=sums,
                        Zs=[Z[q] / ell[q] for q in range(2)],
                        stage=(P[0], P[1], u / (c[0] * c[1]), s * s, Z[0], Z[1], ell[0], ell[1], var[0], var[1])))
    return dict(p=p, X=X, Y=Y, lat=lat, D=D, N=N, jitter=jitter)


# ---------------------------------------------------------------------------------------------------------------------------------
# the finish stage: k_kf_latent's KL scalars, the reverse M x M pass (k_kf_finish / k_kfl_finish<1..3>) and the host chain rule
# ---------------------------------------------------------------------------------------------------------------------------------
def kl_scalars(U, Al, s, d0, d1, dtype=np.float64):
    """klv[0..2] of k_kf_latent / k_kfl_latent: sum U . Alpha, sum log s^2, sum d0_i d1_j s_ij^2 (d_p = diag P_p); klv[3], klv[4] are copies
    of the factor kernel's logdets and need no restatement.  Returns dict name -> (value, S).  The logarithm turns the relative rounding of
    s^2 into an absolute eps, and carries one of its own: each term of the second sum weighs |log s^2| + 2."""
    U, Al, s, d0, d1 = _f(U, dtype), _f(Al, dtype), _f(s, dtype), _f(d0, dtype).reshape(-1), _f(d1, dtype).reshape(-1)
    s2 = s * s
    ls = np.log(s2)
    dd = d0[:, None] * d1[None, :] * s2
    return dict(uAl=((U * Al).sum(), (np.abs(U) * np.abs(Al)).sum()), logs2=(ls.sum(), (np.abs(ls) + 2).sum()), ds2=(dd.sum(), np.abs(dd).sum()))


def krow_from_G(G, aG, K, Kr, Z, zc, jitter, dtype=np.float64, _mom=None, _mut=()):
    """The last lines of the finish kernels for one factor: krow [M][2 + 2 D] from the rows of G (M, M) -- aG its error weight, |G| when G
    is taken as given --, K = K_p + jitter I as tapped, the moment block Kr (M, >= 1 + 2 D) around zc, and Z (M, D):
        kz = K - jitter I,  tt = G . kz,  df = z_jd - z_md,  dz = z_md - zc_d
        krow[m][0] = sum_j tt + Kr[m][0];   krow[m][1 + d] = sum_j 2 tt df + Kr[m][1 + d] - dz Kr[m][0]
        krow[m][1 + D + d] = sum_j tt df^2 + Kr[m][1 + D + d] - 2 dz Kr[m][1 + d] + dz^2 Kr[m][0];   krow[m][1 + 2 D] = 0
    _mom = (Kd, eKd, kd): the Matern form (kronf_matern_ref.finish) -- the moment columns take tt' = G . Kd and are re-centred with kd
    (column 15 of the device block) in place of Kr[:, 0].  _mut: the deliberate mistakes of tests/test_cpu_kronf_finish_ref.py.
    Returns (value, S)."""
    G, aG, K, Kr, Z, zc = _f(G, dtype), _f(aG, dtype), _f(K, dtype), _f(Kr, dtype), _f(Z, dtype), _f(zc, dtype).reshape(-1)
    M, D = Z.shape
    eye = np.eye(M, dtype=dtype)
    kz, akz = K - dtype(jitter) * eye, np.abs(K) + dtype(jitter) * eye
    tt, att = G * kz, aG * akz
    if _mom is None:
        tm, atm, c0 = tt, att, Kr[:, 0]
    else:
        Kd, eKd, kd = _f(_mom[0], dtype), _f(_mom[1], dtype), _f(_mom[2], dtype)
        tm, atm, c0 = G * Kd, aG * np.abs(Kd) + np.abs(G) * eKd, kd
    two = dtype(1) if 'no2' in _mut else dtype(2)
    out, S = np.zeros((M, 2 + 2 * D), dtype=dtype), np.zeros((M, 2 + 2 * D), dtype=dtype)
    out[:, 0], S[:, 0] = tt.sum(1) + Kr[:, 0], att.sum(1) + np.abs(Kr[:, 0])
    for d in range(D):
        df = Z[None, :, d] - Z[:, None, d]
        dz = Z[:, d] - zc[d]
        if 'dzsign' in _mut:
            dz = -dz
        k1, k2 = Kr[:, 1 + d], Kr[:, 1 + D + d]
        out[:, 1 + d] = (two * tm * df).sum(1) + k1 - dz * c0
        S[:, 1 + d] = (2 * atm * np.abs(df)).sum(1) + np.abs(k1) + np.abs(dz) * np.abs(c0)
        out[:, 1 + D + d] = (tm * df * df).sum(1) + k2 - 2 * dz * k1 + dz * dz * c0
        S[:, 1 + D + d] = (atm * df * df).sum(1) + np.abs(k2) + 2 * np.abs(dz) * np.abs(k1) + dz * dz * np.abs(c0)
    return out, S


def finish(w, K0, K1, P0, P1, U, S2, T0, T1, Al, s, Z0, Z1, zc0, zc1, jitter, kl, dtype=np.float64, _mom=(None, None), _mut=()):
    """The reverse M x M pass, from the comment block above KfFinishJob (csrc/zigp_kronf.hip) and the kernel text.  w: the six matrices of
    the work block trimmed to the latent's own grid (dAl, dS2 (M0, M1), dP_p (M_p, M_p), Kr_p (M_p, >= 1 + 2 D_p)); K_p as tapped (jitter
    included), P_p, U, S2, T0, T1, Al (M0, M1) as tapped, s (M0, M1), kl: include_kl.  Per factor p, o the other one, d_p = diag P_p:
        dP0' = dP0 + dAl T0^T, dP1' = dP1 + T1^T dAl;  Q0 = T0 U^T, Q1 = U^T T1;  w0_i = sum_j d1_j S2_ij, w1_j = sum_i d0_i S2_ij
        X = sym(dP') - kl (1/4 (Q + Q^T) + 1/2 diag w);   PXP = P X P;   G = -PXP - kl 1/2 M_o P;   krow_p = krow_from_G(G, ...)
        gu = P0 dAl P1 - kl Alpha;   gs = 2 s dS2 - kl (-1 / s + d0_i d1_j s)
    Returns dict name -> (value, S) for krow0, krow1, gu, gs, G0, G1, PXP0, PXP1 (what k_kfl_finish<3> leaves for factor 1).  S: the nested sum
    of absolute values; the inputs are the stage's own and enter with their magnitudes."""
    P = (_f(P0, dtype), _f(P1, dtype))
    K, Z, zc = (K0, K1), (Z0, Z1), (zc0, zc1)
    U, S2, T0, T1, Al, s = (_f(a, dtype) for a in (U, S2, T0, T1, Al, s))
    dAl, dS2 = _f(w['dAl'], dtype), _f(w['dS2'], dtype)
    M = (P[0].shape[0], P[1].shape[0])
    dv = (np.diag(P[0]), np.diag(P[1]))
    klf = dtype(1 if kl else 0)
    aU, adAl = np.abs(U), np.abs(dAl)
    dP = (_f(w['dP0'], dtype) + dAl @ T0.T, _f(w['dP1'], dtype) + T1.T @ dAl)
    adP = (np.abs(_f(w['dP0'], dtype)) + adAl @ np.abs(T0).T, np.abs(_f(w['dP1'], dtype)) + np.abs(T1).T @ adAl)
    Q, aQ = (T0 @ U.T, U.T @ T1), (np.abs(T0) @ aU.T, aU.T @ np.abs(T1))
    wv, awv = (S2 @ dv[1], S2.T @ dv[0]), (np.abs(S2) @ np.abs(dv[1]), np.abs(S2).T @ np.abs(dv[0]))
    out = {}
    for p in range(2):
        aP = np.abs(P[p])
        X = dP[p] if 'nosym' in _mut else (dP[p] + dP[p].T) / 2
        aX = (adP[p] + adP[p].T) / 2
        if kl:
            if 'noQ' not in _mut:
                X = X - (Q[p] + Q[p].T) / 4
            X = X - np.diag(wv[p]) / 2
            aX = aX + (aQ[p] + aQ[p].T) / 4 + np.diag(awv[p]) / 2
        PXP, aPXP = P[p] @ X @ P[p], aP @ aX @ aP
        coef = klf * dtype(M[p] if 'coefMp' in _mut else M[1 - p]) / 2
        G, aG = -PXP - coef * P[p], aPXP + coef * aP
        out['PXP%d' % p], out['G%d' % p] = (PXP, aPXP), (G, aG)
        out['krow%d' % p] = krow_from_G(G, aG, K[p], w['Kr%d' % p], Z[p], zc[p], jitter, dtype, _mom[p], _mut)
    out['gu'] = (P[0] @ dAl @ P[1] - klf * Al, np.abs(P[0]) @ adAl @ np.abs(P[1]) + klf * np.abs(Al))
    dd = dv[0][:, None] * dv[1][None, :] * s
    out['gs'] = (2 * s * dS2 - klf * (-1 / s + dd), 2 * np.abs(s * dS2) + klf * (1 / np.abs(s) + np.abs(dd)))
    return out


def assemble(krow, gu, gs, ell, var, s_gv, dtype=np.float64):
    """kron_assemble_grads (csrc/zigp_kronc.h) for one latent: the host chain rule from krow_p (M_p, 2 + 2 D_p), gu, gs and s_gv, the sum of the
    variance cotangents over the points:  dZ_p = krow[:, 1 : 1 + D] / ell^2;  d ell_p = sum_m krow[:, 1 + D : 1 + 2 D] / ell^3;
    d var_p = sum_m krow[:, 0] / var_p + s_gv var_other;  d u = gu, d s = gs.  Returns dict name -> (value, S) with Z, ell, var lists over p."""
    out = dict(Z=[], ell=[], var=[], u=(_f(gu, dtype), np.abs(_f(gu, dtype))), s=(_f(gs, dtype), np.abs(_f(gs, dtype))))
    sg = _f(s_gv, dtype).reshape(())
    for p in range(2):
        kr, l, v = _f(krow[p], dtype), _f(ell[p], dtype).reshape(-1), _f(var[p], dtype).reshape(())
        D = l.size
        dZ = kr[:, 1:1 + D] / (l * l)
        out['Z'].append((dZ, np.abs(dZ)))
        out['ell'].append((kr[:, 1 + D:1 + 2 * D].sum(0) / (l * l * l), np.abs(kr[:, 1 + D:1 + 2 * D]).sum(0) / (l * l * l)))
        vo = _f(var[1 - p], dtype).reshape(())
        out['var'].append((kr[:, 0].sum() / v + sg * vo, np.abs(kr[:, 0]).sum() / v + np.abs(sg) * vo))
    return out


def moment_block16(Kr, Kd=None):
    """the 16-column device moment block of a factor from backward()'s Kr (M, 1 + 2 D) and, for a Matern factor, Kd (M) in column 15"""
    out = np.zeros((Kr.shape[0], 16))
    out[:, :Kr.shape[1]] = Kr
    if Kd is not None:
        out[:, 15] = Kd
    return out


def exact_finish(L, D, jitter, kl, dtype=np.float64):
    """finish() on the values an exact-tier step hands its finish stage (L: one latent of exact_problem): K_p + jitter I = c_p I,
    P_p = I / c_p, T0 = U / c_1, T1 = U / c_0, Alpha = U / (c_0 c_1), the integer sums over points.  tests/test_cpu_kronf_finish_ref.py shows
    which of its results are exact in float64 (all of them with kl off; with kl on all but gs where s = 3, see exact_gs_mask)."""
    M, c = L['M'], L['c']
    s = np.sqrt(L['S2'])
    w = dict(L['sums'])
    for q in range(2):
        w['Kr%d' % q] = moment_block16(L['sums']['Kr%d' % q])
    K = [c[q] * np.eye(M[q]) for q in range(2)]
    return finish(w, K[0], K[1], L['P'][0], L['P'][1], L['U'], L['S2'], L['U'] / c[1], L['U'] / c[0], L['U'] / (c[0] * c[1]), s,
                  L['Z'][0], L['Z'][1], L['zc'][0], L['zc'][1], jitter, kl, dtype=dtype)


def exact_gs_mask(L):
    """where gs is exact with kl on: -1 / s is a dyadic number for s in {1, 2} and not for s = 3"""
    return np.sqrt(L['S2']) != 3.0
