"""Host references of the dense chunk loop's stages and of the M x M stage that opens and closes a step, one plain numpy statement per
stage or launch, each with the rounding bound its GPU twin is held to (tests/test_gpu_stages.py, tests/test_gpu_mxm_stages.py).  Written from the formulas in the kernel comments (csrc/zigp_dense.hip header, csrc/zigp_gemm.h epilogues,
csrc/zigp_kernels.h k_pointwise / k_kgrad / k_sym_from_planes) and the oracle (oracle/zigp_oracle.py); tests/test_cpu_stage_ref.py pins their
composition to the oracle on the CPU, so a GPU-vs-stage_ref failure means the kernel is wrong and not the test's idea of the operation.

Bounds.  eps = 2^-53 (unit roundoff), gamma_k = k eps / (1 - k eps).  A sum of k products evaluated in ANY order, with or without fma,
is within gamma_k sum |a_i b_i| of its exact value (Higham, Accuracy and Stability, 3.1 / 3.5).  Two evaluations of the same sum (the
GPU's and a float64 BLAS one) are therefore within 2 gamma_k sum |a_i b_i| of each other; the bounds below carry k + 2 (one spare rounding per
side for a scaling such as alpha or the k-scale) and are written next to the reference they belong to.  Every stage is checked against
the operands ITS kernel reads (the J' and A2 references take the A1 panel the GPU stored), so each bound is that of one product.
"""
import numpy as np

EPS = 2.0 ** -53
LOG2PI = 1.8378770664093454836
C1, C0 = 1.0 - 2.e-3, 1.e-3          # the probit floor of OnOffSVGP.py:178


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def round_up(n, m):
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------------------
# forward products (chunk_forward): A1 = W K, sum_m v A1, sum_m A1^2; value mode: A2 = W^T A1, sum_m s^2 A2^2; gradient mode:
# J' = Rt^T A1 (Rt = (Q W^T)^T), sum_m K J'
# ---------------------------------------------------------------------------------------------------------------------------------
def forward_a1(W, v, K):
    """A1 = W K (W lower triangular, M x M; K M x Nc) with the fused sums.  Returns dict of (value, bound) pairs.
    panel: |gpu - ref| <= 2 gamma_(k+2) (|W||K|)_ij, k = M terms.
    sum v A1: the inner error gamma_(k+2) |v_m| (|W||K|)_mj per term plus the outer sum over Mp rows: gamma_(k+Mp+4) sum_m |v_m| (|W||K|)_mj, doubled.
    sum A1^2: squaring doubles the inner relative error (2 k), so gamma_(2k+Mp+4) sum_m (|W||K|)^2_mj, doubled."""
    M = W.shape[0]
    Mp = round_up(M, 128)
    A1 = W @ K
    B = np.abs(W) @ np.abs(K)
    return dict(A1=(A1, 2 * gamma(M + 2) * B),
                s_vA1=(v @ A1, 2 * gamma(M + Mp + 4) * (np.abs(v) @ B)),
                s_A1sq=(np.sum(A1 * A1, 0), 2 * gamma(2 * M + Mp + 4) * np.sum(B * B, 0)))


def forward_a2(W, s2, A1):
    """sum_m s2_m A2_mj^2, A2 = W^T A1 (A1: the panel the kernel reads).  Bound as sum A1^2 with the weights' magnitudes:
    2 gamma_(2k+Mp+4) sum_m |s2_m| (|W^T||A1|)^2_mj."""
    M = W.shape[0]
    Mp = round_up(M, 128)
    A2 = W.T @ A1
    B = np.abs(W.T) @ np.abs(A1)
    return dict(A2=(A2, 2 * gamma(M + 2) * B), s_s2A2sq=(s2 @ (A2 * A2), 2 * gamma(2 * M + Mp + 4) * (np.abs(s2) @ (B * B))))


def forward_jp(Rt, K, A1):
    """J' = Rt^T A1 (full product) and sum_m K_mj J'_mj (EpiStorePanelKColsum).  panel: 2 gamma_(k+2) (|Rt^T||A1|)_ij;
    sum K J': inner gamma_(k+2) per term, one product and the outer sum over Mp rows: 2 gamma_(k+Mp+4) sum_m |K_mj| (|Rt^T||A1|)_mj."""
    M = Rt.shape[0]
    Mp = round_up(M, 128)
    Jp = Rt.T @ A1
    B = np.abs(Rt.T) @ np.abs(A1)
    return dict(Jp=(Jp, 2 * gamma(M + 2) * B), s_KJ=(np.sum(K * Jp, 0), 2 * gamma(M + Mp + 4) * np.sum(np.abs(K) * B, 0)))


# ---------------------------------------------------------------------------------------------------------------------------------
# rank-N update (latent_chunk_syrk + k_sym_from_planes): C1 = sum_chunks A1 diag(gv) A1^T, symmetric
# ---------------------------------------------------------------------------------------------------------------------------------
def rank_update(chunks):
    """chunks: [(A1 (M,Nc_i), gv (Nc_i))].  Bound: one sum of k = sum Nc_i products a_in (gv_n a_jn) -- the k-scale is one more rounding per
    term, the split-K planes and the chunk-after-chunk accumulation only reorder the sum: 2 gamma_(k+2) (|A1| diag|gv| |A1|^T)_ij."""
    M = chunks[0][0].shape[0]
    C, B, k = np.zeros((M, M)), np.zeros((M, M)), 0
    for A1, gv in chunks:
        C += (A1 * gv[None, :]) @ A1.T
        B += (np.abs(A1) * np.abs(gv)[None, :]) @ np.abs(A1).T
        k += A1.shape[1]
    return C, 2 * gamma(k + 2) * B


def syr_plan(nbm):
    """The split-K plan table of the issue, restated (NOT read from the library): off-diagonal slices So, diagonal Sd = So / 2, the
    largest multiple of 16 in [16, 64] with (n_off + n_diag / 2) So <= 512 workgroups."""
    n_off, n_d = nbm * (nbm - 1) // 2, nbm
    So = int(512 / (n_off + 0.5 * n_d)) // 16 * 16
    So = max(16, min(64, So))
    while So > 16 and n_off * So + n_d * (So // 2) > 512:
        So -= 16
    return So, So // 2


def slice_windows(nk, S):
    """k windows (in columns) of the S slices of a tile over nk BK = 16 steps (syr2k_tiles)."""
    return [(16 * (nk * s // S), 16 * (nk * (s + 1) // S)) for s in range(S)]


# ---------------------------------------------------------------------------------------------------------------------------------
# Kuf cotangent reductions (k_kgrad): F = alpha gm^T + 2 J' diag(gv);  krow[m] = [sum F K, sum F K (x - z_m), sum F K (x - z_m)^2, sum K gm]
# over the columns n < min(Nc, Nrows - n0)
# ---------------------------------------------------------------------------------------------------------------------------------
def kgrad(Jp, K, alpha, gm, gv, X, Z, n0, centre=None, dtype=np.float64):
    """Returns (krow (M, 2+2D), bound).  dtype = np.longdouble gives the extended-precision reference.
    Bound of the GPU side alone (the caller adds the reference's own: the same expression for float64, 2^-11 of it for longdouble): with
    T_mn = (|alpha_m gm_n| + 2 |gv_n J'_mn|) |K_mn| and n the number of valid columns, gamma_(n+8) sum_n T_mn (|x_n - c| + |z_m - c|)^p,
    p = 0, 1, 2 -- the moments are summed about c and moved to z_m after the sum (S1 - dz S0, S2 - 2 dz S1 + dz^2 S0: every term of the
    expansion of ((x - c) - dz)^p enters with its magnitude); c = z_m, i.e. no second term, for the per-row (EXACT) form.  The 8 spare
    roundings: F (3), x - c and its square (3), the shift (2).  Last column, sum_n K gm: gamma_(n+2) sum |K gm|."""
    M, D = Z.shape
    Nc = K.shape[1]
    nv = max(0, min(Nc, X.shape[0] - n0))
    f = lambda a: np.asarray(a, dtype=dtype)
    Jp, K, alpha, gm, gv, Xc, Zc = f(Jp)[:, :nv], f(K)[:, :nv], f(alpha), f(gm)[:nv], f(gv)[:nv], f(X)[n0:n0 + nv], f(Z)
    F = alpha[:, None] * gm[None, :] + 2 * gv[None, :] * Jp
    t = F * K
    T = (np.abs(alpha)[:, None] * np.abs(gm)[None, :] + 2 * np.abs(gv)[None, :] * np.abs(Jp)) * np.abs(K)
    out, bnd = np.zeros((M, 2 + 2 * D), dtype=dtype), np.zeros((M, 2 + 2 * D), dtype=dtype)
    out[:, 0], bnd[:, 0] = t.sum(1), T.sum(1)
    for d in range(D):
        df = Xc[None, :, d] - Zc[:, None, d]
        out[:, 1 + d], out[:, 1 + D + d] = (t * df).sum(1), (t * df * df).sum(1)
        if centre is None:
            mag = np.abs(df)
        else:
            mag = np.abs(Xc[None, :, d] - f(centre)[d]) + np.abs(Zc[:, None, d] - f(centre)[d])
        bnd[:, 1 + d], bnd[:, 1 + D + d] = (T * mag).sum(1), (T * mag * mag).sum(1)
    out[:, 1 + 2 * D] = (K * gm[None, :]).sum(1)
    bnd = gamma(nv + 8) * bnd
    bnd[:, 1 + 2 * D] = gamma(nv + 2) * (np.abs(K) * np.abs(gm)[None, :]).sum(1)
    return out, np.asarray(bnd, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# point-wise stage (k_pointwise)
# ---------------------------------------------------------------------------------------------------------------------------------
PW_GROUPS = 4


def pw_plane_sum(plane, nrows):
    """The kernel's sum of the first nrows partial rows of one plane [np][Nc], in its order: wave g adds the rows g, g + 4, ... from 0,
    then the four group sums are added in group order.  Replicated operation by operation, so the result is the kernel's double."""
    grp = []
    for g in range(PW_GROUPS):
        a = np.zeros(plane.shape[1])
        for q in range(g, nrows, PW_GROUPS):
            a = a + plane[q]
        grp.append(a)
    return ((grp[0] + grp[1]) + grp[2]) + grp[3]


def pw_inputs(part_f, part_g, np1, np2, var_f, var_g, g_offset, gradvar, mean=None, X=None, n0=0, row_end=None):
    """(fm, fv, gm, gv) as the kernel forms them from the planes: fm = plane 0 (+ mean function), fv = var + plane 2 (gradient step) or
    var - plane 1 + plane 2.  The mean function is a chain of fma in the kernel; it is NOT replicated here bit for bit (numpy has no fma):
    callers that need bit-equality use mean = None."""
    Nc = part_f.shape[2]
    fm, gmn = pw_plane_sum(part_f[0], np1[0]), pw_plane_sum(part_g[0], np1[1])
    f2, g2 = pw_plane_sum(part_f[2], np2[0]), pw_plane_sum(part_g[2], np2[1])
    if gradvar:
        fv, gv = var_f + f2, var_g + g2
    else:
        fv, gv = var_f - pw_plane_sum(part_f[1], np1[0]) + f2, var_g - pw_plane_sum(part_g[1], np1[1]) + g2
    gmn = gmn + g_offset
    if mean is not None:
        a, b = mean
        xs = np.zeros((Nc, X.shape[1]))
        nv = max(0, min(Nc, row_end - n0))
        xs[:nv] = X[n0:n0 + nv]
        fm = fm + (b + xs @ np.asarray(a, dtype=np.float64).reshape(-1))
    return fm, fv, gmn, gv


PW_OUTPUTS = ('e1', 'e2', 'ev', 'gfmean', 'gfvar', 'gfmeanu', 've', 'dnoise', 'dfm', 'dfv', 'dgm', 'dgv')


def pointwise_np(fm, fv, gm, gv, y, noise):
    """float64 numpy: the forward part IS the oracle (probit_expectations, variational_expectations); the reverse pass is the chain
    rule of those formulas (z = gm / sqrt(1 + gv), a = 1 / sqrt(1 + 2 gv), cdf = c1 Phi(z) + c0, T = atan(a) / (2 pi) exp(-z^2 (a^2 + 1) / 2),
    e1 = cdf, e2 = clip(cdf - 2 T), ev = clip(cdf - 2 T - cdf^2); F = var_exp):
      dF/dgfmean = (y - gfmean) / noise, dF/dgfvar = dF/dgfmeanu = -1 / (2 noise)
      dfm = dFmu e1 + 2 dFv ev fm, dfv = dFv e2;  de1 = dFmu fm, de2 = dFv fv, dev = dFv fm^2
      dcdf = de1 + de2 + dev (1 - 2 cdf), dT = -2 (de2 + dev)   (clipped branches pass nothing)
      dcdf/dz = c1 phi(z), dT/dz = -z (a^2 + 1) T, dT/da = exp(.) / (2 pi (1 + a^2)) - z^2 a T
      dz/dgm = 1 / sqrt(1 + gv), dz/dgv = -z / (2 (1 + gv)), da/dgv = -a^3."""
    import zigp_oracle as zo
    e1, e2, ev = zo.probit_expectations(gm, gv)
    gfmean, gfvar, gfmeanu = e1 * fm, e2 * fv, ev * fm * fm
    ve = zo.variational_expectations(gfmean, gfvar, gfmeanu, y, noise)
    z = gm / np.sqrt(1. + gv)
    a = 1 / np.sqrt(1. + 2 * gv)
    cdf = e1
    ex = np.exp(-0.5 * (z * z) * (a * a + 1.0))
    T = np.arctan(a) / (2 * np.pi) * ex
    m2 = np.where(cdf - 2 * T > 0, 1.0, 0.0)
    mv = np.where(cdf - 2 * T - cdf * cdf > 0, 1.0, 0.0)
    res = y - gfmean
    q = res * res + gfvar + gfmeanu
    dFmu, dFv = res / noise, -0.5 / noise
    dnoise = -0.5 / noise + 0.5 * q / (noise * noise)
    dfm = dFmu * e1 + dFv * ev * 2.0 * fm
    dfv = dFv * e2
    de1, de2, dev = dFmu * fm, dFv * fv, dFv * fm * fm
    dcdf = de1 + de2 * m2 + dev * mv * (1.0 - 2.0 * cdf)
    dT = -2.0 * (de2 * m2 + dev * mv)
    phi = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    dTdz = -z * (a * a + 1.0) * T
    dTda = ex / (2 * np.pi * (1.0 + a * a)) - z * z * a * T
    dz = dcdf * C1 * phi + dT * dTdz
    dgm = dz / np.sqrt(1. + gv)
    dgv = dz * (-0.5 * z / (1. + gv)) + dT * dTda * (-(a ** 3))
    return dict(e1=e1, e2=e2, ev=ev, gfmean=gfmean, gfvar=gfvar, gfmeanu=gfmeanu, ve=ve, dnoise=dnoise, dfm=dfm, dfv=dfv, dgm=dgm, dgv=dgv)


def pointwise_mp(fm, fv, gm, gv, y, noise, dps=50):
    """The same formulas at 50 digits (mpmath), point by point; returns dict of object arrays of mpf."""
    import mpmath as mp
    mp.mp.dps = dps
    n = len(fm)
    out = {k: np.empty(n, dtype=object) for k in PW_OUTPUTS}
    c1, c0, one, half, two = mp.mpf(1) - mp.mpf('2e-3'), mp.mpf('1e-3'), mp.mpf(1), mp.mpf('0.5'), mp.mpf(2)
    noise = mp.mpf(float(noise))
    for i in range(n):
        f_, v_, g_, w_, y_ = (mp.mpf(float(x[i])) for x in (fm, fv, gm, gv, y))
        z = g_ / mp.sqrt(one + w_)
        a = one / mp.sqrt(one + two * w_)
        cdf = half * (one + mp.erf(z / mp.sqrt(two))) * c1 + c0
        ex = mp.exp(-half * z * z * (a * a + one))
        T = mp.atan(a) / (two * mp.pi) * ex
        e2r, evr = cdf - two * T, cdf - two * T - cdf * cdf
        m2, mv = (one if e2r > 0 else mp.mpf(0)), (one if evr > 0 else mp.mpf(0))
        e1, e2, ev = cdf, (e2r + abs(e2r)) / two, (evr + abs(evr)) / two
        gfmean, gfvar, gfmeanu = e1 * f_, e2 * v_, ev * f_ * f_
        res = y_ - gfmean
        q = res * res + gfvar + gfmeanu
        ve = -half * mp.log(two * mp.pi) - half * mp.log(noise) - half * q / noise
        dFmu, dFv = res / noise, -half / noise
        dnoise = -half / noise + half * q / (noise * noise)
        dfm = dFmu * e1 + dFv * ev * two * f_
        dfv = dFv * e2
        de1, de2, dev = dFmu * f_, dFv * v_, dFv * f_ * f_
        dcdf = de1 + de2 * m2 + dev * mv * (one - two * cdf)
        dT = -two * (de2 * m2 + dev * mv)
        phi = mp.exp(-half * z * z) / mp.sqrt(two * mp.pi)
        dTdz = -z * (a * a + one) * T
        dTda = ex / (two * mp.pi * (one + a * a)) - z * z * a * T
        dz = dcdf * c1 * phi + dT * dTdz
        dgm = dz / mp.sqrt(one + w_)
        dgv = dz * (-half * z / (one + w_)) + dT * dTda * (-(a ** 3))
        for k, val in zip(PW_OUTPUTS, (e1, e2, ev, gfmean, gfvar, gfmeanu, ve, dnoise, dfm, dfv, dgm, dgv)):
            out[k][i] = val
    return out


def pointwise_scales(fm, fv, gm, gv, y, noise):
    """S, the natural scale of each output: the probit moments are O(1) quantities computed with absolute error (c0 floor, cancellation in
    cdf - 2 T - cdf^2), so they enter every expression with magnitude 1; everything else with the sum of the magnitudes of the terms of
    its defining expression.  dgm / dgv: (|dF/de1| + |dF/de2| + |dF/dev|) times |dz/dgm| = 1 / sqrt(1 + gv) resp. the 1 / (1 + gv) that
    bounds |dz/dgv|, |da/dgv| and the derivative factors next to them."""
    fm, fv, y = np.abs(fm), np.abs(fv), np.abs(y)
    one = np.ones_like(fm)
    Q = (y + fm) ** 2 + fv + fm * fm
    dF = ((y + fm) * fm + 0.5 * fv + 0.5 * fm * fm) / noise
    return dict(e1=one, e2=one, ev=one, gfmean=fm, gfvar=fv, gfmeanu=fm * fm,
                ve=0.5 * LOG2PI + 0.5 * abs(np.log(noise)) + 0.5 * Q / noise,
                dnoise=0.5 / noise + 0.5 * Q / noise ** 2,
                dfm=(y + fm) / noise + fm / noise, dfv=0.5 / noise * one,
                dgm=dF / np.sqrt(1. + gv), dgv=dF / (1. + gv))


def mp_err(x, ref):
    """|x - ref| as float64 (ref: object array of mpf)."""
    import mpmath as mp
    return np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(np.asarray(x, dtype=np.float64).reshape(-1), ref)])


def mp_float(ref):
    return np.array([float(b) for b in ref])


# ---------------------------------------------------------------------------------------------------------------------------------
# localisation of a failing element: the message is the point of the exercise
# ---------------------------------------------------------------------------------------------------------------------------------
def locate(i, j):
    return 'row %d col %d = row block %d, column panel %d, 16 x 16 sub-tile (%d, %d)' % (i, j, i // 128, j // 128, i % 128 // 16, j % 128 // 16)


def worst(err, bound):
    """(ratio, flat index) of the largest err / bound; an error against a zero bound is infinite, 0 / 0 is 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    k = int(np.argmax(r))
    return float(r.reshape(-1)[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# M x M reverse stage (latent_mxm_backward, latent_mxm_backward_white): a chain of split-K products (run_gemm_sk), each with a k range
# per 128 x 128 output tile, the finishers SK_STORE (plain or lower tiles only) and SK_PHI, and element-wise / reduction kernels between
# them; then k_kuu_grad[_wide] into slab 0 of krow and k_dense_pack.
# ---------------------------------------------------------------------------------------------------------------------------------
BM, BK, KB = 128, 16, 8          # tile edge, k step, k steps per tile edge
KG_SPLIT = 4

# The k range of tile (bi, bj) of each product in BK steps, nb row blocks (None: the tile is not computed), restated from the comments at
# the launches (NOT read from the library).  Each range skips only blocks in which one factor is structurally zero.
SK_RANGES = {
    'y':     lambda bi, bj, nb: (bj * KB, nb * KB),                              # A W, W lower triangular: k >= j
    'tt':    lambda bi, bj, nb: (0, (min(bi, bj) + 1) * KB),                     # A B^T, both lower triangular: k <= min(i, j)
    'full':  lambda bi, bj, nb: (0, nb * KB),
    'r':     lambda bi, bj, nb: (bi * KB, nb * KB) if bj <= bi else None,        # lower_up: A^T B, A lower triangular (k >= i), lower tiles
    'rfull': lambda bi, bj, nb: (0, nb * KB) if bj <= bi else None,              # lower_all: dense A^T, lower tiles
    't':     lambda bi, bj, nb: (bj * KB, (bi + 1) * KB) if bj <= bi else None,  # Q W: Q lower (k <= i), W lower (k >= j), lower tiles
    's':     lambda bi, bj, nb: (max(bi, bj) * KB, nb * KB),                     # W^T B, B zero above the diagonal tiles: k >= max(i, j)
    'rt':    lambda bi, bj, nb: (0, (bi + 1) * KB),                              # W B, W lower triangular: k <= i
}


def sk_slices(name, nb):
    """run_gemm_sk's slice rule: S = max(1, min(8, shortest k range in BK steps, 512 // computed tiles)) slices per tile."""
    rng = [SK_RANGES[name](bi, bj, nb) for bi in range(nb) for bj in range(nb)]
    rng = [r for r in rng if r is not None and r[1] > r[0]]
    return max(1, min(8, min(k1 - k0 for k0, k1 in rng), 512 // len(rng)))


def sk_windows(name, nb, bi, bj):
    """The k windows (in BK steps) of tile (bi, bj)'s slices, in plane order: k0 + len s // S .. k0 + len (s + 1) // S."""
    r = SK_RANGES[name](bi, bj, nb)
    if r is None:
        return []
    S, (k0, k1) = sk_slices(name, nb), r
    return [(k0 + (k1 - k0) * s // S, k0 + (k1 - k0) * (s + 1) // S) for s in range(S)]


def sk_terms(name, M):
    """(M, M) array: the number of terms of the k range of the tile an element lies in (0: the tile is not computed)."""
    nb = round_up(M, BM) // BM
    t = np.zeros((nb, nb))
    for bi in range(nb):
        for bj in range(nb):
            r = SK_RANGES[name](bi, bj, nb)
            t[bi, bj] = 0 if r is None else BK * (r[1] - r[0])
    return np.kron(t, np.ones((BM, BM)))[:M, :M]


def lower_tiles(M):
    """True where the 128 x 128 tile of an element is on or below the diagonal of tiles."""
    b = np.arange(M) // BM
    return b[:, None] >= b[None, :]


def phi(X):
    """Phi of the Cholesky reverse: the strict lower triangle plus half the diagonal."""
    return np.tril(X, -1) + 0.5 * np.diag(np.diag(X))


def sk_product(name, A, B, lower_only=False, post=None):
    """One split-K product C = A B (A, B: the (M, M) factors AS MULTIPLIED, any transposition applied by the caller) of the reverse stage:
    the whole sum -- a range that is right leaves out structural zeros only, so a range that is short shows as an error -- in the tiles
    the launch computes, zero in the others (lower_only: SK_STORE / SK_PHI define them as zero); post = phi for SK_PHI.
    Bound 2 gamma_(k+2) (|A||B|), k = the terms of the tile's own k range."""
    M = A.shape[0]
    C, Bd = A @ B, 2 * gamma(sk_terms(name, M) + 2) * (np.abs(A) @ np.abs(B))
    if lower_only:
        C, Bd = np.where(lower_tiles(M), C, 0.0), np.where(lower_tiles(M), Bd, 0.0)
    if post is not None:
        C, Bd = post(C), np.tril(Bd)
    return C, Bd


def kuu_grad(G, Kuu, jitter, Z):
    """k_kuu_grad / k_kuu_grad_wide: with Kz = Kuu - jitter I and t_ij = G_ij Kz_ij, the row sums [sum_j t, sum_j 2 t (z_jd - z_id),
    sum_j t (z_id - z_jd)^2, 0] (M, 2 + 2D).  Sums of M terms, each with at most 5 roundings: gamma_(M+5) sum_j |t| |dz|^p."""
    M, D = Z.shape
    Kz = Kuu - jitter * np.eye(M)
    t, T = G * Kz, np.abs(G * Kz)
    out, bnd = np.zeros((M, 2 + 2 * D)), np.zeros((M, 2 + 2 * D))
    out[:, 0], bnd[:, 0] = t.sum(1), T.sum(1)
    for d in range(D):
        df = Z[None, :, d] - Z[:, None, d]
        out[:, 1 + d], out[:, 1 + D + d] = (2 * t * df).sum(1), (t * df * df).sum(1)
        bnd[:, 1 + d], bnd[:, 1 + D + d] = (2 * T * np.abs(df)).sum(1), (T * df * df).sum(1)
    return out, 2 * gamma(M + 5) * bnd


MXM_MODES = ('diag', 'white', 'white_full')
# which k-range rule (SK_RANGES) the launch behind a tap runs, per parametrisation
MXM_PRODUCTS = {'diag': dict(Y='y', T='tt', U='full', R='r', Q='r', QW='t', S='s', P='s', PSP='full'),
                'white': dict(R='r', Q='r', QW='t', S='s'),
                'white_full': dict(Y='y', R='rfull', Q='r', QW='t', S='s')}


def mxm_backward(op, mode='diag', with_data=True, with_kl=True, given=None):
    """The reverse stage of one latent, one numpy statement per launch, in launch order.  op: W, L (lower triangular), Kuu, Z, s ((M), or Lq
    (M, M) for 'white_full'), alpha, v ('diag'), C1 (symmetric), krow [4][>= M][2 + 2D] (initial values; the slabs' column 1 + 2D sums
    to K gm), jitter, P (optional, 'diag': W^T W from the forward stage; absent: the stage forms it).
    given = None: the chain -- every launch reads what the statements before it produced.  given = {name: array} (the GPU's taps and
    outputs): every launch reads the operands ITS kernel read, so each bound is that of one launch.
    Returns {name: (value, bound)} in launch order.  The chain, written out:
      diag:        a1gm = W (K gm), du = W^T a1gm, dsq = diag(W^T C1 W), T = W diag(s^2) W^T, V = T C1 + C1 T - C1,
                   dL = -tril(alpha a1gm^T + du v^T + 2 W^T V), S = W^T Phi(L^T dL) W, G = sym(S) - [kl] 1/2 (P - alpha alpha^T - P diag(s^2) P)
      white:       a1gm = W (K gm), dsq = diag(C1), dL = -tril(alpha a1gm^T + 2 (W^T D) C1), D = diag(s^2 - 1), G = sym(S)
      white_full:  dLq = tril(2 C1 Lq) - [kl] (tril(Lq) - diag(1 / Lq_ii)), dL = -tril(alpha a1gm^T + 2 W^T (Lq Lq^T - I) C1), G = sym(S)
      krow slab 0 += k_kuu_grad(G)."""
    W, L, Kuu, Z, alpha = (np.asarray(op[k], dtype=np.float64) for k in ('W', 'L', 'Kuu', 'Z', 'alpha'))
    M, D = Z.shape
    r = {}

    def get(name):
        return given[name] if given is not None and name in given else r[name][0]

    def put(name, val, bnd):
        r[name] = (val, bnd)

    krow0 = np.array(op['krow'], dtype=np.float64)
    full = mode == 'white_full'
    if full:
        Lq = np.tril(op['s'])
        TmI = Lq @ Lq.T - np.eye(M)
    else:
        s2 = np.asarray(op['s'], dtype=np.float64) ** 2
    if with_data:
        C1in = np.asarray(op['C1'], dtype=np.float64)
        col = krow0[:, :M, 1 + 2 * D]
        kgm = ((col[0] + col[1]) + col[2]) + col[3]                                      # k_gather, slab order
        put('a1gm', np.tril(W) @ kgm, 2 * gamma(M + 2) * (np.abs(np.tril(W)) @ np.abs(kgm)) + gamma(3) * np.abs(W) @ np.abs(col).sum(0))
        if mode == 'diag':
            put('du', W.T @ get('a1gm'), 2 * gamma(M + 2) * (np.abs(W.T) @ np.abs(get('a1gm'))))  # k_gemv_cols
        put('C1', C1in.copy(), np.zeros((M, M)))                                         # plane 0 + zeros: the sum keeps its bits
        C1 = get('C1')
        if mode == 'diag':
            put('Y', *sk_product('y', C1, W))
            put('dsq', np.sum(W * get('Y'), 0), 2 * gamma(M + 2) * np.sum(np.abs(W * get('Y')), 0))   # k_coldot
            put('T', *sk_product('tt', W * s2[None, :], W.T))
            put('U', *sk_product('full', get('T'), C1))
            U = get('U')
            put('V', U + U.T - C1, 2 * gamma(2) * (np.abs(U) + np.abs(U.T) + np.abs(C1)))              # k_uut_minus
            put('R', *sk_product('r', W.T, get('V'), lower_only=True))
            a1gm, du, v = get('a1gm'), get('du'), np.asarray(op['v'], dtype=np.float64)
            R = get('R')
            put('dL', -np.tril(2.0 * R + np.outer(alpha, a1gm) + np.outer(du, v)),
                np.tril(2 * gamma(4) * (2 * np.abs(R) + np.abs(np.outer(alpha, a1gm)) + np.abs(np.outer(du, v)))))   # k_dl_assemble
        else:
            if full:
                put('Y', *sk_product('y', C1, Lq))
                kl = np.tril(Lq) - np.diag(1.0 / np.diag(Lq)) if with_kl else 0.0
                put('dLq', np.tril(2.0 * get('Y')) - kl, gamma(3) * (np.abs(np.tril(2.0 * get('Y'))) + np.abs(kl)))  # k_dlq_assemble
                Rt = op['Rt'] if 'Rt' in op else TmI @ W                               # the image R^T = (T - I) W of the forward stage
                put('R', *sk_product('rfull', Rt.T, C1, lower_only=True))
            else:
                put('dsq', np.diag(C1).copy(), np.zeros(M))                              # k_diag
                put('R', *sk_product('r', ((s2 - 1.0)[:, None] * W).T, C1, lower_only=True))
            a1gm, R = get('a1gm'), get('R')
            put('dL', -np.tril(2.0 * R + np.outer(alpha, a1gm)), np.tril(2 * gamma(3) * (2 * np.abs(R) + np.abs(np.outer(alpha, a1gm)))))
        put('Q', *sk_product('r', L.T, get('dL'), lower_only=True, post=phi))
        put('QW', *sk_product('t', get('Q'), W, lower_only=True))
        put('S', *sk_product('s', W.T, get('QW')))
    elif full:
        kl = np.tril(Lq) - np.diag(1.0 / np.diag(Lq)) if with_kl else np.zeros((M, M))
        put('dLq', -kl, gamma(2) * np.abs(kl))
    G, Gb = np.zeros((M, M)), np.zeros((M, M))
    if with_data:
        S = get('S')
        G, Gb = 0.5 * (S + S.T), gamma(2) * (np.abs(S) + np.abs(S.T))
    if with_kl and mode == 'diag':
        if op.get('P') is None:
            put('P', *sk_product('s', W.T, W))
            P = get('P')
        else:
            P = np.asarray(op['P'], dtype=np.float64)
        put('PSP', *sk_product('full', P, s2[:, None] * P))
        PSP = get('PSP')
        kl = 0.5 * (0.5 * (P + P.T) - np.outer(alpha, alpha) - 0.5 * (PSP + PSP.T))
        G = G - kl
        Gb = Gb + gamma(8) * (np.abs(G) + 0.5 * (np.abs(P) + np.abs(P.T)) + np.abs(np.outer(alpha, alpha)) + 0.5 * (np.abs(PSP) + np.abs(PSP.T)))
    put('G', G, 2 * Gb)                                                                # k_sym_combine
    kg, kb = kuu_grad(get('G'), Kuu, op['jitter'], Z)                                  # k_kuu_grad[_wide]: adds to slab 0, rows < M
    krow = krow0.copy()
    krow[0, :M] += kg
    bnd = np.zeros_like(krow)
    bnd[0, :M] = kb + EPS * np.abs(krow[0, :M])
    put('krow', krow, bnd)
    return r


def dense_pack(krow, du, dsq, s, ell, var, include_kl=True, dkl_du=None, dkl_ds_diag=None):
    """k_dense_pack's gradient blocks of one latent from the reverse stage's results: dZ = sum_slabs krow[:, 1 + d] / ell_d^2,
    du = du - [kl] dKL/du, ds = 2 s dsq - [kl] (-1 / s + c s), dell = sum_m sum_slabs krow[:, 1 + D + d] / ell_d^3, and the Kuf / Kuu part of
    dvar = sum_m sum_slabs krow[:, 0] / var.  dkl_du: alpha (unwhitened) or u (whitened); c = dkl_ds_diag: diag(Kuu^-1) or 1.
    s = None (full covariance): no ds block -- dLq is the reverse stage's own."""
    M = du.shape[0]
    D = (krow.shape[2] - 2) // 2
    k = krow[:, :M].sum(0)
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,))
    out = dict(dZ=k[:, 1:1 + D] / ell ** 2, dell=k[:, 1 + D:1 + 2 * D].sum(0) / ell ** 3, dvar=k[:, 0].sum() / var)
    out['du'] = du - (dkl_du if include_kl else 0.0)
    if s is not None:
        out['ds'] = 2.0 * s * dsq - ((-1.0 / s + dkl_ds_diag * s) if include_kl else 0.0)
    return out


def mxm_int_seed(M, D):
    """The draw of mxm_int_operands the GPU exact tier uses at (M, D); the CPU pin of the exactness premise walks the same draws."""
    return 1000 + M + D


def mxm_int_operands(M, D, seed, mode='diag'):
    """Operands on which the whole reverse stage is EXACT in float64: every tap is a multiple of 1/8 and every product's sum |a||b| stays far
    below 2^50, so each partial sum is exact in any order, with or without fma, and a GPU result must equal the numpy chain bit for bit.
    W, L: unit lower triangular with three further +-1 entries per row at random columns <= i; s^2 in {1, 2} -- passed as s^2's square root
    would not be exact, so s in {1, 2}, s^2 in {1, 4}; C1 = A + A^T with two +-1 entries per row of A; K gm in {-1, 0, 1} spread over
    the four slabs of krow; alpha, v in {-1, 1}; Kuu symmetric and Z with entries in {-2 .. 2}; jitter = 1/2.
    'white_full': Lq lower triangular, diagonal in {1, 2, -1} (1 / Lq_ii exact), two further +-1 entries per row."""
    rs = np.random.RandomState(seed)

    def unit_lower(n_extra):
        A = np.eye(M)
        for i in range(M):
            for j in rs.randint(0, i + 1, n_extra):
                if j < i:
                    A[i, j] = rs.choice([-1.0, 1.0])
        return A

    W, L = unit_lower(3), unit_lower(3)
    A = np.zeros((M, M))
    for i in range(M):
        A[i, rs.randint(0, M, 2)] = rs.choice([-1.0, 1.0], 2)
    Kuu = rs.randint(-2, 3, (M, M)).astype(np.float64)
    Kuu = np.tril(Kuu) + np.tril(Kuu, -1).T
    Mp = round_up(M, BM)
    krow = np.zeros((KG_SPLIT, Mp, 2 + 2 * D))
    krow[rs.randint(0, KG_SPLIT, M), np.arange(M), 1 + 2 * D] = rs.randint(-1, 2, M)
    op = dict(W=W, L=L, Kuu=Kuu, Z=rs.randint(-2, 3, (M, D)).astype(np.float64), C1=A + A.T, krow=krow, jitter=0.5,
              alpha=rs.choice([-1.0, 1.0], M), v=rs.choice([-1.0, 1.0], M), u=rs.choice([-1.0, 1.0], M))
    if mode == 'white_full':
        Lq = np.diag(rs.choice([1.0, 2.0, -1.0], M))
        for i in range(M):
            for j in rs.randint(0, i + 1, 2):
                if j < i:
                    Lq[i, j] = rs.choice([-1.0, 1.0])
        op['s'] = Lq
    else:
        op['s'] = rs.choice([1.0, 2.0], M)
    return op


# ---------------------------------------------------------------------------------------------------------------------------------
# M x M forward stage (latents_forward) behind the factorisation: what it leaves for the chunk loop and the reverse stage
# ---------------------------------------------------------------------------------------------------------------------------------
def mxm_forward(W, L, u, s, white=False, need_grad=True, given=None):
    """One statement per launch, applied to the W and L the factorisation produced.  Unwhitened: v = W u (k_gemv_rows), alpha = W^T v and
    dkinv = column sums of W^2 (k_kl_cols), KL = 1/2 (sum v^2 - M - sum log s^2 + sum dkinv s^2 + sum log L_ii^2) (k_kl_value: four M-term
    sums), Wp = W diag(s^2) (k_colscale), P = W^T W ("s"), Qt = diag(s^2) P - I, Rt = W Qt ("rt"), Wt = W^T.  Whitened: the block wh =
    (s^2 - 1, u, 1) and KL = 1/2 (sum u^2 + sum s^2 - M - sum log s^2) (k_kl_white), alpha = W^T u (k_gemv_cols), Wp = diag(s^2 - 1) W.
    given: the GPU's outputs -- every launch is then checked on the operands its kernel read.  Returns {name: (value, bound)}."""
    M = W.shape[0]
    r = {}

    def get(name):
        return given[name] if given is not None and given.get(name) is not None else r[name][0]

    s2 = s * s
    r['Wt'] = (W.T.copy(), np.zeros((M, M)))
    if white:
        r['wh'] = (np.stack([s2 - 1.0, u, np.ones(M)]), np.stack([EPS * (s2 + 1.0), np.zeros(M), np.zeros(M)]))
        terms = np.array([np.sum(u * u), np.sum(s2), np.sum(np.abs(np.log(s2)))])
        r['kl'] = (0.5 * (np.sum(u * u) - M - np.sum(np.log(s2)) + np.sum(s2)), gamma(M + 4) * (terms.sum() + M))
        if need_grad:
            r['alpha'] = (W.T @ u, 2 * gamma(M + 2) * (np.abs(W.T) @ np.abs(u)))
            r['Wp'] = (get('wh')[0][:, None] * W, 2 * EPS * np.abs(get('wh')[0][:, None] * W))
        return r
    r['v'] = (np.tril(W) @ u, 2 * gamma(M + 2) * (np.abs(np.tril(W)) @ np.abs(u)))
    v = get('v')
    r['alpha'] = (W.T @ v, 2 * gamma(M + 2) * (np.abs(W.T) @ np.abs(v)))
    r['dkinv'] = (np.sum(W * W, 0), 2 * gamma(M + 2) * np.sum(W * W, 0))
    dk, ld = get('dkinv'), np.log(np.diag(L) ** 2)
    terms = np.sum(v * v) + np.sum(np.abs(np.log(s2))) + np.sum(dk * s2) + np.sum(np.abs(ld))
    r['kl'] = (0.5 * (np.sum(v * v) - M - np.sum(np.log(s2)) + np.sum(dk * s2) + np.sum(ld)), gamma(M + 4) * (terms + M))
    if need_grad:
        r['Wp'] = (W * s2[None, :], 2 * EPS * np.abs(W * s2[None, :]))
        r['P'] = sk_product('s', W.T, W)
        P = get('P')
        r['Qt'] = (s2[:, None] * P - np.eye(M), 2 * gamma(2) * (np.abs(s2[:, None] * P) + np.eye(M)))
        r['Rt'] = sk_product('rt', W, get('Qt'))
    return r


def dense_pack_ref(lat_f, lat_g, pw, D, mode='diag', include_kl=True):
    """k_dense_pack's result vector with bounds: {name: (value, bound)} for data, kl, noise, var_f / var_g and per latent tag + dZ, du, ds,
    dell.  lat_*: krow [4][M][2+2D], du, dsq, s (or dLq), kl_vec1, kl_vec2, ell, var, kl; pw [blocks][13].  Sums over the blocks / the M rows
    of the four slabs, each term with the roundings of its formula: gamma_(terms + 8) of the sum of magnitudes."""
    nb = pw.shape[0]
    r = dict(data=(pw[:, 0].sum(), gamma(nb + 2) * np.abs(pw[:, 0]).sum()), noise=(pw[:, 1].sum(), gamma(nb + 2) * np.abs(pw[:, 1]).sum()),
             kl=((lat_f['kl'] + lat_g['kl']) if include_kl else 0.0, EPS * (abs(lat_f['kl']) + abs(lat_g['kl']))))
    for h, (tag, q) in enumerate((('f', lat_f), ('g', lat_g))):
        M = q['du'].shape[0]
        k, ka = q['krow'][:, :M].sum(0), np.abs(q['krow'][:, :M]).sum(0)
        ell = np.broadcast_to(np.asarray(q['ell'], dtype=np.float64), (D,))
        r[tag + 'dZ'] = (k[:, 1:1 + D] / ell ** 2, gamma(8) * ka[:, 1:1 + D] / ell ** 2)
        r[tag + 'dell'] = (k[:, 1 + D:1 + 2 * D].sum(0) / ell ** 3, gamma(M + 8) * ka[:, 1 + D:1 + 2 * D].sum(0) / ell ** 3)
        gv = pw[:, 2 + h]
        r['var_' + tag] = (k[:, 0].sum() / q['var'] + gv.sum(), gamma(M + nb + 8) * (ka[:, 0].sum() / q['var'] + np.abs(gv).sum()))
        r[tag + 'du'] = (q['du'] - (q['kl_vec1'] if include_kl else 0.0), EPS * (np.abs(q['du']) + np.abs(q['kl_vec1'])))
        if mode == 'white_full':
            r[tag + 'ds'] = (q['dLq'], np.zeros_like(q['dLq']))
        else:
            s = q['s']
            klp = (-1.0 / s + q['kl_vec2'] * s) if include_kl else np.zeros(M)
            r[tag + 'ds'] = (2.0 * s * q['dsq'] - klp, gamma(6) * (np.abs(2.0 * s * q['dsq']) + (np.abs(1.0 / s) + np.abs(q['kl_vec2'] * s) if include_kl else 0.0)))
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# Kronecker path (csrc/zigp_kron.hip): the point-wise launches k_kron_pointwise / k_kron_head_pointwise and the panel path's per-point
# kernels k_kron_kbuild, k_kron_colsum, k_kron_da, k_kron_kgrad (tests/test_gpu_kron_stages.py)
# ---------------------------------------------------------------------------------------------------------------------------------
KPW_THREADS, KPW_ACC = 256, 5
TINY = 2.0 ** -960          # floor of every head scale: a result that underflows (exp(-z^2 / 2) at |z| ~ 38 ... 40) is not held to relative accuracy
_MP_CACHE = {}


def pointwise_mp_cached(fm, fv, gm, gv, y, noise):
    """pointwise_mp, remembered per set of evaluation points: the dense and the Kronecker grid tests evaluate at the same doubles."""
    key = tuple(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (fm, fv, gm, gv, y)) + (float(noise),)
    if key not in _MP_CACHE:
        _MP_CACHE[key] = pointwise_mp(fm, fv, gm, gv, y, noise)
    return _MP_CACHE[key]


def kron_pw_inputs(part, knn, offset):
    """(mean, var) as the Kronecker point-wise kernels form them from part [4][Nc] = q0, q1, mean, st: mean + offset and
    knn - q0 q1 + st (scripts/onoff.py:209-211).  The kernel may contract knn - q0 q1 into one fma: callers that need bit-equality use
    operands for which every association is exact."""
    return part[2] + offset, knn - part[0] * part[1] + part[3]


HEAD_OUTPUTS = ('ve', 'dfm', 'dfv', 'dnoise', 'pm', 'pv')


def head_np(lik, fm, fv, y, noise):
    """float64 numpy statement of the single-latent heads (k_kron_head_pointwise), operation by operation.
    'gaussian' (scripts/svgp.py:198-200): ve = -1/2 log 2 pi - 1/2 log s2 - 1/2 ((y - fm)^2 + fv) / s2; predictive density of y: (fm, fv + s2).
    'bernoulli' (scripts/classifier.py:139-140, 210-217): p = c0 + c1 Phi(fm / sqrt(1 + fv)), ve = log(p if y == 1 else 1 - p); (p, p - p^2)."""
    from scipy.special import erf
    fm, fv, y = (np.asarray(a, dtype=np.float64) for a in (fm, fv, y))
    if lik == 'gaussian':
        inv, res = 1.0 / noise, y - fm
        q = res * res + fv
        return dict(ve=-0.5 * LOG2PI - 0.5 * np.log(noise) - 0.5 * q * inv, dfm=res * inv, dfv=-0.5 * inv * np.ones_like(fm),
                    dnoise=-0.5 * inv + 0.5 * q * inv * inv, pm=fm.copy(), pv=fv + noise)
    r = 1.0 / np.sqrt(1.0 + fv)
    z = fm * r
    pr = 0.5 * (1.0 + erf(z * 0.70710678118654752440)) * C1 + C0
    on = y == 1.0
    w = np.where(on, pr, 1.0 - pr)
    dp = np.where(on, 1.0, -1.0) / w
    dz = dp * C1 * 0.39894228040143267794 * np.exp(-0.5 * z * z)
    return dict(ve=np.log(w), dfm=dz * r, dfv=dz * (-0.5 * z / (1.0 + fv)), dnoise=np.zeros_like(fm), pm=pr, pv=pr - pr * pr)


def head_mp(lik, fm, fv, y, noise, dps=50):
    """The same formulas at 50 digits (mpmath), point by point, the clip p = c0 + c1 Phi(z) included; y == 1 exactly is 'on', anything
    else 'off'.  Phi through mpmath's ncdf, which keeps its relative accuracy in the lower tail.  Returns dict of object arrays of mpf."""
    import mpmath as mp
    mp.mp.dps = dps
    n = len(fm)
    out = {k: np.empty(n, dtype=object) for k in HEAD_OUTPUTS}
    c1, c0, one, half, two = mp.mpf(1) - mp.mpf('2e-3'), mp.mpf('1e-3'), mp.mpf(1), mp.mpf('0.5'), mp.mpf(2)
    s2 = mp.mpf(float(noise))
    for i in range(n):
        f_, v_, y_ = (mp.mpf(float(x[i])) for x in (fm, fv, y))
        if lik == 'gaussian':
            res = y_ - f_
            q = res * res + v_
            vals = (-half * mp.log(two * mp.pi) - half * mp.log(s2) - half * q / s2, res / s2, -half / s2, -half / s2 + half * q / (s2 * s2), f_, v_ + s2)
        else:
            z = f_ / mp.sqrt(one + v_)
            pr = c0 + c1 * mp.ncdf(z)
            on = y_ == one
            w = pr if on else one - pr
            dz = (one if on else -one) / w * c1 * mp.npdf(z)
            vals = (mp.log(w), dz / mp.sqrt(one + v_), dz * (-half * z / (one + v_)), mp.mpf(0), pr, pr - pr * pr)
        for k, val in zip(HEAD_OUTPUTS, vals):
            out[k][i] = val
    return out


def head_scales(lik, fm, fv, y, noise):
    """S per output: the sum of the magnitudes it is formed from (as pointwise_scales), floored at TINY.
    Gaussian, q = (y - fm)^2 + fv: ve: 1 + 1/2 |log s2| + 2 q / s2; dnoise: 1/2 / s2 + q / s2^2; dfm, dfv, pm, pv: the value's magnitude.
    Bernoulli, z = fm / sqrt(1 + fv), S_w = 1 + phi(z) |z| (Phi is an O(1) quantity formed with absolute error; the argument's own
    rounding moves it by phi |z| eps), w = p or 1 - p as y selects: ve = log w: |ve| + S_w / w; pm: S_w; pv = p - p^2: p + p^2 +
    S_w |1 - 2 p|; dfm, dfv = +-c1 phi(z) / w times O(1) factors: |value| (4 + z^2 + S_w / w) -- the roundings of the factors, the z^2 of
    exp(-z^2 / 2)'s argument, and w's relative error."""
    r = head_np(lik, fm, fv, y, noise)
    fm, fv, y = (np.asarray(a, dtype=np.float64) for a in (fm, fv, y))
    if lik == 'gaussian':
        q = (y - fm) ** 2 + fv
        S = dict(ve=1.0 + 0.5 * abs(np.log(noise)) + 2.0 * q / noise, dnoise=0.5 / noise + q / noise ** 2, dfm=np.abs(r['dfm']), dfv=np.abs(r['dfv']),
                 pm=np.abs(fm), pv=np.abs(r['pv']))
    else:
        z = fm / np.sqrt(1.0 + fv)
        Sw = 1.0 + np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) * np.abs(z)
        pr = r['pm']
        w = np.where(y == 1.0, pr, 1.0 - pr)
        f = 4.0 + z * z + Sw / w
        S = dict(ve=np.abs(r['ve']) + Sw / w, pm=Sw, pv=pr + pr * pr + Sw * np.abs(1.0 - 2.0 * pr), dfm=np.abs(r['dfm']) * f, dfv=np.abs(r['dfv']) * f,
                 dnoise=np.zeros_like(fm))
    return {k: np.maximum(v, TINY) for k, v in S.items()}


def kron_kbuild(X, col0, Z, ell, var, Nc, dtype=np.float64):
    """k_kron_kbuild: K (M, Nc) = var exp(-1/2 |(z_m - x_n[col0 : col0 + D]) / ell|^2); the padding columns n >= N are the kernel at
    x = 0.  Returns (K, y) with y = -log(K / var), the exponent the kuf tolerance is stated in."""
    f = lambda a: np.asarray(a, dtype=dtype)
    M, D = Z.shape
    xs = np.zeros((Nc, D), dtype=dtype)
    xs[:X.shape[0]] = f(X)[:, col0:col0 + D]
    d = (f(Z)[:, None, :] - xs[None, :, :]) / f(ell)
    y = dtype(0.5) * (d * d).sum(-1)
    return dtype(var) * np.exp(-y), y


def kron_colsum(K0, A0, K1, A1, B1, A0sq, C1, dtype=np.float64):
    """k_kron_colsum: part [4][Nc] = sum_i K0 A0, sum_j K1 A1, sum_i K0 B1, sum_i A0sq C1.  Bound of the GPU side alone (the caller adds the
    reference's own: the same again for float64, 2^-11 of it for longdouble): sums of M products, gamma_(M+2) sum |a b|."""
    f = lambda a: np.asarray(a, dtype=dtype)
    K0, A0, K1, A1, B1, A0sq, C1 = (f(a) for a in (K0, A0, K1, A1, B1, A0sq, C1))
    prods = (K0 * A0, K1 * A1, K0 * B1, A0sq * C1)
    out = np.stack([p.sum(0) for p in prods])
    bnd = np.stack([gamma(p.shape[0] + 2) * np.abs(p).sum(0) for p in prods])
    return out, np.asarray(bnd, dtype=np.float64)


def kron_da(A, C, K, gv, dq, dtype=np.float64):
    """k_kron_da: dA = 2 A gv C, E = dq K + dA.  Bounds: three roundings, gamma_3 |dA|; E one product and one sum more: gamma_4 (|dq K| + |dA|)."""
    f = lambda a: np.asarray(a, dtype=dtype)
    A, C, K, gv, dq = f(A), f(C), f(K), f(gv)[None, :], f(dq)[None, :]
    dA = 2 * A * gv * C
    E = dq * K + dA
    return (dA, np.asarray(gamma(3) * np.abs(dA), dtype=np.float64)), (E, np.asarray(gamma(4) * (np.abs(dq * K) + np.abs(dA)), dtype=np.float64))


def kron_kgrad(B, A, PdA, K, gm, dq, X, col0, Z, krow0=None, dtype=np.float64):
    """k_kron_kgrad: dK = gm B + 2 dq A + PdA; krow[m] += [sum dK K, sum dK K (x_d - z_md), sum dK K (x_d - z_md)^2] over the N = len(X) valid
    columns (x: the columns col0 : col0 + D of X); the last column of krow is not touched.  Returns (krow (M, 2 + 2D), bound).
    Bound of the GPU side alone, as kgrad's: with T_mn = (|gm B| + 2 |dq A| + |PdA|) |K|, gamma_(N+9) (sum_n T |x - z|^p + |krow0|): the
    sum of N terms, 8 spare roundings for dK (4), its product with K, x - z and the moment factors, one for the accumulation."""
    f = lambda a: np.asarray(a, dtype=dtype)
    M, D = Z.shape
    N = X.shape[0]
    B, A, PdA, K, gm, dq, Xc, Zc = f(B)[:, :N], f(A)[:, :N], f(PdA)[:, :N], f(K)[:, :N], f(gm)[None, :N], f(dq)[None, :N], f(X)[:, col0:col0 + D], f(Z)
    t = (gm * B + 2 * dq * A + PdA) * K
    T = (np.abs(gm * B) + 2 * np.abs(dq * A) + np.abs(PdA)) * np.abs(K)
    out = np.zeros((M, 2 + 2 * D), dtype=dtype) if krow0 is None else f(krow0).copy()
    bnd = np.abs(out)
    bnd[:, 1 + 2 * D] = 0
    out[:, 0] += t.sum(1)
    bnd[:, 0] += T.sum(1)
    for d in range(D):
        df = Xc[None, :, d] - Zc[:, None, d]
        out[:, 1 + d] += (t * df).sum(1)
        out[:, 1 + D + d] += (t * df * df).sum(1)
        bnd[:, 1 + d] += (T * np.abs(df)).sum(1)
        bnd[:, 1 + D + d] += (T * df * df).sum(1)
    return out, np.asarray(gamma(N + 9) * bnd, dtype=np.float64)


def kron_dyadic_case(seed=0, Nc=1024):
    """Operands of the Kronecker point-wise launch for which the evaluation point is EXACT: q0, q1, mean, st, the factor variances (and so
    Knn = var0 var1) and the offsets are multiples of 2^-10 of magnitude <= 2^6, so q0 q1 is a multiple of 2^-20 below 2^12 and
    Knn - q0 q1 + st, mean + offset need at most 33 bits in every association, with or without fma
    (tests/test_cpu_stage_ref.py walks the associations in exact rationals).  Points 0 and 1 cancel terms of size 32 (latent f; 10 for
    latent g) down to 2^-20.  Elsewhere the variance stays above 1."""
    rs = np.random.RandomState(4000 + seed)
    u = 2.0 ** -10
    var_f, var_g = (8.0, 4.0), (2.0, 5.0)

    def planes(a, b):          # cancelling points: (a + u)(b - u) = a b + (b - a) u - u^2, st = (b - a) u  ->  Knn - q0 q1 + st = u^2
        q0, q1 = rs.randint(0, 3 * 1024, Nc) * u, rs.randint(0, 3 * 1024, Nc) * u
        mean, st = rs.randint(-4 * 1024, 4 * 1024 + 1, Nc) * u, rs.randint(0, 8 * 1024, Nc) * u
        q0[0], q1[0], st[0] = a + u, b - u, (b - a) * u
        q0[1], q1[1], st[1] = -(a + u), -(b - u), (b - a) * u
        return np.stack([q0, q1, mean, st])

    return dict(part_f=planes(4.0, 8.0), part_g=planes(2.0, 5.0), var_f=var_f, var_g=var_g, f_offset=0.25, g_offset=-1.0, scale=2.5, noise=0.0625)


def kron_panel_operands(kind, M, D, N, Nc, seed, M1=None, col0=2):
    """Operands of the panel kernels.  kind 'int': integers in {-3 .. 3} -- every product and every sum of the four kernels is then an
    integer far below 2^53 (the largest: 1000 terms of |dK K (x - z)^2| <= 30 * 3 * 36), so any order of evaluation, with or without fma,
    gives the same double; 'normal': standard normal panels, K in (0, 1), inputs in (0, 1).  X is (N, ldx) with ldx = col0 + D + 1: the
    factor reads the columns col0 : col0 + D."""
    rs = np.random.RandomState(7000 + seed)
    M1 = M if M1 is None else M1
    ldx = col0 + D + 1
    if kind == 'int':
        draw = lambda *s: rs.randint(-3, 4, s).astype(np.float64)
        pos = draw
    else:
        draw, pos = (lambda *s: rs.randn(*s)), (lambda *s: rs.rand(*s))
    return dict(B=draw(M, Nc), A=draw(M, Nc), PdA=draw(M, Nc), K=pos(M, Nc), C=draw(M, Nc), Asq=pos(M, Nc), K1=pos(M1, Nc), A1=draw(M1, Nc),
                gm=draw(Nc), gv=draw(Nc), dq=draw(Nc), X=pos(N, ldx), Z=pos(M, D), krow0=draw(M, 2 + 2 * D), col0=col0)
