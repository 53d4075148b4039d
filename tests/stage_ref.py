"""Host references of the dense chunk loop's stages, one plain numpy statement per stage, each with the rounding bound its GPU twin is
held to (tests/test_gpu_stages.py).  Written from the formulas in the kernel comments (csrc/zigp_dense.hip header, csrc/zigp_gemm.h epilogues,
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
