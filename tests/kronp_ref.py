"""The Kronecker model in the FACTORED algebra of the GEMM-panel path (csrc/zigp_kron.hip), restated on the CPU -- TEST INFRASTRUCTURE ONLY.

The literal oracle (oracle/zigp_oracle_torch.py, tests/kron_matern_ref.py) forms the dense (M0 M1) x (M0 M1) Kronecker inverse and the dense
(M0 M1) x N cross-covariance: at 130 x 129 inducing points that is a 16 770 x 16 770 matrix and is not evaluated.  This file states the same
model per latent from the factor matrices alone, with P_p = K_p^-1, U = reshape(u), S2 = reshape(s^2), Alpha = P0 U P1, k_p = k_p(Z_p, X_p),
a_p = P_p k_p:

    mean_n = sum_i k0[i,n] (Alpha k1)[i,n]
    var_n  = v0 v1 - (k0 . a0)_n (k1 . a1)_n + sum_i a0[i,n]^2 (S2 a1^2)[i,n]
    KL     = 1/2 [ sum U . Alpha - M0 M1 - sum log s^2 + sum_ij diag(P0)_i diag(P1)_j s_ij^2 + M1 logdet K0 + M0 logdet K1 ]

in torch float64 (the inverse: torch.linalg.inv, as the literal oracle; the log-determinants: the Cholesky diagonal), the point-wise
likelihood terms are the oracle's own functions, gradients come from autograd.  Factor kinds as kron_matern_ref reads them.
tests/test_cpu_kron_blocks.py pins value, KL and every gradient block of this restatement to the literal oracle at 1e-8 on the grids where
both can be evaluated; on a grid where only this one can, it is the reference of tests/test_gpu_kron_blocks.py."""
import numpy as np
import torch

import kron_matern_ref as kmr
from zigp_oracle_torch import DT, _t, probit_expectations, variational_expectations, KRON_KEYS, KRON_VEC_KEYS


def factored_latent(Xt, Z, ell, var, q_mu, q_sqrt, jitter, kinds=kmr.RBF2, with_kl=True):
    """(mean [N,1], var [N,1], KL) of one latent by the factored identities above"""
    M0, M1, d0 = Z[0].shape[0], Z[1].shape[0], Z[0].shape[1]
    Kmm = kmr.factor_Kmm(kinds, Z, ell, var, jitter)
    P = [torch.linalg.inv(K) for K in Kmm]
    k0 = kmr.factor_K(kinds[0], Z[0], Xt[:, :d0], ell[0], var[0])
    k1 = kmr.factor_K(kinds[1], Z[1], Xt[:, d0:], ell[1], var[1])
    U, S2 = q_mu.reshape(M0, M1), torch.square(q_sqrt).reshape(M0, M1)
    a0, a1 = P[0] @ k0, P[1] @ k1
    Al = P[0] @ U @ P[1]
    mu = torch.sum(k0 * (Al @ k1), 0)
    vv = var[0] * var[1] - torch.sum(k0 * a0, 0) * torch.sum(k1 * a1, 0) + torch.sum(torch.square(a0) * (S2 @ torch.square(a1)), 0)
    kl = torch.zeros((), dtype=DT)
    if with_kl:
        ld = [torch.sum(torch.log(torch.square(torch.diagonal(torch.linalg.cholesky(K))))) for K in Kmm]
        kl = 0.5 * (torch.sum(U * Al) - float(M0 * M1) - torch.sum(torch.log(S2))
                    + torch.sum(torch.diagonal(P[0])[:, None] * torch.diagonal(P[1])[None, :] * S2) + M1 * ld[0] + M0 * ld[1])
    return mu.reshape(-1, 1), vv.reshape(-1, 1), kl


def factored_elbo_and_grad(X, Y, p_np, jitter, scale=1.0, g_offset=0.0, include_kl=True, need_grad=True):
    """(elbo, data, kl, grads) as zigp_oracle_torch.kron_elbo_and_grad returns them, from the factored identities"""
    kf, kg = kmr.kinds_of(p_np)
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    p = {}
    for k in KRON_KEYS:
        p[k] = [_t(v).clone().requires_grad_(need_grad) for v in p_np[k]]
    for k in KRON_VEC_KEYS:
        p[k] = _t(p_np[k]).clone().requires_grad_(need_grad)
    with torch.set_grad_enabled(need_grad):
        fmean, fvar, klf = factored_latent(Xt, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter, kf, include_kl)
        gmean, gvar, klg = factored_latent(Xt, p['Zg'], p['ell_g'], p['var_g'], p['u_gm'], p['u_gs_sqrt'], jitter, kg, include_kl)
        gmean = gmean + g_offset
        e1, e2, ev = probit_expectations(gmean, gvar)
        data = torch.sum(variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), Yt, p['noise']))
        kl = klf + klg
        elbo = data * scale - kl
    grads = None
    if need_grad:
        elbo.backward()
        grads = {}
        for k in KRON_KEYS:
            grads[k] = [v.grad.numpy().copy() for v in p[k]]
        for k in KRON_VEC_KEYS:
            grads[k] = p[k].grad.numpy().copy()
    return float(elbo.detach()), float(data.detach()), float(kl.detach()), grads


def factored_predict(X, p_np, jitter, g_offset=0.0):
    """the 9 rows of build_predict (scripts/onoff.py:161-184) as a (9, N) array, from the factored identities"""
    kf, kg = kmr.kinds_of(p_np)
    with torch.no_grad():
        Xt = _t(X)
        lists = lambda tag: [[_t(v) for v in p_np[k + tag]] for k in ('Z', 'ell_', 'var_')]
        fmean, fvar, _ = factored_latent(Xt, *lists('f'), _t(p_np['u_fm']), _t(p_np['u_fs_sqrt']), jitter, kf, False)
        gmean, gvar, _ = factored_latent(Xt, *lists('g'), _t(p_np['u_gm']), _t(p_np['u_gs_sqrt']), jitter, kg, False)
        gmean = gmean + g_offset
        e1, e2, ev = probit_expectations(gmean, gvar)
        rows = (e1 * fmean, e2 * fvar, ev * torch.square(fmean), fmean, fvar, gmean, gvar, e1, ev)
        return np.stack([r.reshape(-1).numpy() for r in rows])


# ---------------------------------------------------------------------------------------------------------------------------------
# The M x M launches of one panel step (kron_run_panels), each restated from the TAPPED inputs of that launch (DenseEngine.test_kron_panel_step,
# include/zigp_diag.h zigp_kronp_tap_latent) in NumPy -- dtype numpy.float64 or numpy.longdouble.  Every image is the padded one the kernels
# work on: [Mq][Mq] per factor, [Mq0][Mq1] per grid, Mq_p = M_p rounded up to 128; K_p and P_p carry the identity in their padding, the grids
# zeros.  Each entry of the result is (value, S), S the sum of the absolute values of the terms of that launch alone (its tapped operands
# enter with their magnitudes): the bound tier of tests/test_gpu_kron_panel_stages.py holds err_gpu <= 4 err_np + 16 eps S.
# _mut: the deliberate mistakes of tests/test_cpu_kronp_ref.py (MUTATIONS below).
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('pbranch',       # k_kron_dp_combine: the p branch of the diagonal term swapped (s2[o lds2 + i] for p = 0)
             'lds2',          # ... its row stride taken as Mq0
             'vecoff',        # ... diag(P_other) read at the other offset of vec
             'vecoff_us',     # k_kron_us / k_kron_kl: d1 = vec instead of vec + Mq0
             'dropplane',     # k_sum_planes: the last split-K plane left out
             'ldT',           # a transposed operand (U in Q1 = U^T T1, T1 in dP1 += T1^T dAl) read with leading dimension Mq0
             'Qhalf',         # 0.25 -> 0.5 on Q
             'Mother',        # k_kron_dk: M_other taken from the factor itself
             'logdet_late')   # k_kron_kl reading L after the backward pass has put P dP P there
MUT_NEEDS_S_BELOW_NK = 'Snk'  # S forced to nk: differs from the rule only where nk > 512 / (nba nbb) -- b3's dP0 (tests: facts and plane count)


def _f(a, dtype):
    return np.asarray(a, dtype=dtype)


def _mm(A, B, with_S=True):
    return A @ B, (np.abs(A) @ np.abs(B) if with_S else None)


def split_k_slices(nk, nba, nbb):
    """nred's rule: the number of split-K slices of a reduction with nba x nbb output tiles over nk k-blocks of 16 columns"""
    return max(1, min(nk, 512 // max(1, nba * nbb)))


def sum_planes(planes, _mut=()):
    """k_sum_planes: the planes added in plane order, one rounding per addition -- in float64 this is the kernel's own arithmetic"""
    planes = np.asarray(planes)
    out = np.zeros(planes.shape[1:], dtype=planes.dtype)
    for s in range(planes.shape[0] - (1 if 'dropplane' in _mut else 0)):
        out = out + planes[s]
    return out


def _wrong_ld(A, ld):
    """the [Mq0][Mq1] image A read as if its rows were ld apart (indices past the image wrap: any value there is as wrong)"""
    r, c = A.shape
    idx = (np.arange(r)[:, None] * ld + np.arange(c)[None, :]) % A.size
    return A.reshape(-1)[idx]


def dp_combine(dP, Q, S2, vec, p, M, Mq, kl, dtype, _mut=()):
    """k_kron_dp_combine for factor p: sym(dP) - kl (1/4 (Q + Q^T) + 1/2 diag w), w_i = sum_o diag(P_other)_o s2[i, o] (p = 0) or s2[o, i] (p = 1)
    over the other factor's M_other real points, s2 read from the flat [Mq0][Mq1] image with row stride Mq1, diag(P_other) from vec at
    offset Mq0 (p = 0) or 0 (p = 1)"""
    dP, vec, flat = _f(dP, dtype), _f(vec, dtype), _f(S2, dtype).reshape(-1)
    v, S = (dP + dP.T) / 2, (np.abs(dP) + np.abs(dP).T) / 2
    if kl:
        Q = _f(Q, dtype)
        qc = dtype(0.5 if 'Qhalf' in _mut else 0.25)
        v, S = v - qc * (Q + Q.T), S + qc * (np.abs(Q) + np.abs(Q).T)
        off = Mq[0] if p == 0 else 0
        if 'vecoff' in _mut:
            off = Mq[0] - off
        lds2 = Mq[0] if 'lds2' in _mut else Mq[1]
        Mo = M[1 - p]
        dother = vec[(off + np.arange(Mo)) % vec.size]      # (a wrong offset can run past vec: the index wraps, any value there is as wrong)
        i, o = np.arange(Mq[p])[:, None], np.arange(Mo)[None, :]
        row_major = (p == 0) != ('pbranch' in _mut)
        idx = (i * lds2 + o) if row_major else (o * lds2 + i)
        s2 = flat[idx % flat.size]
        w, aw = (s2 * dother[None, :]).sum(1), (np.abs(s2) * np.abs(dother)[None, :]).sum(1)
        v, S = v - np.diag(w) / 2, S + np.diag(aw) / 2
    return v, S


def kuu_rows(G, K, Z, jitter, dtype):
    """k_kuu_grad on the real [M][M] part: (M, 2 + 2 D) additions to krow -- column 0 sum_j G Kz, 1 + d: sum_j 2 G Kz (z_jd - z_md),
    1 + D + d: sum_j G Kz (z_jd - z_md)^2, last column untouched; Kz = K - jitter I"""
    Z = _f(Z, dtype)
    M, D = Z.shape
    G, K = _f(G, dtype)[:M, :M], _f(K, dtype)[:M, :M]
    kz, akz = K - dtype(jitter) * np.eye(M, dtype=dtype), np.abs(K) + dtype(jitter) * np.eye(M, dtype=dtype)
    t, at = G * kz, np.abs(G) * akz
    out, S = np.zeros((M, 2 + 2 * D), dtype=dtype), np.zeros((M, 2 + 2 * D), dtype=dtype)
    out[:, 0], S[:, 0] = t.sum(1), at.sum(1)
    for d in range(D):
        df = Z[None, :, d] - Z[:, None, d]
        out[:, 1 + d], S[:, 1 + d] = (2 * t * df).sum(1), (2 * at * np.abs(df)).sum(1)
        out[:, 1 + D + d], S[:, 1 + D + d] = (t * df * df).sum(1), (at * df * df).sum(1)
    return out, S


def restate(t, M, Z, s, jitter, kl, planes_of='dAl', dtype=np.float64, _mut=(), with_S=True):
    """Every M x M launch of one latent of a panel step from the taps t of DenseEngine.test_kron_panel_step (or of simulate()): name -> (value, S).
    M = (M0, M1), Z = [Z0, Z1], s: q_sqrt as (M0, M1), kl: include_kl.  Names: P0, P1, T0, Al, vec, klv (kl), red (the plane sum of the
    reduction planes_of), T1_a, dU, T1_b, dP_acc0/1, Q0/1 (kl), dP_comb0/1, T0_/T1_ (= dP P), PdPP0/1, G0/1, krow0/1, gu, gs.
    with_S=False: the matrix products come back with S = None (the long-double pass of the GPU test needs the values only)."""
    ab = (lambda A, B: np.abs(A) @ np.abs(B)) if with_S else (lambda A, B: None)
    mm = lambda A, B: _mm(A, B, with_S)
    Mq = tuple(-(-m // 128) * 128 for m in M)
    g = lambda k, q=None: _f(t[k] if q is None else t[k][q], dtype)
    out = {}
    P = [g('P', 0), g('P', 1)]
    for q in range(2):
        W = g('W', q)
        out['P%d' % q] = (W.T @ W, ab(W.T, W))
    U, S2, T0, Al, dAl, dS2, vec = (g(k) for k in ('U', 'S2', 'T0', 'Al', 'dAl', 'dS2', 'vec'))
    out['T0'] = mm(U, P[1])
    out['Al'] = mm(P[0], T0)
    out['vec'] = (np.concatenate([np.diag(P[0]), np.diag(P[1])]), np.concatenate([np.abs(np.diag(P[0])), np.abs(np.diag(P[1]))]))
    s = _f(s, dtype)
    d0 = vec[:M[0]]
    d1 = vec[:M[1]] if 'vecoff_us' in _mut else vec[Mq[0]:Mq[0] + M[1]]
    if kl:
        import kronf_ref
        k3 = kronf_ref.kl_scalars(U[:M[0], :M[1]], Al[:M[0], :M[1]], s, d0, d1, dtype)
        ld = []
        for q in range(2):
            l = np.diag(g('PdPP' if 'logdet_late' in _mut else 'L', q))[:M[q]]
            ll = np.log(l * l)
            ld.append((ll.sum(), (np.abs(ll) + 2).sum()))
        vals = [k3['uAl'], k3['logs2'], k3['ds2'], ld[0], ld[1]]
        out['klv'] = (np.array([v for v, _ in vals], dtype=dtype), np.array([S for _, S in vals], dtype=dtype))
    if 'planes' in t:
        r = sum_planes(_f(t['planes'], dtype), _mut)
        out['red'] = (r, np.abs(_f(t['planes'], dtype)).sum(0))
    out['T1_a'] = mm(dAl, P[1])
    out['dU'] = mm(P[0], g('T1_a'))
    out['T1_b'] = mm(P[0], U)
    T1b = g('T1_b')
    T1b_T = _wrong_ld(T1b, Mq[0]) if 'ldT' in _mut else T1b
    U_T = _wrong_ld(U, Mq[0]) if 'ldT' in _mut else U
    r0, r1 = g('dP_red', 0), g('dP_red', 1)
    out['dP_acc0'] = (r0 + dAl @ T0.T, np.abs(r0) + ab(dAl, T0.T) if with_S else None)
    out['dP_acc1'] = (r1 + T1b_T.T @ dAl, np.abs(r1) + ab(T1b_T.T, dAl) if with_S else None)
    if kl:
        out['Q0'] = mm(T0, U.T)
        out['Q1'] = (U_T.T @ T1b, ab(U_T.T, T1b))
    for q in range(2):
        out['dP_comb%d' % q] = dp_combine(g('dP_acc', q), t['Q'][q] if kl else None, S2, vec, q, M, Mq, kl, dtype, _mut)
        out['T%d_' % q] = mm(g('dP_comb', q), P[q])
        out['PdPP%d' % q] = mm(P[q], g('T', q))
        coef = dtype((M[q] if 'Mother' in _mut else M[1 - q]) / 2.0 if kl else 0.0)
        PXP = g('PdPP', q)
        out['G%d' % q] = (-PXP - coef * P[q], np.abs(PXP) + coef * np.abs(P[q]))
        kr, aS = kuu_rows(g('G', q), g('K', q), Z[q], jitter, dtype)
        kn = g('krow_n', q)
        full, fS = kn.copy(), np.abs(kn)
        full[:M[q]] += kr
        fS[:M[q]] += aS
        out['krow%d' % q] = (full, fS)
    klf = dtype(1 if kl else 0)
    dUr, dS2r, Alr = g('dU')[:M[0], :M[1]], dS2[:M[0], :M[1]], Al[:M[0], :M[1]]
    dd = d0[:, None] * d1[None, :] * s
    out['gu'] = (dUr - klf * Alr, np.abs(dUr) + klf * np.abs(Alr))
    out['gs'] = (2 * s * dS2r - klf * (-1 / s + dd), 2 * np.abs(s * dS2r) + klf * (1 / np.abs(s) + np.abs(dd)))
    return out


TAP_OF = dict(P0=('P', 0), P1=('P', 1), T0='T0', Al='Al', vec='vec', klv='klv', T1_a='T1_a', dU='dU', T1_b='T1_b', dP_acc0=('dP_acc', 0),
              dP_acc1=('dP_acc', 1), Q0=('Q', 0), Q1=('Q', 1), dP_comb0=('dP_comb', 0), dP_comb1=('dP_comb', 1), T0_=('T', 0), T1_=('T', 1),
              PdPP0=('PdPP', 0), PdPP1=('PdPP', 1), G0=('G', 0), G1=('G', 1), krow0=('krow', 0), krow1=('krow', 1), gu='gu', gs='gs')


def tap_of(t, name, planes_of='dAl'):
    """the tap a restate() entry stands for"""
    if name == 'red':
        return t['dP_red'][int(planes_of[2])] if planes_of.startswith('dP') else t[planes_of]
    k = TAP_OF[name]
    return t[k] if isinstance(k, str) else t[k[0]][k[1]]


def simulate(X, p, tag, cot, jitter, kl, planes=8, dtype=np.float64):
    """The taps of one latent of a panel step computed on the CPU in `dtype` (RBF factors): what restate() is handed when no GPU is there.
    cot = [4][N] (gm, gv, dq0, dq1).  The split-K planes of dAl are `planes` column ranges of the points.  Every launch's output is the value
    of its restate() entry evaluated on the outputs before it, so restate(simulate(...)) reproduces the taps."""
    import zigp_oracle as o
    Z, ell, var = p['Z' + tag], p['ell_' + tag], [float(np.squeeze(v)) for v in p['var_' + tag]]
    M = (Z[0].shape[0], Z[1].shape[0])
    Mq = tuple(-(-m // 128) * 128 for m in M)
    D0 = Z[0].shape[1]
    N = X.shape[0]
    gm, gv, dq0, dq1 = (_f(c, dtype) for c in cot)

    def pad(A, shape, eye=False):
        out = np.eye(shape[0], dtype=dtype) if eye else np.zeros(shape, dtype=dtype)
        out[:A.shape[0], :A.shape[1]] = A
        return out

    t = {k: [None, None] for k in ('K', 'L', 'W', 'P', 'krow_n', 'dP_red', 'dP_acc', 'Q', 'dP_comb', 'T', 'PdPP', 'G', 'krow')}
    Kp = []
    for q in range(2):
        K = _f(o.rbf_K(Z[q], None, ell[q], var[q]), dtype) + dtype(jitter) * np.eye(M[q], dtype=dtype)
        L = np.linalg.cholesky(K.astype(np.float64)).astype(dtype)
        W = np.linalg.inv(L.astype(np.float64)).astype(dtype)
        t['K'][q], t['L'][q], t['W'][q] = pad(K, (Mq[q], Mq[q]), True), pad(L, (Mq[q], Mq[q]), True), pad(W, (Mq[q], Mq[q]), True)
        t['P'][q] = t['W'][q].T @ t['W'][q]
        cols = X[:, :D0] if q == 0 else X[:, D0:]
        Kp.append(pad(_f(o.rbf_K(Z[q], cols, ell[q], var[q]), dtype), (Mq[q], N)))
    P = t['P']
    s = _f(p['u_%ss_sqrt' % tag], dtype).reshape(M)
    t['U'], t['S2'] = pad(_f(p['u_%sm' % tag], dtype).reshape(M), Mq), pad(s * s, Mq)
    t['T0'] = t['U'] @ P[1]
    t['Al'] = P[0] @ t['T0']
    t['vec'] = np.concatenate([np.diag(P[0]), np.diag(P[1])])
    A = [P[q] @ Kp[q] for q in range(2)]
    Asq = [a * a for a in A]
    Bx = [t['Al'] @ Kp[1], t['Al'].T @ Kp[0]]
    Cx = [t['S2'] @ Asq[1], t['S2'].T @ Asq[0]]
    for q, dq in enumerate((dq0, dq1)):
        dA = 2 * A[q] * gv[None, :] * Cx[q]
        E = dq[None, :] * Kp[q] + dA
        PdA = P[q] @ dA
        dK = gm[None, :] * Bx[q] + 2 * dq[None, :] * A[q] + PdA
        tk = dK * Kp[q]
        Dq = Z[q].shape[1]
        cols = _f(X[:, :D0] if q == 0 else X[:, D0:], dtype)
        kr = np.zeros((Mq[q], 2 + 2 * Dq), dtype=dtype)
        kr[:, 0] = tk.sum(1)
        for d in range(Dq):
            df = cols[None, :, d] - pad(_f(Z[q], dtype), (Mq[q], Dq))[:, d:d + 1]
            kr[:, 1 + d], kr[:, 1 + Dq + d] = (tk * df).sum(1), (tk * df * df).sum(1)
        kr[M[q]:] = 0
        t['krow_n'][q] = kr
        t['dP_red'][q] = E @ Kp[q].T
    cuts = [N * i // planes for i in range(planes + 1)]
    t['planes'] = np.stack([(Kp[0][:, a:b] * gm[None, a:b]) @ Kp[1][:, a:b].T for a, b in zip(cuts[:-1], cuts[1:])])
    t['dAl'] = sum_planes(t['planes'])
    t['dS2'] = (Asq[0] * gv[None, :]) @ Asq[1].T
    order = ['T1_a', 'dU', 'T1_b', 'dP_acc0', 'dP_acc1'] + (['Q0', 'Q1'] if kl else [])
    for q in range(2):
        order += ['dP_comb%d' % q, 'T%d_' % q, 'PdPP%d' % q, 'G%d' % q, 'krow%d' % q]
    order += ['gu', 'gs'] + (['klv'] if kl else [])
    for name in order:      # each launch from the outputs before it (restate() reads only taps that are already there)
        k = TAP_OF[name]
        probe = _Partial(t)
        v = restate(probe, M, Z, s, jitter, kl, 'dAl', dtype)[name][0]
        if isinstance(k, str):
            t[k] = v
        else:
            t[k[0]][k[1]] = v
    if not kl:
        del t['Q']
    return t, M, s


class _Partial(dict):
    """taps under construction: an entry that is not there yet reads as zeros of the right shape (restate() computes every entry on each
    call; only the one whose inputs are complete is taken)"""
    def __init__(self, t):
        super().__init__(t)
        ref = t['P']
        self._mq = (ref[0].shape[0], ref[1].shape[0])

    def __missing__(self, k):
        return np.zeros(self._mq)

    def __getitem__(self, k):
        v = dict.__getitem__(self, k) if dict.__contains__(self, k) else self.__missing__(k)
        if isinstance(v, list):
            q_shapes = [(self._mq[q], self._mq[q]) for q in range(2)]
            return [np.zeros(q_shapes[q]) if x is None else x for q, x in enumerate(v)]
        return v
