"""CPU suite: the host references of tests/stage_ref.py pinned to the oracle, so that a GPU-vs-stage_ref failure in test_gpu_stages.py
means the kernel is wrong and not the test's idea of the operation.  Needs no GPU."""
import numpy as np
import pytest
import scipy.linalg as sl
import torch

from conftest import make_problem, relerr
import stage_ref as sr
import zigp_oracle as zo
import zigp_oracle_torch as ot

JITTER = 1e-6


def _latent(p, tag, X):
    """The operands of the chunk loop for one latent, from the oracle's kernel and scipy.linalg's factorisation."""
    Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
    M = Z.shape[0]
    Kuu = zo.rbf_K(Z, None, ell, var) + np.eye(M) * JITTER
    L = sl.cholesky(Kuu, lower=True)
    W = sl.solve_triangular(L, np.eye(M), lower=True)
    u, s2 = p['u_%sm' % tag].reshape(-1), p['u_%ss_sqrt' % tag].reshape(-1) ** 2
    K = zo.rbf_K(Z, X, ell, var)
    P = W.T @ W
    Rt = W @ (s2[:, None] * P - np.eye(M))          # Qt = diag(s^2) P - I, Rt = W Qt = (Q W^T)^T  (latents_forward)
    return dict(M=M, W=W, v=W @ u, s2=s2, K=K, Rt=Rt, var=var, cond=np.linalg.cond(Kuu), alpha=W.T @ (W @ u))


def _compose(X, Y, p, g_offset=0.0):
    out = {}
    for tag in 'fg':
        q = _latent(p, tag, X)
        a1 = sr.forward_a1(q['W'], q['v'], q['K'])
        A1 = a1['A1'][0]
        a2 = sr.forward_a2(q['W'], q['s2'], A1)
        jp = sr.forward_jp(q['Rt'], q['K'], A1)
        q.update(A1=A1, Jp=jp['Jp'][0], mean=a1['s_vA1'][0], sq1=a1['s_A1sq'][0], sq2=a2['s_s2A2sq'][0], kj=jp['s_KJ'][0])
        q['var_value'] = q['var'] - q['sq1'] + q['sq2']
        q['var_grad'] = q['var'] + q['kj']
        out[tag] = q
    fm = out['f']['mean'] + zo.mean_function(X, p).reshape(-1)
    gm = out['g']['mean'] + g_offset
    return out, fm, gm


PROBLEMS = [dict(N=700, M=40, D=2, seed=3, Mg=None, mean=False), dict(N=900, M=33, D=3, seed=5, Mg=57, mean=True)]


def _problem(c):
    X, Y, p = make_problem(c['N'], c['M'], c['D'], seed=c['seed'], Mg=c['Mg'])
    if c['mean']:
        p = dict(p, mean_a=np.array([0.5, -0.25, 0.125]), mean_b=0.2)
    return X, Y, p


@pytest.mark.parametrize('c', PROBLEMS, ids=['square', 'ragged_mean'])
def test_composed_references_reproduce_the_oracle(c):
    """A1, the column sums and the point-wise formulas, composed, give build_predict's nine outputs and elbo's data term within the rule of
    test_gpu_dense.py for the W-form against the oracle's triangular solves: max(1e-9, 1e-13 cond(Kuu)) relative."""
    X, Y, p = _problem(c)
    g_offset = -1.0 if c['mean'] else 0.0
    lat, fm, gm = _compose(X, Y, p, g_offset)
    cond = max(lat['f']['cond'], lat['g']['cond'])
    tol = max(1e-9, 1e-13 * cond)
    ref = zo.build_predict(X, p, JITTER, g_offset)
    for variant in ('var_value', 'var_grad'):      # var - sum A1^2 + sum s^2 A2^2 and var + sum K J'
        fv, gv = lat['f'][variant], lat['g'][variant]
        o = sr.pointwise_np(fm, fv, gm, gv, Y.reshape(-1), p['noise'])
        mine = (o['gfmean'], o['gfvar'], o['gfmeanu'], fm, fv, gm, gv, o['e1'], o['ev'])
        for i, (a, b) in enumerate(zip(mine, ref)):
            e = relerr(a, b.reshape(-1))
            print('cond(Kuu)=%.2e %s out9[%d] relerr=%.2e' % (cond, variant, i, e))
            assert e < tol, (variant, i, e)
        data_ref = zo.elbo(X, Y, p, JITTER, g_offset=g_offset)[1]
        e = abs(np.sum(o['ve']) - data_ref) / abs(data_ref)
        print('cond(Kuu)=%.2e %s data term relerr=%.2e' % (cond, variant, e))
        assert e < tol, (variant, e)


@pytest.mark.parametrize('c', PROBLEMS, ids=['square', 'ragged_mean'])
def test_sum_K_Jp_is_the_variance_term_to_the_rounding_bound(c):
    """sum_m K J' = sum s^2 A2^2 - sum A1^2 holds for ANY W (pure algebra: J' = (W^T W S - I) W^T A1, A1 = W K), so the two sides are two
    evaluations of one polynomial in (K, W, s^2) whose terms' magnitudes sum to  B = |K|^T |W^T| (S |W| |W^T| + I) |W| |K|  per column, at a
    depth of at most 5 M + 16 roundings (K -> A1 -> A2 -> square -> sum, resp. W -> P -> Q^T -> R^T -> J' -> sum): |lhs - rhs| <= 2 gamma_(5M+16) B."""
    X, Y, p = _problem(c)
    lat, _, _ = _compose(X, Y, p)
    for tag in 'fg':
        q = lat[tag]
        M = q['M']
        aW, aK = np.abs(q['W']), np.abs(q['K'])
        B = np.sum(aK * (aW.T @ ((q['s2'][:, None] * (aW @ aW.T) + np.eye(M)) @ (aW @ aK))), 0)
        err = np.abs(q['kj'] - (q['sq2'] - q['sq1']))
        r, k = sr.worst(err, 2 * sr.gamma(5 * M + 16) * B)
        print('latent %s M=%d: identity error / bound = %.3g (column %d)' % (tag, M, r, k))
        assert r <= 1.0


def _rule(name, mine, other, truth, S):
    """err(mine) <= 4 err(other) + 16 eps S, element-wise; returns the largest err(mine) / (eps S)."""
    e_m, e_o = sr.mp_err(mine, truth), sr.mp_err(other, truth)
    bad = e_m > 4 * e_o + 16 * sr.EPS * S
    worst = float(np.max(e_m / (sr.EPS * S)))
    print('%-7s largest err / (eps S): stage_ref %.3g, autograd %.3g' % (name, worst, float(np.max(e_o / (sr.EPS * S)))))
    assert not bad.any(), (name, int(np.argmax(bad)), e_m[bad][:3], e_o[bad][:3])
    return worst


@pytest.mark.parametrize('c', PROBLEMS, ids=['square', 'ragged_mean'])
def test_pointwise_cotangents_against_autograd_at_the_same_doubles(c):
    """gm / gv of both latents and the noise derivative against torch autograd of the oracle's probit_expectations + variational_expectations
    at the SAME float64 (fmean, fvar, gmean, gvar): no conditioning in between, so the rule is err <= 4 err_autograd + 16 eps S against
    the 50-digit evaluation."""
    X, Y, p = _problem(c)
    lat, fm, gm = _compose(X, Y, p)
    fv, gv = lat['f']['var_value'], lat['g']['var_value']
    y = Y.reshape(-1)
    n = 256                                              # points (mpmath is the slow side)
    fm, fv, gm, gv, y = fm[:n], fv[:n], gm[:n], gv[:n], y[:n]
    o = sr.pointwise_np(fm, fv, gm, gv, y, p['noise'])
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (fm, fv, gm, gv)]
    noise = torch.tensor(float(p['noise']), dtype=torch.float64, requires_grad=True)
    e1, e2, ev = ot.probit_expectations(t[2], t[3])
    ve = ot.variational_expectations(e1 * t[0], e2 * t[1], ev * torch.square(t[0]), torch.tensor(y), noise)
    # per-point noise derivative: one backward per output would be slow; d ve_n / d noise through a per-point copy of the noise
    noise_n = torch.full((n,), float(p['noise']), dtype=torch.float64, requires_grad=True)
    ve_n = ot.variational_expectations(e1 * t[0], e2 * t[1], ev * torch.square(t[0]), torch.tensor(y), noise_n)
    torch.sum(ve_n).backward()
    auto = dict(dfm=t[0].grad.numpy(), dfv=t[1].grad.numpy(), dgm=t[2].grad.numpy(), dgv=t[3].grad.numpy(), dnoise=noise_n.grad.numpy(),
                ve=ve.detach().numpy())
    truth = sr.pointwise_mp(fm, fv, gm, gv, y, p['noise'])
    S = sr.pointwise_scales(fm, fv, gm, gv, y, p['noise'])
    for k in ('ve', 'dfm', 'dfv', 'dgm', 'dgv', 'dnoise'):
        _rule(k, o[k], auto[k], truth[k], S[k])


def test_kuf_cotangent_sums_are_the_kernel_gradients():
    """krow's columns are the reverse of KernSE.K: with Phi = sum_mn F_mn K_mn(Z, X, ell, var) and F held fixed, dPhi/dvar = sum_m krow[m,0] / var,
    dPhi/dZ_md = krow[m,1+d] / ell_d^2, dPhi/dell_d = sum_m krow[m,1+D+d] / ell_d^3 (autograd through the oracle's kernel), and F itself is
    dData/dK at fixed W: alpha gm^T + 2 J' diag(gv)."""
    X, Y, p = make_problem(300, 21, 3, seed=11)
    lat, fm, gmn = _compose(X, Y, p)
    y = Y.reshape(-1)
    o = sr.pointwise_np(fm, lat['f']['var_value'], gmn, lat['g']['var_value'], y, p['noise'])
    for tag, gmk, gvk in (('f', 'dfm', 'dfv'), ('g', 'dgm', 'dgv')):
        q = lat[tag]
        Zt, ellt, vart = (torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (p['Z' + tag], p['ell_' + tag], p['var_' + tag]))
        Kt = ot.rbf_K(Zt, torch.tensor(X), ellt, vart)
        # F = dData/dK at fixed W, u, s: autograd through the conditional written with W
        Wt, ut, s2t = torch.tensor(q['W']), torch.tensor(p['u_%sm' % tag].reshape(-1)), torch.tensor(q['s2'])
        Kl = Kt.detach().clone().requires_grad_(True)
        A1 = Wt @ Kl
        A2 = Wt.t() @ A1
        mean = (Wt @ ut) @ A1
        var = float(q['var']) - torch.sum(A1 * A1, 0) + s2t @ (A2 * A2)
        other = lat['g' if tag == 'f' else 'f']
        if tag == 'f':
            e1, e2, ev = ot.probit_expectations(torch.tensor(gmn), torch.tensor(other['var_value']))
            fmean, fvar = mean, var
        else:
            e1, e2, ev = ot.probit_expectations(mean, var)
            fmean, fvar = torch.tensor(fm), torch.tensor(other['var_value'])
        data = torch.sum(ot.variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), torch.tensor(y), torch.tensor(float(p['noise']), dtype=torch.float64)))
        data.backward()
        F = q['alpha'][:, None] * o[gmk][None, :] + 2 * q['Jp'] * o[gvk][None, :]
        tol = max(1e-9, 1e-13 * q['cond'])
        e = relerr(F, Kl.grad.numpy())
        print('latent %s cond(Kuu)=%.2e F = dData/dK relerr %.2e' % (tag, q['cond'], e))
        assert e < tol
        krow, _ = sr.kgrad(q['Jp'], q['K'], q['alpha'], o[gmk], o[gvk], X, p['Z' + tag], 0)
        torch.sum(torch.tensor(F) * Kt).backward()
        ell = np.asarray(p['ell_' + tag])
        D = X.shape[1]
        assert relerr(np.sum(krow[:, 0]) / q['var'], float(vart.grad)) < 1e-11
        assert relerr(krow[:, 1:1 + D] / ell ** 2, Zt.grad.numpy()) < 1e-11
        assert relerr(np.sum(krow[:, 1 + D:1 + 2 * D], 0) / ell ** 3, ellt.grad.numpy()) < 1e-11
        assert relerr(krow[:, 1 + 2 * D], q['K'] @ o[gmk]) < 1e-13
        # the extended-precision reference and the centred bound are the same sums
        kl, bnd = sr.kgrad(q['Jp'], q['K'], q['alpha'], o[gmk], o[gvk], X, p['Z' + tag], 0, centre=p['Z' + tag].mean(0), dtype=np.longdouble)
        r, k = sr.worst(np.abs(np.asarray(kl, dtype=np.float64) - krow), 2 * bnd)
        print('latent %s float64 kgrad reference against longdouble: error / bound %.3g' % (tag, r))
        assert r <= 1.0
        # a row range: n0 > 0 and fewer rows than columns
        k2, _ = sr.kgrad(q['Jp'][:, :200], q['K'][:, :200], q['alpha'], o[gmk][:200], o[gvk][:200], X[:250], p['Z' + tag], 100)
        k3, _ = sr.kgrad(q['Jp'][:, :150], q['K'][:, :150], q['alpha'], o[gmk][:150], o[gvk][:150], X[100:250], p['Z' + tag], 0)
        assert np.array_equal(k2, k3)


def test_rank_update_reference_and_plan_table():
    rs = np.random.RandomState(0)
    A, g = rs.randn(5, 48), rs.randn(48)
    B, h = rs.randn(5, 16), rs.randn(16)
    C, bnd = sr.rank_update([(A, g), (B, h)])
    ref = np.zeros((5, 5))
    for i in range(5):
        for j in range(5):
            ref[i, j] = sum(A[i, n] * g[n] * A[j, n] for n in range(48)) + sum(B[i, n] * h[n] * B[j, n] for n in range(16))
    assert np.all(np.abs(C - ref) <= bnd) and np.all(np.abs(C - C.T) <= bnd)
    # the plan table of the issue: nbm -> (So, Sd)
    table = {1: (64, 32), 2: (64, 32), 3: (64, 32), 4: (64, 32), 5: (32, 16), 6: (16, 8), 7: (16, 8), 8: (16, 8), 9: (16, 8), 16: (16, 8)}
    for nbm, plan in table.items():
        assert sr.syr_plan(nbm) == plan, nbm
    assert sr.slice_windows(64, 64)[:2] == [(0, 16), (16, 32)] and sr.slice_windows(64, 32)[-1] == (992, 1024)


def test_plane_sum_order_and_bounds_reference_side():
    """pw_plane_sum adds what the kernel adds; and the float64 BLAS side of the (B) comparisons stays inside its own half of the bound
    against longdouble (the issue's CPU check, at a smaller size)."""
    rs = np.random.RandomState(1)
    plane = rs.randn(9, 64)
    assert np.allclose(sr.pw_plane_sum(plane, 6), plane[:6].sum(0), rtol=0, atol=1e-14)
    assert np.array_equal(sr.pw_plane_sum(plane, 1), plane[0]) and np.array_equal(sr.pw_plane_sum(plane, 0), np.zeros(64))
    M, Nc = 150, 256
    for spread in (False, True):
        W, K = np.tril(rs.randn(M, M)), rs.randn(M, Nc)
        if spread:
            W = W * 10.0 ** rs.uniform(-8, 8, W.shape)
            K = K * 10.0 ** rs.uniform(-8, 8, K.shape)
        v = rs.randn(M)
        a1 = sr.forward_a1(W, v, K)
        Wl, Kl = W.astype(np.longdouble), K.astype(np.longdouble)
        A1l = Wl @ Kl
        for name, truth in (('A1', A1l), ('s_vA1', v.astype(np.longdouble) @ A1l), ('s_A1sq', np.sum(A1l * A1l, 0))):
            val, bnd = a1[name]
            r, _ = sr.worst(np.abs(np.asarray(val - truth, dtype=np.float64)), bnd / 2)
            print('spread=%d %s: float64 reference error / its half of the bound = %.3g' % (spread, name, r))
            assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# M x M reverse stage: the slice rule, the exact-tier operands, and the whole gradient composed from the references
# ---------------------------------------------------------------------------------------------------------------------------------
def test_split_k_slice_rule_table():
    """run_gemm_sk's S per product and row-block count, as the issue states it: 8 everywhere up to nb = 8; from nb = 9 the full products take
    512 // nb^2 (6 at nb = 9, 3 at nb = 12) while the lower-tile products keep more (8 at nb = 9, 6 at nb = 12)."""
    full, lower = ('y', 'tt', 'full', 's', 'rt'), ('r', 'rfull', 't')
    for nb in range(1, 9):
        assert {sr.sk_slices(n, nb) for n in full + lower} == {8}, nb
    assert {sr.sk_slices(n, 9) for n in full} == {6} and {sr.sk_slices(n, 9) for n in lower} == {8}
    assert {sr.sk_slices(n, 12) for n in full} == {3} and {sr.sk_slices(n, 12) for n in lower} == {6}
    # an 8-step range in 6 slices splits unevenly; every window list tiles its range without gap or overlap
    assert sr.sk_windows('y', 9, 0, 8) == [(64, 65), (65, 66), (66, 68), (68, 69), (69, 70), (70, 72)]
    for name in sr.SK_RANGES:
        for nb in (1, 2, 3, 9, 12):
            for bi in range(nb):
                for bj in range(nb):
                    w, r = sr.sk_windows(name, nb, bi, bj), sr.SK_RANGES[name](bi, bj, nb)
                    if r is None:
                        assert w == []
                        continue
                    assert w[0][0] == r[0] and w[-1][1] == r[1] and all(a[1] == b[0] for a, b in zip(w, w[1:])) and all(b > a for a, b in w)


# the draws of the GPU exact tier (tests/test_gpu_mxm_stages.py): every size at D = 3 in every mode, every D at M = 300 unwhitened
EXACT_DRAWS = [(M, 3, mode) for M in (9, 127, 128, 129, 300, 1100, 1536) for mode in sr.MXM_MODES] + [(300, D, 'diag') for D in (1, 8, 9, 17, 64)]


@pytest.mark.parametrize('M,D,mode', EXACT_DRAWS, ids=lambda v: str(v))
def test_integer_operands_make_the_reverse_stage_exact(M, D, mode):
    """What entitles test_gpu_mxm_stages.py to demand bit equality, on the very draws it uses (sr.mxm_int_seed): every value of the float64
    numpy chain is a multiple of 1/8 (krow: of 1/16, one more halving by Kuu - jitter I) and, for every product, max (|A||B|) stays below
    2^50 -- so every partial sum is exactly representable, in any order, with or without fma."""
    op = sr.mxm_int_operands(M, D, seed=sr.mxm_int_seed(M, D), mode=mode)
    for P in ((None, 'given') if mode == 'diag' else (None,)):
        if P is not None:
            op = dict(op, P=op['W'].T @ op['W'])
        r = sr.mxm_backward(op, mode)
        worst = 0.0
        for name, (val, bnd) in r.items():
            q = 16.0 if name == 'krow' else 8.0
            assert np.array_equal(val * q, np.round(val * q)), (name, M, mode)
            if name in sr.MXM_PRODUCTS[mode]:
                k = sr.sk_terms(sr.MXM_PRODUCTS[mode][name], M)
                mag = np.max(np.where(k > 0, bnd / (2 * sr.gamma(k + 2) + (k == 0)), 0.0))
                worst = max(worst, mag)
        print('M=%d D=%d %s P %s: largest (|A||B|) of a product 2^%.1f' % (M, D, mode, P, np.log2(max(worst, 1.0))))
        assert worst < 2.0 ** 50
        if M > 128:
            assert np.count_nonzero(r['G'][0]) > 0.5 * M * M
            if mode == 'diag':
                far = r['S'][0][-(M % 128 or 128):, :128]                                  # the far lower tile holds something in most places
                assert np.count_nonzero(far) > 0.5 * far.size, (np.count_nonzero(far), far.size)


def _mxm_fixture(D, seed):
    """Two latents, Mf != Mg, neither a multiple of 32, a few hundred rows; lengthscales short enough for cond(Kuu) <= 1e4."""
    X, Y, p = make_problem(300, 21, D, seed=seed, Mg=13, ell=0.12 if D == 2 else 0.45)
    return X, Y, p


def _mxm_forward(X, Y, p, tag, mode, base=None):
    """The chunk loop's operands of one latent: A = W K, the mean / variance the point-wise stage sees, the panel J' and alpha of the Kuf
    cotangent F = alpha gm^T + 2 J' diag(gv).  Unwhitened: what _compose reached (base = its latent: W, v, alpha, K, A1, J', the mean and
    the gradient step's variance), plus the factor L and diag(Kuu^-1); whitened: the same operands for the other two parametrisations."""
    Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
    M = Z.shape[0]
    Kuu = zo.rbf_K(Z, None, ell, var) + np.eye(M) * JITTER
    L = sl.cholesky(Kuu, lower=True)
    u = p['u_%sm' % tag].reshape(-1)
    if mode == 'diag':
        W = base['W']
        return dict(M=M, W=W, L=L, Kuu=Kuu, Z=Z, K=base['K'], A=base['A1'], u=u, var=var, ell=ell, cond=base['cond'],
                    s=p['u_%ss_sqrt' % tag].reshape(-1), v=base['v'], alpha=base['alpha'], dkinv=np.sum(W * W, 0), Jp=base['Jp'], mean=base['mean'],
                    varn=base['var_grad'])
    W = sl.solve_triangular(L, np.eye(M), lower=True)
    K = zo.rbf_K(Z, X, ell, var)
    A = W @ K
    q = dict(M=M, W=W, L=L, Kuu=Kuu, Z=Z, K=K, A=A, u=u, var=var, ell=ell, cond=np.linalg.cond(Kuu))
    if mode == 'white':
        s = p['u_%ss_sqrt' % tag].reshape(-1)
        d = s * s - 1.0
        q.update(s=s, alpha=W.T @ u, Jp=(d[:, None] * W).T @ A, mean=u @ A, varn=var + d @ (A * A))
    else:
        Lq = np.tril(np.asarray(p['u_%ss_sqrt' % tag]).reshape(M, M))
        TmI = Lq @ Lq.T - np.eye(M)
        q.update(s=Lq, alpha=W.T @ u, Jp=(TmI @ W).T @ A, mean=u @ A, varn=var + np.sum(A * (TmI @ A), 0))
    return q


def _mxm_gradient(X, Y, p, mode, include_kl=True, rows=True):
    """The whole gradient from the stage references: forward operands, point-wise cotangents, rank-N update, Kuf cotangent sums, the M x M
    reverse stage, the pack formulas."""
    D = X.shape[1]
    base = _compose(X, Y, p)[0] if mode == 'diag' else dict(f=None, g=None)      # the unwhitened forward is the existing composition
    lat = {tag: _mxm_forward(X, Y, p, tag, mode, base[tag]) for tag in 'fg'}
    g = {}
    if rows:
        o = sr.pointwise_np(lat['f']['mean'], lat['f']['varn'], lat['g']['mean'], lat['g']['varn'], Y.reshape(-1), p['noise'])
        g['noise'] = np.sum(o['dnoise'])
    else:
        g['noise'] = 0.0
    for tag, gmk, gvk in (('f', 'dfm', 'dfv'), ('g', 'dgm', 'dgv')):
        q = lat[tag]
        M = q['M']
        krow = np.zeros((sr.KG_SPLIT, M, 2 + 2 * D))
        op = dict(W=q['W'], L=q['L'], Kuu=q['Kuu'], Z=q['Z'], s=q['s'], alpha=q['alpha'], v=q.get('v'), jitter=JITTER, krow=krow)
        if rows:
            gm, gv = o[gmk], o[gvk]
            op['C1'] = sr.rank_update([(q['A'], gv)])[0]
            krow[0] = sr.kgrad(q['Jp'], q['K'], q['alpha'], gm, gv, X, q['Z'], 0)[0]
        r = sr.mxm_backward(op, mode, with_data=rows, with_kl=include_kl)
        q['G'] = r['G'][0]
        zero = np.zeros(M)
        du = r['du'][0] if 'du' in r else (r['a1gm'][0] if rows else zero)
        dsq = r['dsq'][0] if 'dsq' in r else zero
        if mode == 'diag':
            pk = sr.dense_pack(r['krow'][0], du, dsq, q['s'], q['ell'], q['var'], include_kl, q['alpha'], q['dkinv'])
        elif mode == 'white':
            pk = sr.dense_pack(r['krow'][0], du, dsq, q['s'], q['ell'], q['var'], include_kl, q['u'], 1.0)
        else:
            pk = sr.dense_pack(r['krow'][0], du, dsq, None, q['ell'], q['var'], include_kl, q['u'], None)
            pk['ds'] = r['dLq'][0]
        g['Z' + tag], g['u_%sm' % tag], g['u_%ss_sqrt' % tag], g['ell_' + tag] = pk['dZ'], pk['du'], pk['ds'], pk['dell']
        g['var_' + tag] = pk['dvar'] + (np.sum(o[gvk]) if rows else 0.0)
    return g, lat


# Largest relative difference per block (relative to the block's largest entry) between the composed references and the oracle's autograd,
# measured on these fixtures (all modes, D = 2 and 5, with and without KL / rows): 1.37e-13 / 3.8e-14 (unwhitened, D = 2 / 5), 4.3e-14 /
# 1.6e-14 (whitened), 1.51e-13 / 2.0e-14 (full covariance).  The assertion is ten times the largest, far under the cap 1e-9.
MXM_PIN_MEASURED = 1.6e-13
MXM_PIN_CAP = 1e-9


def _mxm_oracle(mode):
    import whiten_ref
    import fullcov_ref
    return {'diag': ot, 'white': whiten_ref, 'white_full': fullcov_ref}[mode]


@pytest.mark.parametrize('D', [2, 5])
@pytest.mark.parametrize('mode', sr.MXM_MODES)
def test_composed_reverse_stage_is_the_oracle_gradient(mode, D):
    """Every key of PARAM_KEYS from the stage references (forward operands -> point-wise cotangents -> C1 and krow -> sr.mxm_backward ->
    sr.dense_pack) against elbo_and_grad of the oracle (unwhitened), tests/whiten_ref.py and tests/fullcov_ref.py, with the KL, without it,
    and with no rows (then G = -dKL/dKuu, also asserted in closed form).  cond(Kuu) <= 1e4 for both latents, so the project's rule
    1e-13 cond caps the difference at 1e-9 relative per block.  Measured: at most 1.51e-13 relative per block (full covariance, D = 2); the
    assertion is ten times the measured floor, 1.6e-12 (MXM_PIN_MEASURED): two float64 evaluations in different summation orders."""
    import fullcov_ref
    X, Y, p = _mxm_fixture(D, seed=21 + D)
    if mode == 'white_full':
        p = fullcov_ref.make_lq(p, seed=D, negative=1)
    worst = 0.0
    for include_kl, rows in ((True, True), (False, True), (True, False)):
        g, lat = _mxm_gradient(X, Y, p, mode, include_kl, rows)
        assert max(lat['f']['cond'], lat['g']['cond']) <= 1e4, (lat['f']['cond'], lat['g']['cond'])
        Xr, Yr = (X, Y) if rows else (X[:0], Y[:0])
        ref = _mxm_oracle(mode).elbo_and_grad(Xr, Yr, p, JITTER, include_kl=include_kl)[3]
        for k in ot.PARAM_KEYS:
            a, b = np.asarray(g[k], dtype=np.float64).reshape(-1), np.asarray(ref[k], dtype=np.float64).reshape(-1)
            scale = np.max(np.abs(b))
            e = float(np.max(np.abs(a - b)) / scale) if scale > 0 else float(np.max(np.abs(a)))
            worst = max(worst, e)
            print('MXM-PIN %s D=%d kl=%d rows=%d %-10s cond %.1e / %.1e  rel diff %.2e' % (mode, D, include_kl, rows, k, lat['f']['cond'], lat['g']['cond'], e))
            assert e <= MXM_PIN_CAP, (k, e)
            assert e <= 10 * MXM_PIN_MEASURED, (k, e)
        if not rows and mode == 'diag':      # G = -dKL/dKuu = -1/2 (Kuu^-1 - alpha alpha^T - Kuu^-1 diag(s^2) Kuu^-1)
            for tag in 'fg':
                q = lat[tag]
                Ki = np.linalg.inv(q['Kuu'])
                G = -0.5 * (Ki - np.outer(q['alpha'], q['alpha']) - Ki @ np.diag(q['s'] ** 2) @ Ki)
                assert relerr(q['G'], G) <= 1e-13 * q['cond'] + 1e-12
        if not rows and mode != 'diag':      # the whitened KL does not see Kuu
            assert not lat['f']['G'].any() and not lat['g']['G'].any()
    print('MXM-PIN %s D=%d largest rel diff over all blocks %.2e' % (mode, D, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# Kronecker stage references (tests/test_gpu_kron_stages.py)
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_FM = [-40, -8, -3, -1, -1e-3, 0, 1e-3, 1, 3, 8, 40]
HEAD_FV = [1e-10, 1e-3, 0.1, 1, 10, 1e3, 1e6]


@pytest.mark.parametrize('lik,noise', [('bernoulli', 1.0), ('gaussian', 1e-4), ('gaussian', 1e-2), ('gaussian', 1.0)])
def test_head_reference_alone_is_within_4_eps_S_of_the_truth(lik, noise):
    """The premise of err_gpu <= 4 err_np + 16 eps S: head_np over the GPU test's grid, at the doubles 1 + (target - 1) the kernel is given,
    stays below 4 eps S of the 50-digit head_mp on every output, nothing excluded (largest figure on this grid: 1.3)."""
    ys = [0, 1, 0.5] if lik == 'bernoulli' else [0, 0.7, -3]
    fm, fv, y = np.array(np.meshgrid(HEAD_FM, HEAD_FV, ys, indexing='ij'), dtype=np.float64).reshape(3, -1)
    fv = 1.0 + (fv - 1.0)
    ref, truth, S = sr.head_np(lik, fm, fv, y, noise), sr.head_mp(lik, fm, fv, y, noise), sr.head_scales(lik, fm, fv, y, noise)
    for k in sr.HEAD_OUTPUTS:
        r = sr.mp_err(ref[k], truth[k]) / (sr.EPS * S[k])
        i = int(np.argmax(r))
        print('head %-9s noise %-6g %-6s largest err_np / (eps S) = %.3g at fm %g fv %g y %g' % (lik, noise, k, r[i], fm[i], fv[i], y[i]))
        assert r[i] < 4.0, (lik, noise, k, r[i])
    if lik == 'bernoulli':       # y == 1 exactly is 'on'; 0.5 is 'off', as 0
        on, off, half = y == 1.0, y == 0.0, y == 0.5
        assert np.array_equal(ref['ve'][off], ref['ve'][half]) and not np.array_equal(ref['ve'][on], ref['ve'][off])
        assert all(a == b for a, b in zip(truth['ve'][off], truth['ve'][half]))


def test_dyadic_evaluation_points_are_exact_in_every_association():
    """stage_ref.kron_dyadic_case in exact rationals: every partial result of Knn - q0 q1 + st in either association (and the product
    itself, so also with the product fused into the subtraction) and of mean + offset is a double, so the float64 statement is THE value."""
    from fractions import Fraction as F
    c = sr.kron_dyadic_case()
    exact = lambda x: F(float(x)) == x
    for part, var, off in ((c['part_f'], c['var_f'], c['f_offset']), (c['part_g'], c['var_g'], c['g_offset'])):
        knn = var[0] * var[1]
        mean, fv = sr.kron_pw_inputs(part, knn, off)
        assert F(knn) == F(var[0]) * F(var[1])
        for n in range(part.shape[1]):
            q0, q1, mu, st = (F(float(part[r, n])) for r in range(4))
            for v in (q0, q1, mu, st):
                assert (v * 1024).denominator == 1 and abs(v) <= 64
            prod = q0 * q1
            steps = (prod, F(knn) - prod, F(knn) - prod + st, F(knn) + st, st - prod, mu + F(off))
            assert all(exact(s) for s in steps), n
            assert F(float(fv[n])) == F(knn) - prod + st and F(float(mean[n])) == mu + F(off)
        assert fv[0] == 2.0 ** -20 and fv[1] == 2.0 ** -20 and abs(part[0, 0] * part[1, 0]) >= var[0] * var[1]
        assert np.all(fv[2:] > 1.0)


@pytest.mark.parametrize('M,D,N', [(5, 1, 1), (16, 3, 257), (33, 8, 1000)])
def test_kron_panel_restatements_float64_against_longdouble(M, D, N):
    """float64 against the longdouble evaluation of the same statement, within the statement's own bound (+ 2^-11 of it for the reference)."""
    Nc = 1024
    o = sr.kron_panel_operands('normal', M, D, N, Nc, seed=M + D, M1=M + 3)
    L = np.longdouble
    a = (o['K'], o['A'], o['K1'], o['A1'], o['B'], o['Asq'], o['C'])
    (r64, b), (rl, _) = sr.kron_colsum(*a), sr.kron_colsum(*a, dtype=L)
    assert sr.worst(np.abs(r64 - rl), b * (1 + 2.0 ** -11))[0] <= 1.0
    a = (o['A'], o['C'], o['K'], o['gv'], o['dq'])
    for (r64, b), (rl, _) in zip(sr.kron_da(*a), sr.kron_da(*a, dtype=L)):
        assert sr.worst(np.abs(r64 - rl), b * (1 + 2.0 ** -11))[0] <= 1.0
    a = (o['B'], o['A'], o['PdA'], o['K'], o['gm'], o['dq'], o['X'], o['col0'], o['Z'])
    (r64, b), (rl, _) = sr.kron_kgrad(*a, krow0=o['krow0']), sr.kron_kgrad(*a, krow0=o['krow0'], dtype=L)
    ratio = sr.worst(np.abs(r64 - rl), b * (1 + 2.0 ** -11))[0]
    print('kron_kgrad float64 / longdouble: largest error / bound %.3g' % ratio)
    assert ratio <= 1.0
    assert np.array_equal(r64[:, 1 + 2 * D], o['krow0'][:, 1 + 2 * D])
    # the columns n >= N are not part of the statement
    a2 = tuple(np.where(np.arange(Nc) < N, x, 1e300) if isinstance(x, np.ndarray) and x.shape[-1] == Nc else x for x in a)
    assert np.array_equal(sr.kron_kgrad(*a2, krow0=o['krow0'])[0], r64)
    K64, y = sr.kron_kbuild(o['X'], o['col0'], o['Z'], np.full(D, 0.7), 1.7, Nc)
    Kl, yl = sr.kron_kbuild(o['X'], o['col0'], o['Z'], np.full(D, 0.7), 1.7, Nc, dtype=L)
    assert np.all(np.abs(K64 - Kl) <= (4.0 + 8.0 * yl) * np.finfo(np.float64).eps * Kl + L(5e-324))
    assert np.array_equal(K64[:, N:], np.repeat(K64[:, N:N + 1], Nc - N, 1)) and K64[:, N:].all()      # the kernel at x = 0, not zero


@pytest.mark.parametrize('M,D,N', [(5, 1, 1), (16, 3, 257), (33, 8, 1000)])
def test_kron_panel_integer_operands_are_exact(M, D, N):
    """The premise of the bit-equal tier: integer operands, every magnitude sum far below 2^53, and the float64 statement equal to the
    longdouble one."""
    Nc = 1024
    o = sr.kron_panel_operands('int', M, D, N, Nc, seed=M + D, M1=M + 3)
    for k, v in o.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, np.round(v)) and np.max(np.abs(v)) <= 3, k
    L = np.longdouble
    a = (o['K'], o['A'], o['K1'], o['A1'], o['B'], o['Asq'], o['C'])
    (r64, b), (rl, _) = sr.kron_colsum(*a), sr.kron_colsum(*a, dtype=L)
    assert np.array_equal(r64, rl) and np.max(b) / sr.gamma(M + 2) < 2.0 ** 40
    a = (o['A'], o['C'], o['K'], o['gv'], o['dq'])
    for (r64, b), (rl, _) in zip(sr.kron_da(*a), sr.kron_da(*a, dtype=L)):
        assert np.array_equal(r64, rl) and np.max(np.abs(r64)) <= 63
    a = (o['B'], o['A'], o['PdA'], o['K'], o['gm'], o['dq'], o['X'], o['col0'], o['Z'])
    (r64, b), (rl, _) = sr.kron_kgrad(*a, krow0=o['krow0']), sr.kron_kgrad(*a, krow0=o['krow0'], dtype=L)
    assert np.array_equal(r64, rl) and np.array_equal(r64, np.round(r64)) and np.max(b) / sr.gamma(N + 9) < 2.0 ** 40
