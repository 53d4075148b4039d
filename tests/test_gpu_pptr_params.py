"""cfg5 on the REAL precipitation parameters (tests/golden/pptr.npz = the reference's data/pptr.pickle; init of scripts/onoff.py:51-76:
l_s = 8 on a 10-degree domain, sigma^2 = 20 / 10, l_t = 5e-3, u = 0.1 randn, jitter 1e-5 :18): a 1000-row minibatch (scripts/onoff.py:55),
full gradient against the literal dense oracle + autograd, and the 9-tuple of predict_onoff (jitter 1e-6 onofftf/onoffpred.py:13,
gmean - 1 :141) -- on BASELINE's 32 x 32 grid and on the reference's own [10, 100] (:52-53).

The spatial factor is the badly conditioned one.  Where the GPU's factored evaluation and the literal dense order
part by more than 1e-6, the test applies the rule of tests/test_gpu_kron.py: the GPU must stay within 3x of the OP-ORDER FLOOR -- the
distance from the oracle of the same factored identities evaluated on the CPU with the oracle's own LU inverse (values) or its autograd
(gradients) -- and within 10x of the oracle's own error against a 40-digit evaluation.  Every number is printed (and recorded in
HISTORY.md section 1)."""
import os

import mpmath as mp
import numpy as np
import pytest

from conftest import relerr
from test_gpu_kron import _factored_with_oracle_inverse, _mp_kron_inf

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
NAMES = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')


from kron_nd import pptr_problem as _pptr_params      # noqa: E402  (the fixture lives with the other Kronecker problems; the name is kept for its users)


def _inv_compensated():
    """torch.linalg.inv whose reverse pass -P^T dP P^T is evaluated in 40-digit arithmetic and rounded once (forward: the plain LU
    inverse).  That product is the one place where the factored reverse pass loses digits on an ill-conditioned factor
    (tools/dd_experiment.py); the engine carries it in two-double arithmetic (kf_dd_mac, csrc/zigp_kronf.hip)."""
    import torch

    class Inv(torch.autograd.Function):
        @staticmethod
        def forward(ctx, K):
            P = torch.linalg.inv(K)
            ctx.save_for_backward(P)
            return P

        @staticmethod
        def backward(ctx, dP):
            (P,) = ctx.saved_tensors
            with mp.workdps(40):
                Pm, dPm = mp.matrix(P.numpy().tolist()), mp.matrix(dP.numpy().tolist())
                G = -(Pm.T * dPm * Pm.T)
                out = np.array([[float(G[i, j]) for j in range(G.cols)] for i in range(G.rows)])
            return torch.as_tensor(out, dtype=P.dtype)

    return Inv.apply


def _factored_elbo_and_grad_torch(X, Y, p_np, jitter, scale, compensated=False):
    """The FACTORED identities the engine evaluates (HISTORY.md section 5b / SURVEY.md a10, a11), on the CPU in torch with the oracle's own
    inverse (torch.linalg.inv, LU) and autograd: its distance from the literal dense order is what the op order alone costs.
    compensated: the reverse pass of the inverse in 40 digits (_inv_compensated) -- the accurate evaluation of the same algebra, against
    which the literal oracle's OWN float64 error on the ill-conditioned gradient blocks is measured."""
    import torch
    import zigp_oracle_torch as ot
    t = ot._t
    inv = _inv_compensated() if compensated else torch.linalg.inv
    p = {k: [t(v).clone().requires_grad_(True) for v in p_np[k]] for k in ot.KRON_KEYS}
    for k in ot.KRON_VEC_KEYS:
        p[k] = t(p_np[k]).clone().requires_grad_(True)
    Xt, Yt = t(X), t(Y).reshape(-1, 1)

    def latent(tag):
        Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
        M0, M1 = Z[0].shape[0], Z[1].shape[0]
        K = [ot.rbf_K(Z[q], None, ell[q], var[q]) + torch.eye(Z[q].shape[0], dtype=ot.DT) * jitter for q in range(2)]
        P = [inv(Kq) for Kq in K]
        d0 = Z[0].shape[1]
        k0, k1 = ot.rbf_K(Z[0], Xt[:, :d0], ell[0], var[0]), ot.rbf_K(Z[1], Xt[:, d0:], ell[1], var[1])
        U, S2 = p['u_%sm' % tag].reshape(M0, M1), torch.square(p['u_%ss_sqrt' % tag]).reshape(M0, M1)
        Al = P[0] @ U @ P[1]
        a0, a1 = P[0] @ k0, P[1] @ k1
        mu = torch.einsum('in,ij,jn->n', k0, Al, k1)
        vv = var[0] * var[1] - (k0 * a0).sum(0) * (k1 * a1).sum(0) + torch.einsum('in,ij,jn->n', a0 ** 2, S2, a1 ** 2)
        kl = 0.5 * (torch.sum(U * Al) - M0 * M1 - torch.sum(torch.log(S2))
                    + torch.einsum('i,ij,j->', torch.diagonal(P[0]), S2, torch.diagonal(P[1]))
                    + M1 * torch.logdet(K[0]) + M0 * torch.logdet(K[1]))
        return mu.reshape(-1, 1), vv.reshape(-1, 1), kl

    fm, fv, klf = latent('f')
    gm, gv, klg = latent('g')
    e1, e2, ev = ot.probit_expectations(gm, gv)
    data = torch.sum(ot.variational_expectations(e1 * fm, e2 * fv, ev * torch.square(fm), Yt, p['noise']))
    elbo = data * scale - (klf + klg)
    elbo.backward()
    g = {k: [v.grad.numpy().copy() for v in p[k]] for k in ot.KRON_KEYS}
    for k in ot.KRON_VEC_KEYS:
        g[k] = p[k].grad.numpy().copy()
    return float(elbo.detach()), float(data.detach()), float((klf + klg).detach()), g


def _conds(p, jit):
    import zigp_oracle as o
    out = {}
    for tag in ('f', 'g'):
        for q, nm in ((0, 's'), (1, 't')):
            K = o.rbf_K(p['Z' + tag][q], None, p['ell_' + tag][q], float(np.squeeze(p['var_' + tag][q]))) + jit * np.eye(p['Z' + tag][q].shape[0])
            out['K_%s(%s)' % (nm, tag)] = np.linalg.cond(K)
    return out


@pytest.mark.parametrize('grid', [(32, 32), (10, 100)])
def test_pptr_init_minibatch_gradient_matches_literal_oracle(engine, grid):
    """Full gradient of a 1000-row minibatch step at the pptr init.  Tolerance 1e-6 (north_star) against the literal oracle -- except
    where the ORACLE's own float64 error is larger: at 32 x 32 (cond(K_s) = 5e7) the literal order itself is only good to ~1e-3 on
    d / d Z_s.  Its error is measured against the accurate evaluation of the same algebra (CPU, reverse pass of the inverse in 40
    digits), and the GPU must (i) be at least as close to that evaluation as the oracle is, (ii) differ from the oracle by no more than
    2x the oracle's own error.  (Rounds 2-3 allowed 3x the distance of a float64 CPU evaluation of the factored algebra instead: the
    engine was then less accurate than the reference's op order on those blocks)"""
    import zigp_oracle_torch as ot
    Xtr, Ytr, xb, yb, p = _pptr_params(grid)
    jit, scale = 1e-5, Xtr.shape[0] / 1000.0                                  # scripts/onoff.py:18,311
    print('\npptr init, grid %s, jitter %g: cond ' % (grid, jit) + ', '.join('%s %.2e' % kv for kv in _conds(p, jit).items()))
    ed, kl, g = engine.kron_elbo(p, xb, yb, jitter=jit, scale=scale)
    e_r, d_r, kl_r, g_r = ot.kron_elbo_and_grad(xb, yb, p, jit, scale=scale)
    e_c, d_c, kl_c, g_c = _factored_elbo_and_grad_torch(xb, yb, p, jit, scale)
    e_a, d_a, kl_a, g_a = _factored_elbo_and_grad_torch(xb, yb, p, jit, scale, compensated=True)
    print('  data term: gpu %.12e oracle %.12e (rel %.2e; CPU factored %.2e)   KL: gpu %.10e oracle %.10e (rel %.2e; CPU factored %.2e)'
          % (ed, scale * d_r, abs(ed - scale * d_r) / abs(scale * d_r), abs(scale * d_c - scale * d_r) / abs(scale * d_r),
             kl, kl_r, abs(kl - kl_r) / abs(kl_r), abs(kl_c - kl_r) / abs(kl_r)))
    assert abs(ed - scale * d_r) <= 1e-6 * abs(scale * d_r)
    assert abs(kl - kl_r) <= 1e-7 * abs(kl_r)
    worst = worst_a = 0.0
    for k in ('Zf', 'Zg', 'ell_f', 'ell_g', 'var_f', 'var_g', 'u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'noise'):
        a_, b_, c_, d_ = g[k], g_r[k], g_c[k], g_a[k]
        for q, (a, b, c, d) in enumerate(zip(a_, b_, c_, d_) if isinstance(b_, list) else ((a_, b_, c_, d_),)):
            a, b, c, d = (np.asarray(v).reshape(-1) for v in (a, b, c, d))
            e_gpu, fac64 = relerr(a, b), relerr(c, b)
            e_gpu_acc, e_orc_acc = relerr(a, d), relerr(b, d)
            worst, worst_a = max(worst, e_gpu), max(worst_a, e_gpu_acc)
            print('  grad %-10s[%d] gpu vs oracle %.2e | vs the accurate evaluation: gpu %.2e, literal oracle %.2e | float64 CPU factored vs oracle %.2e   max|ref| %.3e'
                  % (k, q, e_gpu, e_gpu_acc, e_orc_acc, fac64, np.max(np.abs(b))))
            assert e_gpu < max(1e-6, 2.0 * e_orc_acc), (k, q, e_gpu, e_orc_acc)
            assert e_gpu_acc < max(1e-6, e_orc_acc), (k, q, e_gpu_acc, e_orc_acc)
    print('  worst gradient block: vs oracle %.2e, vs the accurate evaluation %.2e' % (worst, worst_a))


@pytest.mark.parametrize('grid', [(32, 32), (10, 100)])
def test_pptr_init_predict_9tuple_matches_literal_oracle(engine, grid):
    import zigp_oracle as o
    Xtr, Ytr, xb, yb, p = _pptr_params(grid)
    jit, goff = 1e-6, -1.0                                                    # onofftf/onoffpred.py:13,141
    print('\npptr init predict, grid %s, jitter %g: cond ' % (grid, jit) + ', '.join('%s %.2e' % kv for kv in _conds(p, jit).items()))
    out = engine.kron_predict(p, xb, jitter=jit, g_offset=goff)
    ref = o.kron_build_predict(xb, p, jit, goff)
    errs = [relerr(out[i], ref[i].reshape(-1)) for i in range(9)]
    print('  9-tuple gpu vs oracle: ' + ', '.join('%s %.2e' % (n, e) for n, e in zip(NAMES, errs)))
    npts = 12
    for tag, (im, iv) in (('f', (3, 4)), ('g', (5, 6))):
        cm, cv = _factored_with_oracle_inverse(xb, p, tag, jit)
        tm, tv = _mp_kron_inf(xb, p['Z' + tag], p['ell_' + tag], [float(np.squeeze(v)) for v in p['var_' + tag]], p['u_%sm' % tag],
                              p['u_%ss_sqrt' % tag], jit, npts)
        if tag == 'g':
            cm, tm = cm + goff, tm + goff
        for nm, idx, cpu, truth in (('mean', im, cm, tm), ('var', iv, cv, tv)):
            e, floor = relerr(out[idx], ref[idx].reshape(-1)), relerr(cpu, ref[idx].reshape(-1))
            e_gpu, e_orc = relerr(out[idx][:npts], truth), relerr(ref[idx].reshape(-1)[:npts], truth)
            print('  %s%s: gpu vs oracle %.2e, op-order floor %.2e | vs 40 digits (12 points): gpu %.2e, oracle %.2e' % (tag, nm, e, floor, e_gpu, e_orc))
            assert e < max(1e-6, 3.0 * floor), (tag, nm, e, floor)
            assert e_gpu < max(1e-6, 10 * e_orc), (tag, nm, e_gpu, e_orc)
    # the moments downstream of (mean, var) inherit their error, no more
    assert max(errs) < max(1e-6, 3.0 * max(errs[3:7]))



def _mp_latent(X, Z, ell, var, u, s, jit):
    """factored kron_inf + GaussKLkron pieces in 40 digits: -> (mu list, var list, KL)"""
    n = X.shape[0]
    f = lambda v: v.v if isinstance(v, _MpScalar) else mp.mpf(float(v))
    def kmat(A, B, l, v):
        return mp.matrix([[f(v) * mp.exp(-sum(((f(a[d]) - f(b[d])) / f(l[d])) ** 2 for d in range(len(l))) / 2) for b in B] for a in A])
    K, P, ks, c0 = [], [], [], 0
    for q in range(2):
        Kq = kmat(Z[q], Z[q], ell[q], var[q])
        for i in range(Z[q].shape[0]):
            Kq[i, i] += mp.mpf(jit)
        K.append(Kq); P.append(Kq ** -1)
        ks.append(kmat(Z[q], X[:, c0:c0 + Z[q].shape[1]], ell[q], var[q]))
        c0 += Z[q].shape[1]
    M0, M1 = Z[0].shape[0], Z[1].shape[0]
    U = mp.matrix(M0, M1); S2 = mp.matrix(M0, M1)
    for i in range(M0):
        for j in range(M1):
            U[i, j] = f(u[i * M1 + j]); S2[i, j] = f(s[i * M1 + j]) ** 2
    Al = P[0] * U * P[1]
    a0, a1 = P[0] * ks[0], P[1] * ks[1]
    B1 = Al * ks[1]                      # (M0, n)
    a0sq = mp.matrix(M0, n); a1sq = mp.matrix(M1, n)
    for i in range(M0):
        for k in range(n): a0sq[i, k] = a0[i, k] ** 2
    for j in range(M1):
        for k in range(n): a1sq[j, k] = a1[j, k] ** 2
    C1 = S2 * a1sq
    knn = f(var[0]) * f(var[1])
    mu, vv = [], []
    for k in range(n):
        m = sum(ks[0][i, k] * B1[i, k] for i in range(M0))
        q0 = sum(ks[0][i, k] * a0[i, k] for i in range(M0)); q1 = sum(ks[1][j, k] * a1[j, k] for j in range(M1))
        st = sum(a0sq[i, k] * C1[i, k] for i in range(M0))
        mu.append(m); vv.append(knn - q0 * q1 + st)
    kl = sum(U[i, j] * Al[i, j] for i in range(M0) for j in range(M1)) - M0 * M1 - sum(mp.log(S2[i, j]) for i in range(M0) for j in range(M1)) \
        + sum(P[0][i, i] * S2[i, j] * P[1][j, j] for i in range(M0) for j in range(M1)) + M1 * mp.log(mp.det(K[0])) + M0 * mp.log(mp.det(K[1]))
    return mu, vv, kl / 2


def _mp_data_term(fm, fv, gm, gv, Y, noise):
    tot = mp.mpf(0)
    c1, c0 = 1 - mp.mpf('2e-3'), mp.mpf('1e-3')
    for k in range(len(fm)):
        z = gm[k] / mp.sqrt(1 + gv[k]); a = 1 / mp.sqrt(1 + 2 * gv[k])
        cdf = (1 + mp.erf(z / mp.sqrt(2))) / 2 * c1 + c0
        T = mp.atan(a) / (2 * mp.pi) * mp.exp(-(z * z) * (a * a + 1) / 2)
        e1, e2r, evr = cdf, cdf - 2 * T, cdf - 2 * T - cdf * cdf
        e2, ev = (e2r + abs(e2r)) / 2, (evr + abs(evr)) / 2
        y = mp.mpf(float(Y[k]))
        q = (y - e1 * fm[k]) ** 2 + e2 * fv[k] + ev * fm[k] ** 2
        tot += -mp.log(2 * mp.pi) / 2 - mp.log(mp.mpf(float(noise))) / 2 - q / (2 * mp.mpf(float(noise)))
    return tot


def test_pptr_init_illconditioned_gradient_entries_against_40_digit_differences(engine):
    """At the pptr init on the 32 x 32 grid cond(K_s) ~ 5e7 and the gradient with respect to the SPATIAL inducing inputs and hyperparameters
    is determined to ~1e-2 only in float64: the literal dense oracle and the factored identities (both on the CPU, both with an LU
    inverse) differ by that much.  Truth for a handful of entries: central differences of the ELBO evaluated in 40-digit arithmetic
    (100 rows).  CPU dry run: on the largest dZ_s entry of f the literal order is off by 4e-5 and the factored identities by 2e-3 (the
    explicit K_s^-1 enters the reverse pass twice); the lengthscale entries by 1e-8 .. 2e-7.  The GPU carries that product in two-double
    arithmetic (round 4) and must be within 1e-7 or AT LEAST AS CLOSE AS THE LITERAL ORACLE on every probed entry -- the numbers are printed."""
    import zigp_oracle_torch as ot
    Xtr, Ytr, xb, yb, p = _pptr_params((32, 32))
    n, jit, scale = 100, 1e-5, 7.0
    X, Y = xb[:n], yb[:n]
    mp.mp.dps = 40
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=jit, scale=scale)
    e_r, d_r, kl_r, g_r = ot.kron_elbo_and_grad(X, Y, p, jit, scale=scale)
    e_c, d_c, kl_c, g_c = _factored_elbo_and_grad_torch(X, Y, p, jit, scale)
    e_a, d_a, kl_a, g_a = _factored_elbo_and_grad_torch(X, Y, p, jit, scale, compensated=True)   # the yardstick of the minibatch test, validated here
    noise = float(np.squeeze(p['noise']))

    def latent(pp, tag):
        return _mp_latent(X, pp['Z' + tag], pp['ell_' + tag], [float(np.squeeze(v)) for v in pp['var_' + tag]], pp['u_%sm' % tag].reshape(-1),
                          pp['u_%ss_sqrt' % tag].reshape(-1), jit)

    base = {t: latent(p, t) for t in ('f', 'g')}

    def elbo_mp(pp, tag):            # only latent `tag` differs from p
        lat = dict(base)
        lat[tag] = latent(pp, tag)
        return mp.mpf(scale) * _mp_data_term(lat['f'][0], lat['f'][1], lat['g'][0], lat['g'][1], Y.reshape(-1), noise) - (lat['f'][2] + lat['g'][2])

    d0 = _mp_data_term(base['f'][0], base['f'][1], base['g'][0], base['g'][1], Y.reshape(-1), noise)
    print('\n100 rows, 32 x 32: data term vs 40 digits: gpu %.2e oracle %.2e | KL: gpu %.2e oracle %.2e'
          % (abs(ed / scale - float(d0)) / abs(float(d0)), abs(d_r - float(d0)) / abs(float(d0)),
             abs(kl - float(base['f'][2] + base['g'][2])) / abs(kl_r), abs(kl_r - float(base['f'][2] + base['g'][2])) / abs(kl_r)))
    h = mp.mpf('1e-12')
    for tag in ('f', 'g'):
        iz = np.unravel_index(np.argmax(np.abs(g_r['Z' + tag][0])), g_r['Z' + tag][0].shape)
        for what in ('Z', 'ell'):
            vals = {}
            for sgn in (+1, -1):
                pp = dict(p)
                if what == 'Z':
                    # the perturbed entry must stay exact in 40 digits: patch it after the float conversion inside _mp_latent
                    pp['Z' + tag] = [_Perturbed(p['Z' + tag][0], iz, sgn * h), p['Z' + tag][1]]
                else:
                    pp['ell_' + tag] = [_Perturbed(p['ell_' + tag][0], (0,), sgn * h), p['ell_' + tag][1]]
                vals[sgn] = elbo_mp(pp, tag)
            truth = float((vals[+1] - vals[-1]) / (2 * h))
            if what == 'Z':
                got, orc, fac, acc = g['Z' + tag][0][iz], g_r['Z' + tag][0][iz], g_c['Z' + tag][0][iz], g_a['Z' + tag][0][iz]
            else:
                got, orc, fac, acc = g['ell_' + tag][0][0], g_r['ell_' + tag][0][0], g_c['ell_' + tag][0][0], g_a['ell_' + tag][0][0]
            e_gpu, e_orc, e_fac, e_acc = (abs(v - truth) / abs(truth) for v in (got, orc, fac, acc))
            print('  d ELBO / d %s_%s[0]%s = %.10e (40-digit differences): gpu off by %.2e, literal oracle %.2e, CPU factored float64 %.2e, '
                  'CPU factored with the compensated inverse reverse pass %.2e' % (what, tag, list(iz) if what == 'Z' else '[0]', truth, e_gpu, e_orc, e_fac, e_acc))
            assert e_acc < max(1e-7, e_orc), (tag, what, e_acc, e_orc)      # the yardstick is at least as good as the oracle
            assert e_gpu < max(1e-7, e_orc), (tag, what, e_gpu, e_orc, e_fac)          # no less accurate than the reference's op order


class _Perturbed:
    """array whose entry `idx` reads value + delta in 40-digit arithmetic (delta far below float64 resolution): float(a[i]) of every
    other entry is unchanged, the perturbed one returns an mpf through __float__-free access in _mp_latent's f()"""

    def __init__(self, a, idx, delta):
        self.a, self.idx, self.delta, self.shape = np.asarray(a), tuple(idx), delta, np.asarray(a).shape

    def __getitem__(self, i):
        if self.a.ndim == 1:
            return _MpScalar(mp.mpf(float(self.a[i])) + (self.delta if (i,) == self.idx else 0))
        return _Row(self, i)

    def __len__(self):
        return self.shape[0]

    def __iter__(self):
        return (self[i] for i in range(self.shape[0]))


class _Row:
    def __init__(self, parent, i):
        self.p, self.i = parent, i

    def __getitem__(self, d):
        return _MpScalar(mp.mpf(float(self.p.a[self.i, d])) + (self.p.delta if (self.i, d) == self.p.idx else 0))

    def __len__(self):
        return self.p.shape[1]


class _MpScalar:
    def __init__(self, v):
        self.v = v


@pytest.mark.parametrize('grid,rows', [((32, 32), 1000), ((10, 100), 777), ((40, 9), 500)])
def test_kron_f_mu_offset_value_gradient_and_predict(engine, grid, rows):
    """build_predict's optional f_mu (scripts/onoff.py:161,168-169; onofftf/onoffpred.py:127,135-136) on the on/off Kronecker path:
    fused small grid, larger grid, panel path; and on rows of the resident data set."""
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    from test_gpu_kron import make_kron_problem
    X, Y, p = make_kron_problem(rows, grid[0], grid[1], seed=31)
    fmu = 0.37
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=1e-5, scale=2.0, f_mu=fmu)
    e_r, d_r, kl_r, g_r = ot.kron_elbo_and_grad(X, Y, p, 1e-5, scale=2.0, f_mu=fmu)
    assert abs(ed - 2.0 * d_r) <= 1e-7 * abs(2.0 * d_r) and abs(kl - kl_r) <= 1e-7 * abs(kl_r)
    assert abs(g['f_mu'] - g_r['f_mu']) <= 1e-6 * abs(g_r['f_mu']), (g['f_mu'], g_r['f_mu'])
    assert relerr(g['u_fm'], g_r['u_fm'].reshape(-1)) < 1e-6 and relerr(g['Zf'][0], g_r['Zf'][0]) < 1e-6
    ed0, _, g0 = engine.kron_elbo(p, X, Y, jitter=1e-5, scale=2.0)
    assert 'f_mu' not in g0 and abs(ed0 - ed) > 1e-6 * abs(ed)                 # the offset matters; without it no extra gradient entry
    out = engine.kron_predict(p, X, jitter=1e-5, g_offset=-1.0, f_mu=fmu)
    out0 = engine.kron_predict(p, X, jitter=1e-5, g_offset=-1.0)
    ref = o.kron_build_predict(X, p, 1e-5, -1.0, f_mu=fmu)
    assert np.max(np.abs(out[3] - out0[3] - fmu)) < 1e-12 and np.array_equal(out[4:], out0[4:])      # fmean shifted, f's variance and g untouched
    for i in range(9):       # (the op-order floor of these synthetic factors is covered in test_gpu_kron.py; here: the offset reaches every output)
        assert relerr(out[i], ref[i].reshape(-1)) < 5e-6, NAMES[i]
    engine.set_data(X, Y)
    b = engine.kron_elbo(p, rows=(0, rows), jitter=1e-5, scale=2.0, f_mu=fmu)
    assert b[0] == ed and b[2]['f_mu'] == g['f_mu']


def test_pivot_rtol_zero_gives_the_bare_positive_pivot_test(engine):
    """ZIGP_ENOTPD by default means pivot <= 8 eps (variance + jitter); zigp_set_pivot_rtol(0) is the reference's test (tf.cholesky /
    LAPACK: fail on a NON-POSITIVE pivot only).  A Kuu with a pivot of a few eps passes only under the latter."""
    import zigp
    from conftest import make_problem
    X, Y, p = make_problem(600, 24, 2, seed=5)
    bad = dict(p, Zf=p['Zf'].copy())
    bad['Zf'][7] = bad['Zf'][3] + 1e-9          # two inducing points 1e-9 apart, jitter 0: the pivot is ~1e-17 * var, positive or not by rounding
    engine.set_data(X, Y)
    with pytest.raises(zigp.NotPositiveDefiniteError):
        engine.elbo(bad, jitter=0.0, need_grad=False)
    assert engine.lib.zigp_last_info(engine.ctx) == 8        # 1-based pivot index
    close = dict(p, Zf=p['Zf'].copy())
    close['Zf'][7] = close['Zf'][3] + 3e-8      # pivot ~ 2 * (3e-8 / ell)^2 ~ 1e-14 var: above 8 eps, fine either way
    engine.set_data(X, Y)
    a = engine.elbo(close, jitter=0.0, need_grad=False)
    engine.set_pivot_rtol(0.0)
    try:
        b = engine.elbo(close, jitter=0.0, need_grad=False)
        assert a[0] == b[0] and a[1] == b[1]
        try:                                     # exactly duplicated points: pivot = rounding noise; with rtol 0 it passes iff it rounded positive
            r = engine.elbo(dict(p, Zf=np.vstack([p['Zf'][:-1], p['Zf'][:1]])), jitter=0.0, need_grad=False)
            assert not np.isfinite(r[0]) or abs(r[0]) > 0
        except zigp.NotPositiveDefiniteError:
            pass
    finally:
        engine.set_pivot_rtol(8.0)
    with pytest.raises(ValueError):
        engine.set_pivot_rtol(-1.0)
