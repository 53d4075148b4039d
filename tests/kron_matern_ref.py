"""The Kronecker (space x time) model and its heads with a kernel kind PER FACTOR, restated on the CPU -- TEST INFRASTRUCTURE ONLY.

oracle/zigp_oracle_torch.py states kron_inf, gauss_kl_kron, kron_elbo_and_grad and kron_head_elbo_and_grad in the reference's literal
(dense) op order for RBF factors.  This file restates the same lines around a kernel argument per factor, as matern_ref.py does for the
dense model: an RBF factor goes through the oracle's own rbf_K (so with every kind 'rbf' each function below returns the oracle's bits),
a Matern factor through matern_ref.kern_K (GPflow 0.4.0's Stationary / Matern32 / Matern52: direct differences, r = sqrt(r2 + 1e-12),
the diagonal of K(Z, Z) at r = 1e-6).  Knn = var0 var1 for every kind (Kdiag = var).  Gradients come from autograd.

Kinds of a parameter dict, as DenseEngine reads them: p.get('kern_f', 'rbf') / p.get('kern_g', 'rbf'), each a name (both factors) or a pair
(kind0, kind1).  PARITY UNPINNED in the sense of DESIGN.md section 1, like matern_ref.py."""
import numpy as np
import torch

import zigp_oracle_torch as ot
import matern_ref as mr
from zigp_oracle_torch import DT, _t, probit_expectations, variational_expectations, KRON_KEYS, KRON_VEC_KEYS, HEAD_KEYS

KINDS = mr.KINDS
PAIRS = tuple((a, b) for a in KINDS for b in KINDS)      # the nine (kind0, kind1) of a latent
RBF2 = ('rbf', 'rbf')


def pair_of(v):
    return (v, v) if isinstance(v, str) else (v[0], v[1])


def kinds_of(p):
    """((kind0, kind1) of f, (kind0, kind1) of g)"""
    return pair_of(p.get('kern_f', 'rbf')), pair_of(p.get('kern_g', 'rbf'))


def with_kinds(p, kf, kg=None):
    """a copy of the parameter dict p (arrays shared, read-only) with the factor kinds kf of f and kg of g"""
    q = dict(p)
    q['kern_f'] = kf
    if kg is not None:
        q['kern_g'] = kg
    return q


def factor_K(kind, X, X2, ell, var):
    """kern.K of one factor: the oracle's expanded-square RBF (onofftf/main.py:41-57) or matern_ref's direct-difference Matern"""
    if kind == 'rbf':
        return ot.rbf_K(X, X2, ell, var)
    return mr.kern_K(kind, X, X2, ell, var)


def kron_inf(Xnew, Z_list, ell_list, var_list, q_mu, q_sqrt, jitter, kinds=RBF2):
    """scripts/onoff.py:186-213, literal (dense) op order: zigp_oracle_torch.kron_inf around factor_K"""
    Kmm = [factor_K(k, Z, None, l, v) + torch.eye(Z.shape[0], dtype=DT) * jitter for k, Z, l, v in zip(kinds, Z_list, ell_list, var_list)]
    Kinv = [torch.linalg.inv(K) for K in Kmm]
    alpha = ot.kron_mv(Kinv, q_mu)
    Nb = Xnew.shape[0]
    Knn = torch.ones((Nb, 1), dtype=DT)
    Kmn_kron, c0 = [], 0
    for k, Z, l, v in zip(kinds, Z_list, ell_list, var_list):
        xnew = Xnew[:, c0:c0 + Z.shape[1]]
        c0 += Z.shape[1]
        Knn = Knn * v
        Kmn_kron.append(factor_K(k, Z, xnew, l, v))
    S = torch.diag(torch.square(q_sqrt).reshape(-1))
    Kmn = (Kmn_kron[0][:, None, :] * Kmn_kron[1][None, :, :]).reshape(-1, Nb)
    A = torch.matmul(ot.np_kron(*Kinv), Kmn)
    mu = torch.matmul(Kmn.t(), alpha)
    var = Knn - torch.diagonal(torch.matmul(Kmn.t(), A) - torch.matmul(torch.matmul(A.t(), S), A)).reshape(-1, 1)
    return mu, var


def factor_Kmm(kinds, Z_list, ell_list, var_list, jitter):
    return [factor_K(k, Z, None, l, v) + torch.eye(Z.shape[0], dtype=DT) * jitter for k, Z, l, v in zip(kinds, Z_list, ell_list, var_list)]


gauss_kl_kron = ot.gauss_kl_kron      # onofftf/main.py:350-387: kernel-free, it takes the factor matrices


def kron_elbo_and_grad(X, Y, p_np, jitter, scale=1.0, g_offset=0.0, include_kl=True, need_grad=True, f_mu=None):
    """zigp_oracle_torch.kron_elbo_and_grad with the factor kinds of p_np: (elbo, data, kl, grads)"""
    kf, kg = kinds_of(p_np)
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    p = {}
    for k in KRON_KEYS:
        p[k] = [_t(v).clone().requires_grad_(need_grad) for v in p_np[k]]
    for k in KRON_VEC_KEYS:
        p[k] = _t(p_np[k]).clone().requires_grad_(need_grad)
    fmu = None if f_mu is None else _t(f_mu).clone().requires_grad_(need_grad)
    with torch.set_grad_enabled(need_grad):
        fmean, fvar = kron_inf(Xt, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter, kf)
        if fmu is not None:
            fmean = fmean + fmu
        gmean, gvar = kron_inf(Xt, p['Zg'], p['ell_g'], p['var_g'], p['u_gm'], p['u_gs_sqrt'], jitter, kg)
        gmean = gmean + g_offset
        e1, e2, ev = probit_expectations(gmean, gvar)
        data = torch.sum(variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), Yt, p['noise']))
        kl = torch.zeros((), dtype=DT)
        if include_kl:
            Kf = factor_Kmm(kf, p['Zf'], p['ell_f'], p['var_f'], jitter)
            Kg = factor_Kmm(kg, p['Zg'], p['ell_g'], p['var_g'], jitter)
            kl = gauss_kl_kron(p['u_fm'], p['u_fs_sqrt'], Kf) + gauss_kl_kron(p['u_gm'], p['u_gs_sqrt'], Kg)
        elbo = data * scale - kl
    grads = None
    if need_grad:
        elbo.backward()
        grads = {}
        for k in KRON_KEYS:
            grads[k] = [v.grad.numpy().copy() for v in p[k]]
        for k in KRON_VEC_KEYS:
            grads[k] = p[k].grad.numpy().copy()
        if fmu is not None:
            grads['f_mu'] = float(fmu.grad)
    return float(elbo.detach()), float(data.detach()), float(kl.detach()), grads


def kron_head_elbo_and_grad(X, Y, p_np, lik, jitter, scale=1.0, f_mu=0.0, include_kl=True, need_grad=True):
    """zigp_oracle_torch.kron_head_elbo_and_grad with the f kinds of p_np"""
    kf = kinds_of(p_np)[0]
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    p = {k: [_t(v).clone().requires_grad_(need_grad) for v in p_np[k]] for k in HEAD_KEYS}
    for k in ('u_fm', 'u_fs_sqrt'):
        p[k] = _t(p_np[k]).clone().requires_grad_(need_grad)
    p['noise'] = _t(p_np.get('noise', 1.0)).clone().requires_grad_(need_grad)
    p['f_mu'] = _t(f_mu).clone().requires_grad_(need_grad)
    with torch.set_grad_enabled(need_grad):
        fmean, fvar = kron_inf(Xt, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter, kf)
        fmean = fmean + p['f_mu']
        if lik == 'gaussian':
            ve = -0.5 * np.log(2 * np.pi) - 0.5 * torch.log(p['noise']) - 0.5 * (torch.square(Yt - fmean) + fvar) / p['noise']
        else:
            pr = 0.5 * (1.0 + torch.erf(fmean / torch.sqrt(1 + fvar) / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
            ve = torch.log(torch.where(Yt == 1, pr, 1 - pr))
        data = torch.sum(ve)
        kl = torch.zeros((), dtype=DT)
        if include_kl:
            kl = gauss_kl_kron(p['u_fm'], p['u_fs_sqrt'], factor_Kmm(kf, p['Zf'], p['ell_f'], p['var_f'], jitter))
        elbo = data * scale - kl
    grads = None
    if need_grad:
        elbo.backward()
        grads = {k: [v.grad.numpy().copy() for v in p[k]] for k in HEAD_KEYS}
        for k in ('u_fm', 'u_fs_sqrt', 'noise', 'f_mu'):
            grads[k] = p[k].grad.numpy().copy() if p[k].grad is not None else np.zeros(tuple(p[k].shape))
    return float(elbo.detach()), float(data.detach()), float(kl.detach()), grads


def _lists(p_np, tag):
    return [_t(v) for v in p_np['Z' + tag]], [_t(v) for v in p_np['ell_' + tag]], [_t(v) for v in p_np['var_' + tag]]


def kron_build_predict(X, p_np, jitter, g_offset=0.0, f_mu=None):
    """The 9 rows of build_predict (scripts/onoff.py:161-184) as a (9, N) array"""
    kf, kg = kinds_of(p_np)
    with torch.no_grad():
        Xt = _t(X)
        Z, l, v = _lists(p_np, 'f')
        fmean, fvar = kron_inf(Xt, Z, l, v, _t(p_np['u_fm']), _t(p_np['u_fs_sqrt']), jitter, kf)
        if f_mu is not None:
            fmean = fmean + float(f_mu)
        Z, l, v = _lists(p_np, 'g')
        gmean, gvar = kron_inf(Xt, Z, l, v, _t(p_np['u_gm']), _t(p_np['u_gs_sqrt']), jitter, kg)
        gmean = gmean + g_offset
        e1, e2, ev = probit_expectations(gmean, gvar)
        rows = (e1 * fmean, e2 * fvar, ev * torch.square(fmean), fmean, fvar, gmean, gvar, e1, ev)
        return np.stack([r.reshape(-1).numpy() for r in rows])


def kron_head_predict(X, p_np, lik, jitter, f_mu=0.0):
    """(4, N): fmean, fvar, pfmean, pfvar as zigp_kron_head_predict orders them"""
    kf = kinds_of(p_np)[0]
    with torch.no_grad():
        Z, l, v = _lists(p_np, 'f')
        fmean, fvar = kron_inf(_t(X), Z, l, v, _t(p_np['u_fm']), _t(p_np['u_fs_sqrt']), jitter, kf)
        fmean = fmean + float(f_mu)
        if lik == 'gaussian':
            pm, pv = fmean, fvar + float(np.squeeze(p_np['noise']))
        else:
            pm = 0.5 * (1.0 + torch.erf(fmean / torch.sqrt(1 + fvar) / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
            pv = pm - torch.square(pm)
        return np.stack([r.reshape(-1).numpy() for r in (fmean, fvar, pm, pv)])


# ---- what the reference alone does on a fixture: op-order floor and conditioning, as kron_nd.fixture_floor_and_cond measures them ----
def factor_K_np(kind, X, X2, ell, var):
    with torch.no_grad():
        return factor_K(kind, _t(X), None if X2 is None else _t(X2), _t(ell), float(np.squeeze(var))).numpy()


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def factored(X, p, tag, jit):
    """(mean, var) of one latent by the FACTORED identities the engine evaluates, in float64 with np.linalg.inv"""
    kinds = kinds_of(p)['fg'.index(tag)]
    Z, ell, var = p['Z' + tag], p['ell_' + tag], [float(np.squeeze(v)) for v in p['var_' + tag]]
    P = [np.linalg.inv(factor_K_np(kinds[q], Z[q], None, ell[q], var[q]) + jit * np.eye(Z[q].shape[0])) for q in range(2)]
    d0 = Z[0].shape[1]
    k0, k1 = factor_K_np(kinds[0], Z[0], X[:, :d0], ell[0], var[0]), factor_K_np(kinds[1], Z[1], X[:, d0:], ell[1], var[1])
    M0, M1 = Z[0].shape[0], Z[1].shape[0]
    U, S2 = np.asarray(p['u_%sm' % tag]).reshape(M0, M1), np.square(p['u_%ss_sqrt' % tag]).reshape(M0, M1)
    a0, a1 = P[0] @ k0, P[1] @ k1
    mu = np.einsum('in,ij,jn->n', k0, P[0] @ U @ P[1], k1)
    vv = var[0] * var[1] - (k0 * a0).sum(0) * (k1 * a1).sum(0) + np.einsum('in,ij,jn->n', a0 ** 2, S2, a1 ** 2)
    return mu, vv


def fixture_floor_and_cond(X, p, jit):
    """(op-order floor, {kind: max cond(K_p + jitter I)}) of a fixture with the factor kinds of p"""
    ref = kron_build_predict(X, p, jit, 0.0)
    floor, cond = 0.0, {}
    for tag, (im, iv) in (('f', (3, 4)), ('g', (5, 6))):
        mu, vv = factored(X, p, tag, jit)
        floor = max(floor, _relerr(mu, ref[im]), _relerr(vv, ref[iv]))
        kinds = kinds_of(p)['fg'.index(tag)]
        for q in range(2):
            Z = p['Z' + tag][q]
            K = factor_K_np(kinds[q], Z, None, p['ell_' + tag][q], p['var_' + tag][q]) + jit * np.eye(Z.shape[0])
            cond[kinds[q]] = max(cond.get(kinds[q], 0.0), float(np.linalg.cond(K)))
    return floor, cond


# ---- the fixtures: cases of kron_nd.CASES with kinds cycling through the mixed combinations.  Every one of the nine (kind0, kind1)
# pairs stands on at least one latent; f differs from g on six cases. ----
FIXTURES = {
    'd11': (('matern32', 'matern52'), ('rbf', 'matern32')),
    'd21-12': (('rbf', 'matern32'), ('matern52', 'rbf')),
    'd21-mix': (('matern52', 'matern52'), ('matern32', 'rbf')),
    'd31': (('matern32', 'matern32'), ('matern32', 'matern32')),
    'd17': (('rbf', 'matern52'), ('matern52', 'matern32')),
    'p88': (('matern52', 'rbf'), ('rbf', 'rbf')),
    'p43': (('matern32', 'rbf'), ('matern32', 'matern52')),
    'L32': (('matern52', 'matern32'), ('matern52', 'matern32')),
}


def fixture(name):
    """(X, Y, p) of kron_nd.problem(name) with the fixture's kinds in p (arrays shared with kron_nd's cache, read-only)"""
    import kron_nd
    X, Y, p = kron_nd.problem(name)
    kf, kg = FIXTURES[name]
    return X, Y, with_kinds(p, kf, kg)
