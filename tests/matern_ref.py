"""Matern 3/2 and 5/2 kernels for either latent of the dense model, restated on the CPU -- TEST INFRASTRUCTURE ONLY (like whiten_ref.py).

The kernels follow GPflow 0.4.0 (gpflow/kernels.py Stationary / Matern32 / Matern52), which the reference model is handed as "gpflow
objects for function & gamma kernels" (onoffgpf/OnOffSVGP.py:22):
    r2 = sum_d ((x_d - z_d) / ell_d)^2            Stationary.square_dist
    r  = sqrt(r2 + 1e-12)                         Stationary.euclid_dist (the floor keeps coincident points differentiable)
    Matern32   k = var (1 + sqrt3 r) exp(-sqrt3 r)
    Matern52   k = var (1 + sqrt5 r + (5/3) r^2) exp(-sqrt5 r)        with r^2 the square of the floored r
    Kdiag = var exactly; the diagonal of K(Z, Z) is the formula at r = 1e-6 (K(X) goes through euclid_dist as well).
The derivative factor of the reverse pass, K' = -dk / d(r2 / 2) (K' = K for the RBF kernel):
    Matern32   K' = 3 var exp(-sqrt3 r)           Matern52   K' = (5/3) var (1 + sqrt5 r) exp(-sqrt5 r)
GPflow is not installable next to this project, so these formulas are restated from its source as recalled, not run against it: PARITY
UNPINNED in the sense of DESIGN.md section 1 (as oracle/zigp_oracle.py says of the whole model).

In torch float64, so that gradients come from autograd as the reference gets them from tf.gradients.  r2 is formed from direct
differences (not from |x|^2 + |z|^2 - 2 x.z as KernSE does, onofftf/main.py:41-57): next to the 1e-12 floor the cancellation of that form
(1e-16 |x / ell|^2) would decide what a coincident pair evaluates to.  The conditional and the KL of the three parametrisations are
restated around a kernel argument from the same lines as oracle/zigp_oracle_torch.py (diagonal, unwhitened), whiten_ref.py (whitened) and
fullcov_ref.py (whitened, full covariance); the KLs, the probit moments and the likelihood are taken from those files as they are.
"""
import math

import numpy as np
import torch

import zigp_oracle_torch as ot
import whiten_ref as wr
import fullcov_ref as fr
from zigp_oracle_torch import DT, _t, probit_expectations, variational_expectations, PARAM_KEYS, MEAN_KEYS  # noqa: F401

KINDS = ('rbf', 'matern32', 'matern52')
FLOOR = 1e-12


def square_dist(X, X2, ell):
    """(n1, n2) scaled squared distances from direct differences; X2 None: X"""
    A = X / ell
    B = A if X2 is None else X2 / ell
    return torch.sum(torch.square(A[:, None, :] - B[None, :, :]), 2)


def k_of_r2(kind, r2, var):
    """the kernel as a function of the scaled squared distance"""
    if kind == 'rbf':
        return var * torch.exp(-r2 / 2)
    r = torch.sqrt(r2 + FLOOR)
    if kind == 'matern32':
        return var * (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    if kind == 'matern52':
        return var * (1.0 + math.sqrt(5.0) * r + 5.0 / 3.0 * torch.square(r)) * torch.exp(-math.sqrt(5.0) * r)
    raise ValueError(kind)


def kd_of_r2(kind, r2, var):
    """K' = -dk / d(r2 / 2), closed form"""
    if kind == 'rbf':
        return var * torch.exp(-r2 / 2)
    r = torch.sqrt(r2 + FLOOR)
    if kind == 'matern32':
        return 3.0 * var * torch.exp(-math.sqrt(3.0) * r)
    if kind == 'matern52':
        return 5.0 / 3.0 * var * (1.0 + math.sqrt(5.0) * r) * torch.exp(-math.sqrt(5.0) * r)
    raise ValueError(kind)


def kern_K(kind, X, X2, ell, var):
    return k_of_r2(kind, square_dist(X, X2, ell), var)


def kern_K_np(kind, X, X2, ell, var):
    with torch.no_grad():
        return kern_K(kind, _t(X), None if X2 is None else _t(X2), _t(np.broadcast_to(ell, (np.shape(X)[1],)).copy()), float(var)).numpy()


def mode_of(p):
    """'diag', 'white' or 'white_full' from p['whiten'] / p['q_diag'], as DenseEngine reads them"""
    if not p.get('whiten', False):
        return 'diag'
    return 'white' if p.get('q_diag', True) else 'white_full'


def conditional(kind, mode, Xnew, Z, ell, var, q_mu, q_sqrt, jitter):
    """onofftf/main.py:257-305 around kern.K: the unwhitened diagonal branch (zigp_oracle_torch.conditional), whiten=True with a
    diagonal q_sqrt (whiten_ref.conditional_white) or with a 3-d q_sqrt (fullcov_ref.conditional_white_full)."""
    M = Z.shape[0]
    Kmn = kern_K(kind, Z, Xnew, ell, var)
    Kmm = kern_K(kind, Z, None, ell, var) + torch.eye(M, dtype=DT) * jitter
    Lm = torch.linalg.cholesky(Kmm)
    A = torch.linalg.solve_triangular(Lm, Kmn, upper=False)
    fvar = var - torch.sum(torch.square(A), 0)                                    # :278 (Kdiag = var)
    if mode == 'diag':
        A = torch.linalg.solve_triangular(Lm.t(), A, upper=True)                  # :284
    fmean = torch.matmul(A.t(), q_mu.reshape(M, 1))                               # :287
    if mode == 'white_full':
        fvar = fvar + torch.sum(torch.square(torch.matmul(fr._lq(q_sqrt, M).t(), A)), 0)      # :293-295,302
    else:
        fvar = fvar + torch.sum(torch.square(A * q_sqrt.reshape(M, 1)), 0)        # :291,302
    return fmean.reshape(-1, 1), fvar.reshape(-1, 1)


def latents(X, p, kinds, mode, jitter, g_offset=0.0):
    """(fmean, fvar, gmean, gvar) of build_predict (onoffgpf/OnOffSVGP.py:124-142)"""
    fmean, fvar = conditional(kinds[0], mode, X, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter)
    if 'mean_a' in p:                                                             # fmean + self.mean_function(Xnew), :134
        fmean = fmean + torch.matmul(X, p['mean_a'].reshape(-1, 1))
    if 'mean_b' in p:
        fmean = fmean + p['mean_b']
    gmean, gvar = conditional(kinds[1], mode, X, p['Zg'], p['ell_g'], p['var_g'], p['u_gm'], p['u_gs_sqrt'], jitter)
    return fmean, fvar, gmean + g_offset, gvar


def data_term(X, Y, p, kinds, mode, jitter, g_offset=0.0):
    fmean, fvar, gmean, gvar = latents(X, p, kinds, mode, jitter, g_offset)
    e1, e2, ev = probit_expectations(gmean, gvar)
    return torch.sum(variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), Y.reshape(-1, 1), p['noise']))


def latent_kl(kind, mode, Z, ell, var, q_mu, q_sqrt, jitter):
    if mode == 'white':
        return wr.gauss_kl_white_diag(q_mu, q_sqrt)
    if mode == 'white_full':
        return fr.gauss_kl_white_full(q_mu, q_sqrt)
    K = kern_K(kind, Z, None, ell, var) + torch.eye(Z.shape[0], dtype=DT) * jitter          # onoffgpf/OnOffSVGP.py:96-101
    return ot.gauss_kl_diag(q_mu, q_sqrt, K)


def prior_kl2(p, kinds, mode, jitter):
    return [latent_kl(kinds[h], mode, p['Z' + t], p['ell_' + t], p['var_' + t], p['u_%sm' % t], p['u_%ss_sqrt' % t], jitter)
            for h, t in enumerate('fg')]


def kinds_of(p):
    return (p.get('kern_f', 'rbf'), p.get('kern_g', 'rbf'))


_NOT_PARAMS = ('whiten', 'q_diag', 'kern_f', 'kern_g')


def _tensors(p_np):
    return {k: _t(p_np[k]) for k in PARAM_KEYS + tuple(k for k in MEAN_KEYS if p_np.get(k) is not None)}


def build_predict(X, p_np, jitter, g_offset=0.0):
    """The 9 rows of OnOffSVGP.build_predict (:152) as a (9, N) NumPy array; kernels and parametrisation from p_np as the engine reads them."""
    with torch.no_grad():
        fmean, fvar, gmean, gvar = latents(_t(X), _tensors(p_np), kinds_of(p_np), mode_of(p_np), jitter, g_offset)
        e1, e2, ev = probit_expectations(gmean, gvar)
        rows = (e1 * fmean, e2 * fvar, ev * torch.square(fmean), fmean, fvar, gmean, gvar, e1, ev)
        return np.stack([r.reshape(-1).numpy() for r in rows])


def elbo_and_grad(X, Y, p_np, jitter, scale=1.0, g_offset=0.0, chunk=20000, include_kl=True, need_grad=True):
    """As zigp_oracle_torch.elbo_and_grad: (elbo, data, kl, grads dict of numpy), rows in chunks (the data term is a sum over points)."""
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    kinds, mode = kinds_of(p_np), mode_of(p_np)
    p = ot.make_leaves({k: v for k, v in p_np.items() if k not in _NOT_PARAMS})
    data = 0.0
    for s in range(0, Xt.shape[0], chunk):
        with torch.set_grad_enabled(need_grad):
            d = data_term(Xt[s:s + chunk], Yt[s:s + chunk], p, kinds, mode, jitter, g_offset)
        if need_grad:
            (d * scale).backward()
        data += float(d.detach())
    kl = 0.0
    if include_kl:
        with torch.set_grad_enabled(need_grad):
            k = sum(prior_kl2(p, kinds, mode, jitter))
        if need_grad:
            (-k).backward()
        kl = float(k.detach())
    grads = {k: (p[k].grad.numpy().copy() if p[k].grad is not None else np.zeros(tuple(p[k].shape))) for k in p} if need_grad else None
    return data * scale - kl, data, kl, grads


def kuu_cond(p_np, jitter=1e-6):
    """cond(Kuu + jitter I) of latent f, the number the parity bounds scale with"""
    K = kern_K_np(kinds_of(p_np)[0], p_np['Zf'], None, p_np['ell_f'], p_np['var_f']) + jitter * np.eye(np.shape(p_np['Zf'])[0])
    return float(np.linalg.cond(K))


def problem(N, Mf, Mg, D, ell=None, seed=None):
    """The parity fixtures of tests/test_gpu_matern.py (and of the positive-definiteness check in test_cpu_matern.py): conftest.make_problem
    with the inducing inputs TAKEN FROM THE DATA ROWS -- Zf the first Mf rows, Zg the last Mg -- so that the Kuf panels hold pairs at
    r2 = 0 exactly; D = 1 is stretched to [0, 10] with lengthscale 2 and has u of size 0.01 (the dense 1-D case of tests/test_gpu_dense.py
    and tests/test_gpu_whiten.py: Kuu is as ill-conditioned as the jitter lets it be there)."""
    from conftest import make_problem
    ell = {1: 2.0}.get(D, 0.3 + 0.075 * D) if ell is None else ell
    X, Y, p = make_problem(N, Mf, D, seed=N + Mf if seed is None else seed, Mg=Mg, ell=ell, u_scale=0.01 if D == 1 else 0.5)
    if D == 1:
        X = X * 10.0
    p['Zf'], p['Zg'] = X[:Mf].copy(), X[N - Mg:].copy()
    return X, Y, p


# ---- the panel formulas in extended precision (numpy.longdouble: 64-bit mantissa on x86-64), for the stage test ----
def panel_formula(kind, X, Z, ell, var, dtype):
    """(K, K') (M, N) of kern.K(Z, X) in `dtype` arithmetic (np.float64: the plain NumPy formula; np.longdouble: the yardstick)"""
    X, Z, ell = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype), np.asarray(ell, dtype=dtype)
    var = dtype(var)
    d = (Z[:, None, :] - X[None, :, :]) / ell
    r2 = np.sum(d * d, axis=2)
    r = np.sqrt(r2 + dtype(FLOOR))
    if kind == 'matern32':
        a = np.sqrt(dtype(3.0))
        e = np.exp(-a * r)
        return var * (dtype(1.0) + a * r) * e, dtype(3.0) * var * e
    a = np.sqrt(dtype(5.0))
    e = np.exp(-a * r)
    return var * (dtype(1.0) + a * r + dtype(5.0) / dtype(3.0) * r * r) * e, dtype(5.0) / dtype(3.0) * var * (dtype(1.0) + a * r) * e
