"""Whitened variational parametrisation, restated on the CPU -- TEST INFRASTRUCTURE ONLY (like dense_fit_ref.py).

GPConditional(..., whiten=True) (onofftf/main.py:257-305: the second back-substitution of :282-284 is skipped) and the white GaussKL
(q_mu, q_sqrt, K=None: :193-195,227-228,246) in the reference's op order, in torch float64 so that gradients come from autograd as the
reference gets them from tf.gradients.  Everything the two parametrisations share -- the kernel, the probit moments, the likelihood
-- is taken from oracle/zigp_oracle_torch.py; OnOffSVGP.build_predict / build_likelihood (onoffgpf/OnOffSVGP.py:107-152) are restated
around them with whiten=True passed through (:133,137) and gauss_kl_white_diag as the prior KL (:88-91).

q(u) = N(L u_m, L diag(u_s_sqrt^2) L^T) with L = chol(Kuu + jitter I): `explicit_full_cov` evaluates the same model through that
definition (dense mean and covariance, textbook conditional, dense Gaussian KL) and pins this file in tests/test_cpu_whiten_ref.py.
"""
import numpy as np
import torch

import zigp_oracle_torch as ot
from zigp_oracle_torch import DT, _t, rbf_K, probit_expectations, variational_expectations, PARAM_KEYS, MEAN_KEYS  # noqa: F401


def conditional_white(Xnew, Z, ell, var, q_mu, q_sqrt, jitter):
    """onofftf/main.py:257-305 with whiten=True, diag q."""
    M = Z.shape[0]
    Kmn = rbf_K(Z, Xnew, ell, var)
    Kmm = rbf_K(Z, None, ell, var) + torch.eye(M, dtype=DT) * jitter
    Lm = torch.linalg.cholesky(Kmm)
    A = torch.linalg.solve_triangular(Lm, Kmn, upper=False)
    fvar = var - torch.sum(torch.square(A), 0)                                    # :278
    fmean = torch.matmul(A.t(), q_mu.reshape(M, 1))                               # :287 (no :284)
    fvar = fvar + torch.sum(torch.square(A * q_sqrt.reshape(M, 1)), 0)            # :291,302
    return fmean.reshape(-1, 1), fvar.reshape(-1, 1)


def gauss_kl_white_diag(q_mu, q_sqrt):
    """onofftf/main.py:187-252 with K=None, diag branch."""
    M = q_mu.numel()
    q_mu, q_sqrt = q_mu.reshape(M, 1), q_sqrt.reshape(M, 1)
    twoKL = torch.sum(torch.square(q_mu)) - float(M) - torch.sum(torch.log(torch.square(q_sqrt))) + torch.sum(torch.square(q_sqrt))
    return 0.5 * twoKL


def latents(X, p, jitter, g_offset=0.0):
    """(fmean, fvar, gmean, gvar) of build_predict (onoffgpf/OnOffSVGP.py:124-142) with whiten=True."""
    fmean, fvar = conditional_white(X, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter)
    if 'mean_a' in p:                                                             # fmean + self.mean_function(Xnew), :134
        fmean = fmean + torch.matmul(X, p['mean_a'].reshape(-1, 1))
    if 'mean_b' in p:
        fmean = fmean + p['mean_b']
    gmean, gvar = conditional_white(X, p['Zg'], p['ell_g'], p['var_g'], p['u_gm'], p['u_gs_sqrt'], jitter)
    return fmean, fvar, gmean + g_offset, gvar


def data_term(X, Y, p, jitter, g_offset=0.0):
    fmean, fvar, gmean, gvar = latents(X, p, jitter, g_offset)
    e1, e2, ev = probit_expectations(gmean, gvar)
    return torch.sum(variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), Y.reshape(-1, 1), p['noise']))


def prior_kl(p):
    return gauss_kl_white_diag(p['u_fm'], p['u_fs_sqrt']) + gauss_kl_white_diag(p['u_gm'], p['u_gs_sqrt'])


def _tensors(p_np):
    return {k: _t(p_np[k]) for k in PARAM_KEYS + tuple(k for k in MEAN_KEYS if p_np.get(k) is not None)}


def build_predict(X, p_np, jitter, g_offset=0.0):
    """The 9 rows of OnOffSVGP.build_predict (:152) as a (9, N) NumPy array."""
    with torch.no_grad():
        fmean, fvar, gmean, gvar = latents(_t(X), _tensors(p_np), jitter, g_offset)
        e1, e2, ev = probit_expectations(gmean, gvar)
        rows = (e1 * fmean, e2 * fvar, ev * torch.square(fmean), fmean, fvar, gmean, gvar, e1, ev)
        return np.stack([r.reshape(-1).numpy() for r in rows])


def elbo_and_grad(X, Y, p_np, jitter, scale=1.0, g_offset=0.0, chunk=20000, include_kl=True, need_grad=True):
    """As zigp_oracle_torch.elbo_and_grad: (elbo, data, kl, grads dict of numpy), rows in chunks (the data term is a sum over points)."""
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    p = ot.make_leaves({k: v for k, v in p_np.items() if k != 'whiten'})
    data = 0.0
    for s in range(0, Xt.shape[0], chunk):
        with torch.set_grad_enabled(need_grad):
            d = data_term(Xt[s:s + chunk], Yt[s:s + chunk], p, jitter, g_offset)
        if need_grad:
            (d * scale).backward()
        data += float(d.detach())
    kl = 0.0
    if include_kl:
        with torch.set_grad_enabled(need_grad):
            k = prior_kl(p)
        if need_grad:
            (-k).backward()
        kl = float(k.detach())
    grads = {k: (p[k].grad.numpy().copy() if p[k].grad is not None else np.zeros(tuple(p[k].shape))) for k in p} if need_grad else None
    return data * scale - kl, data, kl, grads


def explicit_full_cov(X, p_np, jitter, g_offset=0.0):
    """The same model through its definition: m = L u, S = L diag(s^2) L^T, then the UNWHITENED full-covariance formulas
    mean = Kfu Kuu^-1 m, var = k** - diag(Kfu Kuu^-1 Kuf) + diag(Kfu Kuu^-1 S Kuu^-1 Kuf), KL(N(m, S) || N(0, Kuu)) with dense matrices.
    Returns ((fmean, fvar, gmean, gvar) as NumPy vectors, kl)."""
    p = _tensors(p_np)
    Xt = _t(X)
    out, kl = [], 0.0
    for tag, off in (('f', 0.0), ('g', g_offset)):
        Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
        M = Z.shape[0]
        u, s = p['u_%sm' % tag].reshape(M, 1), p['u_%ss_sqrt' % tag].reshape(M)
        Kuu = rbf_K(Z, None, ell, var) + torch.eye(M, dtype=DT) * jitter
        L = torch.linalg.cholesky(Kuu)
        m, S = L @ u, L @ torch.diag(s * s) @ L.t()
        Kinv = torch.linalg.inv(Kuu)
        B = Kinv @ rbf_K(Z, Xt, ell, var)                  # Kuu^-1 Kuf
        mean = (B.t() @ m).reshape(-1)
        if tag == 'f':
            if 'mean_a' in p:
                mean = mean + (Xt @ p['mean_a'].reshape(-1, 1)).reshape(-1)
            if 'mean_b' in p:
                mean = mean + p['mean_b'].reshape(-1)
        Kuf = rbf_K(Z, Xt, ell, var)
        v = var - torch.sum(Kuf * B, 0) + torch.sum(B * (S @ B), 0)
        out += [(mean + off).numpy(), v.numpy()]
        kl += 0.5 * float(torch.trace(Kinv @ S) + (m.t() @ Kinv @ m).reshape(()) - M + torch.logdet(Kuu) - torch.logdet(S))
    return tuple(out), kl
