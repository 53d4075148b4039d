"""Full-covariance q(u) on the whitened model, restated on the CPU -- TEST INFRASTRUCTURE ONLY (like whiten_ref.py).

GPConditional(..., whiten=True) with a 3-d q_sqrt (onofftf/main.py:257-305: the back-substitution of :282-284 skipped, the q_sqrt.ndims
== 3 branch of :292-296) and the white GaussKL's 3-d branch (q_mu, q_sqrt, K=None: :193-195,208-213,224,227-228,246) in the reference's
op order, in torch float64 so that gradients come from autograd as the reference gets them from tf.gradients.  The kernel, the probit
moments and the likelihood come from oracle/zigp_oracle_torch.py; build_predict / build_likelihood (onoffgpf/OnOffSVGP.py:107-152) are
restated around them with whiten=True (:133,137) and gauss_kl_white as the prior KL (:88-89).

u_fs_sqrt / u_gs_sqrt are (M, M) or (M, M, 1) (num_latent = 1); only band_part(q_sqrt, -1, 0) is read, so whatever lies above the
diagonal changes nothing and gets a zero gradient.  q(u) = N(L u_m, L Lq Lq^T L^T), L = chol(Kuu + jitter I): `explicit_full_cov`
evaluates the same model through that definition and pins this file in tests/test_cpu_fullcov_ref.py.
"""
import numpy as np
import torch

import zigp_oracle_torch as ot
from zigp_oracle_torch import DT, _t, rbf_K, probit_expectations, variational_expectations, PARAM_KEYS, MEAN_KEYS  # noqa: F401


def _lq(q_sqrt, M):
    """tf.matrix_band_part(tf.transpose(q_sqrt, (2, 0, 1)), -1, 0) for num_latent = 1: the (M, M) lower triangle (:212, :293)."""
    return torch.tril(q_sqrt.reshape(M, M))


def conditional_white_full(Xnew, Z, ell, var, q_mu, q_sqrt, jitter):
    """onofftf/main.py:257-305 with whiten=True and a 3-d q_sqrt."""
    M = Z.shape[0]
    Kmn = rbf_K(Z, Xnew, ell, var)
    Kmm = rbf_K(Z, None, ell, var) + torch.eye(M, dtype=DT) * jitter
    Lm = torch.linalg.cholesky(Kmm)
    A = torch.linalg.solve_triangular(Lm, Kmn, upper=False)
    fvar = var - torch.sum(torch.square(A), 0)                                    # :278
    fmean = torch.matmul(A.t(), q_mu.reshape(M, 1))                               # :287 (no :284)
    LTA = torch.matmul(_lq(q_sqrt, M).t(), A)                                     # :293-295
    fvar = fvar + torch.sum(torch.square(LTA), 0)                                 # :302
    return fmean.reshape(-1, 1), fvar.reshape(-1, 1)


def gauss_kl_white_full(q_mu, q_sqrt):
    """onofftf/main.py:187-252 with K=None, the q_sqrt.ndims == 3 branch."""
    M = q_mu.numel()
    Lq = _lq(q_sqrt, M)                                                           # :212
    mahalanobis = torch.sum(torch.square(q_mu))                                   # :218
    constant = -float(M)                                                          # :221 (NM = M * num_latent)
    logdet_qcov = torch.sum(torch.log(torch.square(torch.diagonal(Lq))))          # :213,224
    trace = torch.sum(torch.square(Lq))                                           # :228
    return 0.5 * (mahalanobis + constant - logdet_qcov + trace)                   # :243,252


def latents(X, p, jitter, g_offset=0.0):
    """(fmean, fvar, gmean, gvar) of build_predict (onoffgpf/OnOffSVGP.py:124-142) with whiten=True, q_diag=False."""
    fmean, fvar = conditional_white_full(X, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter)
    if 'mean_a' in p:                                                             # fmean + self.mean_function(Xnew), :134
        fmean = fmean + torch.matmul(X, p['mean_a'].reshape(-1, 1))
    if 'mean_b' in p:
        fmean = fmean + p['mean_b']
    gmean, gvar = conditional_white_full(X, p['Zg'], p['ell_g'], p['var_g'], p['u_gm'], p['u_gs_sqrt'], jitter)
    return fmean, fvar, gmean + g_offset, gvar


def data_term(X, Y, p, jitter, g_offset=0.0):
    fmean, fvar, gmean, gvar = latents(X, p, jitter, g_offset)
    e1, e2, ev = probit_expectations(gmean, gvar)
    return torch.sum(variational_expectations(e1 * fmean, e2 * fvar, ev * torch.square(fmean), Y.reshape(-1, 1), p['noise']))


def prior_kl(p):
    return gauss_kl_white_full(p['u_fm'], p['u_fs_sqrt']) + gauss_kl_white_full(p['u_gm'], p['u_gs_sqrt'])


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
    """As zigp_oracle_torch.elbo_and_grad: (elbo, data, kl, grads dict of numpy), rows in chunks (the data term is a sum over points).
    The u_*s_sqrt gradients have the shape of the inputs; their strict upper triangle is exactly 0."""
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    p = ot.make_leaves({k: v for k, v in p_np.items() if k not in ('whiten', 'q_diag')})
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
    """The same model through its definition: m = L u, S = L Lq Lq^T L^T, then the UNWHITENED full-covariance formulas
    mean = Kfu Kuu^-1 m, var = k** - diag(Kfu Kuu^-1 Kuf) + diag(Kfu Kuu^-1 S Kuu^-1 Kuf), KL(N(m, S) || N(0, Kuu)) with dense matrices.
    Returns ((fmean, fvar, gmean, gvar) as NumPy vectors, kl)."""
    p = _tensors(p_np)
    Xt = _t(X)
    out, kl = [], 0.0
    for tag, off in (('f', 0.0), ('g', g_offset)):
        Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
        M = Z.shape[0]
        u, Lq = p['u_%sm' % tag].reshape(M, 1), torch.tril(p['u_%ss_sqrt' % tag].reshape(M, M))
        Kuu = rbf_K(Z, None, ell, var) + torch.eye(M, dtype=DT) * jitter
        L = torch.linalg.cholesky(Kuu)
        m, S = L @ u, L @ Lq @ Lq.t() @ L.t()
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


def make_lq(p, seed=0, negative=0, garbage=False):
    """The test problems' factors: Lq = diag(s) + (0.1 / sqrt(M)) tril(randn, -1) from the diagonal model's s (conftest.make_problem), as
    (M, M).  negative: that many diagonal entries get a minus sign; garbage: the strict upper triangle is filled with numbers the
    model must ignore.  Returns a copy of p with whiten=True, q_diag=False."""
    rs, rg = np.random.RandomState(1000 + seed), np.random.RandomState(2000 + seed)     # the garbage has a stream of its own: same Lq with and without
    q = dict(p, whiten=True, q_diag=False)
    for tag in 'fg':
        s = np.asarray(p['u_%ss_sqrt' % tag], dtype=np.float64).reshape(-1)
        M = s.size
        Lq = np.diag(s) + (0.1 / np.sqrt(M)) * np.tril(rs.randn(M, M), -1)
        if negative:
            idx = rs.choice(M, size=min(negative, M), replace=False)
            Lq[idx, idx] *= -1.0
        if garbage:
            Lq = Lq + np.triu(7.0 + 100.0 * rg.randn(M, M), 1)
        q['u_%ss_sqrt' % tag] = Lq
    return q
