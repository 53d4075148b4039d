"""The single-latent heads on the dense path (zigp_head_elbo / zigp_head_predict), restated on the CPU -- TEST INFRASTRUCTURE ONLY.

GPflow 0.4.0's SVGP with likelihoods.Gaussian / likelihoods.Bernoulli as the reference's baselines state it: latent f through
matern_ref.conditional(kind, mode, ...) and matern_ref.latent_kl (the three kernels and the diag / white / white-full parametrisations,
checked by tests/test_cpu_matern.py and tests/test_cpu_fullcov_ref.py), the mean function of f as matern_ref.latents adds it, and the
head as the literal lines of oracle.kron_head_elbo and oracle.head_probit:
    'gaussian'   ve = -0.5 log(2 pi) - 0.5 log(noise) - 0.5 ((Y - fmean)^2 + fvar) / noise           scripts/svgp.py:198-200
    'bernoulli'  pr = 0.5 (1 + erf(x / sqrt 2)) (1 - 2e-3) + 1e-3 at x = fmean / sqrt(1 + fvar),     scripts/classifier.py:139,216-217
                 ve = log(where(Y == 1, pr, 1 - pr))                                                 classifier.py:213-214
In torch float64; gradients come from autograd.  `mistake` plants one of five deliberate errors (tests/test_cpu_dense_head.py shows that
each is caught): 'no_fv', 'no_clamp', 'y_gt_0', 'dfv_sign' (in the hand-derived cotangents, head_cotangents) and 'placeholder_kl'.
"""
import math

import numpy as np
import torch

import zigp_oracle_torch as ot
import matern_ref as mr
from zigp_oracle_torch import DT, _t

HEAD_KEYS = ('Zf', 'u_fm', 'u_fs_sqrt', 'ell_f', 'var_f', 'noise')
LIKS = ('gaussian', 'bernoulli')
MISTAKES = ('no_fv', 'no_clamp', 'y_gt_0', 'dfv_sign', 'placeholder_kl')
_NOT_PARAMS = ('whiten', 'q_diag', 'kern_f', 'kern_g')


def head_probit(x, mistake=None):                                        # classifier.py:216-217
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return cdf if mistake == 'no_clamp' else cdf * (1 - 2e-3) + 1e-3


def head_ve(lik, fmean, fvar, Y, noise, mistake=None):
    """(N, 1) expected log-likelihood of each row"""
    if lik == 'gaussian':
        q = torch.square(Y - fmean) + (0.0 if mistake == 'no_fv' else fvar)
        return -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(noise) - 0.5 * q / noise        # svgp.py:198-200
    pr = head_probit(fmean / torch.sqrt(1 + fvar), mistake)                                    # classifier.py:139
    on = (Y > 0) if mistake == 'y_gt_0' else (Y == 1)
    return torch.log(torch.where(on, pr, 1 - pr))                                              # classifier.py:213-214


def head_cotangents(lik, fm, fv, y, noise, mistake=None):
    """(dfm, dfv, dnoise) of ve, hand-derived as the kernel forms them (k_kron_head_pointwise): numpy float64.
    Gaussian: dfm = (y - fm) / noise, dfv = -1/2 / noise, dnoise = -1/2 / noise + 1/2 q / noise^2.
    Bernoulli, z = fm / sqrt(1 + fv), w = p or 1 - p: dz = +-(1 - 2e-3) phi(z) / w, dfm = dz / sqrt(1 + fv), dfv = -dz z / (2 (1 + fv))."""
    from scipy.special import erf
    fm, fv, y = (np.asarray(a, dtype=np.float64) for a in (fm, fv, y))
    sign = -1.0 if mistake == 'dfv_sign' else 1.0
    if lik == 'gaussian':
        inv, res = 1.0 / noise, y - fm
        q = res * res + fv
        return res * inv, sign * (-0.5 * inv) * np.ones_like(fm), -0.5 * inv + 0.5 * q * inv * inv
    r = 1.0 / np.sqrt(1.0 + fv)
    z = fm * r
    pr = 0.5 * (1.0 + erf(z / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
    on = y == 1.0
    dz = np.where(on, 1.0 / pr, -1.0 / (1.0 - pr)) * (1 - 2e-3) * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    return dz * r, sign * dz * (-0.5 * z / (1.0 + fv)), np.zeros_like(fm)


def latent_f(X, p, kind, mode, jitter):
    """(fmean, fvar) (N, 1) of latent f with its mean function (onoffgpf/OnOffSVGP.py:134)"""
    fmean, fvar = mr.conditional(kind, mode, X, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter)
    if 'mean_a' in p:
        fmean = fmean + torch.matmul(X, p['mean_a'].reshape(-1, 1))
    if 'mean_b' in p:
        fmean = fmean + p['mean_b']
    return fmean, fvar


def _leaves(p_np, need_grad):
    keys = HEAD_KEYS + tuple(k for k in ot.MEAN_KEYS if p_np.get(k) is not None)
    return {k: _t(p_np.get(k, 1.0)).clone().requires_grad_(need_grad) for k in keys}


def _placeholder_kl(mode, jitter):
    """KL of the placeholder latent of a head call (one point at the origin, u = 0, s = 1, ell = var = 1, RBF): what 'placeholder_kl'
    leaves in"""
    one = torch.ones(1, dtype=DT)
    return mr.latent_kl('rbf', mode, torch.zeros(1, 1, dtype=DT), one, 1.0, torch.zeros(1, 1, dtype=DT),
                        torch.ones(1, 1, 1, dtype=DT) if mode == 'white_full' else torch.ones(1, 1, dtype=DT), jitter)


def elbo_and_grad(X, Y, p_np, lik, jitter, scale=1.0, include_kl=True, need_grad=True, chunk=500, mistake=None):
    """(elbo, data, kl, grads): data = sum ve (unscaled), elbo = scale * data - kl, grads of elbo for HEAD_KEYS (+ mean_a / mean_b) as numpy
    arrays.  p_np: the f fields, 'noise' (Gaussian), 'whiten' / 'q_diag' / 'kern_f' as DenseEngine reads them."""
    Xt, Yt = _t(X), _t(Y).reshape(-1, 1)
    kind, mode = p_np.get('kern_f', 'rbf'), mr.mode_of(p_np)
    p = _leaves({k: v for k, v in p_np.items() if k not in _NOT_PARAMS}, need_grad)
    data = 0.0
    for s in range(0, Xt.shape[0], chunk):
        with torch.set_grad_enabled(need_grad):
            fmean, fvar = latent_f(Xt[s:s + chunk], p, kind, mode, jitter)
            d = torch.sum(head_ve(lik, fmean, fvar, Yt[s:s + chunk], p['noise'], mistake))
        if need_grad:
            (d * scale).backward()
        data += float(d.detach())
    kl = 0.0
    if include_kl:
        with torch.set_grad_enabled(need_grad):
            k = mr.latent_kl(kind, mode, p['Zf'], p['ell_f'], p['var_f'], p['u_fm'], p['u_fs_sqrt'], jitter)
            if mistake == 'placeholder_kl':
                k = k + _placeholder_kl(mode, jitter)
        if need_grad:
            (-k).backward()
        kl = float(k.detach())
    grads = {k: (p[k].grad.numpy().copy() if p[k].grad is not None else np.zeros(tuple(p[k].shape))) for k in p} if need_grad else None
    return data * scale - kl, data, kl, grads


def head_predict(X, p_np, lik, jitter):
    """(4, N): fmean, fvar, pfmean, pfvar -- Gaussian: fmean, fvar + noise; Bernoulli: pr, pr - pr^2 (classifier.py:140)"""
    with torch.no_grad():
        p = _leaves({k: v for k, v in p_np.items() if k not in _NOT_PARAMS}, False)
        fmean, fvar = latent_f(_t(X), p, p_np.get('kern_f', 'rbf'), mr.mode_of(p_np), jitter)
        if lik == 'gaussian':
            rows = (fmean, fvar, fmean, fvar + p['noise'])
        else:
            pr = head_probit(fmean / torch.sqrt(1 + fvar))
            rows = (fmean, fvar, pr, pr - torch.square(pr))
        return np.stack([r.reshape(-1).numpy() for r in rows])


# ---- the kernel's own arithmetic on the partial-row planes, for the stage test (float64 numpy, operation by operation) ----
def wave_sum(v):
    """The kernel's sum over the 64 lanes of a wave: the xor-shuffle tree v += v[lane ^ o], o = 32, 16, ..., 1 (every lane ends with the
    same double).  v: (..., 64); returns (...)."""
    v = np.array(v, dtype=np.float64, copy=True)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]
