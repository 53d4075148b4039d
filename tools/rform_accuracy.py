"""CPU experiment: accuracy of the variance a gradient step takes from the J' panel (the "R-form").  A gradient step forms R = Q W^T once
(Q = P S - I, P = W^T W = Kuu^-1, S = diag(s^2)) and J' = R A1 with A1 = W K for the reverse pass anyway; per column

    k^T J' = k^T P S P k - k^T P k = sum s^2 A2^2 - sum A1^2,

so var = sigma^2 + colsum(K o J') and the A2 product (A2 = W^T A1) is not needed.  Unlike the rejected B-form (tools/bform_accuracy.py), no
P S P - P is formed: J' comes from the same W-form factors as before.  This prints, per configuration, cond(Kuu) and the largest relative
error of the variance of both forms (products with the explicit inverse W, as the engine computes them) against an 80-bit evaluation with
iterative refinement, and writes the table to profiles/rform_accuracy.log.  tests/test_cpu_rform_variance.py checks the small cases."""
import os
import sys

import numpy as np
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import zigp_oracle as o


def variance_errors(Z, ellv, var, s, X, jit=1e-6, npts=48):
    """(cond(Kuu), relative error of the W-form variance, of the R-form variance), both against 80-bit, over the first npts rows of X"""
    M = Z.shape[0]
    Kuu = o.rbf_K(Z, Z, ellv, var) + jit * np.eye(M)
    cond = np.linalg.cond(Kuu)
    L = sl.cholesky(Kuu, lower=True)
    Kuf = o.rbf_K(Z, X[:npts], ellv, var)
    W = sl.solve_triangular(L, np.eye(M), lower=True)
    s2 = s ** 2
    A1 = W @ Kuf
    A2 = W.T @ A1
    var_w = var - np.sum(A1 ** 2, 0) + np.sum(s2[:, None] * A2 ** 2, 0)          # value-only ELBO and predict
    P = W.T @ W
    Qt = s2[:, None] * P - np.eye(M)                                              # Q^T = S P - I
    R = (W @ Qt).T                                                                # R = Q W^T
    var_r = var + np.sum(Kuf * (R @ A1), 0)                                       # gradient step: sigma^2 + colsum(K o J')
    Kl, kl = Kuu.astype(np.longdouble), Kuf.astype(np.longdouble)

    def solve_ld(b):          # Kuu^-1 b in 80-bit arithmetic: float64 factor + iterative refinement
        x = sl.cho_solve((L, True), b.astype(np.float64)).astype(np.longdouble)
        for _ in range(8):
            x = x + sl.cho_solve((L, True), (b - Kl @ x).astype(np.float64)).astype(np.longdouble)
        return x
    T = np.stack([solve_ld(kl[:, i]) for i in range(Kuf.shape[1])], 1)
    var_t = np.longdouble(var) - np.sum(kl * T, 0) + np.sum((s2[:, None].astype(np.longdouble)) * T * T, 0)
    ew = float(np.max(np.abs(var_w - var_t) / np.abs(var_t)))
    er = float(np.max(np.abs(var_r - var_t) / np.abs(var_t)))
    return cond, ew, er


def cases(full=True):
    """(name, Z, ell, var, s, X): cfg3 (full only), cfg2 and the parity tests' shapes"""
    import bench
    from conftest import make_problem
    out = []
    for M in ((1024, 512) if full else (512,)):
        X, Y, p = bench.synth(4096, M, 3)
        tag = 'cfg3' if M == 1024 else 'cfg2'
        out.append(('%s f' % tag, p['Zf'], p['ell_f'], 1.0, np.ones(M), X))
        out.append(('%s g' % tag, p['Zg'], p['ell_g'], 5.0, np.ones(M), X))
    for (N, M, D, ell) in ((2048, 128, 3, 0.3), (3000, 200, 3, 0.25), (1500, 300, 2, 0.2), (1500, 96, 4, 0.5), (1300, 150, 8, 0.9)):
        X, Y, p = make_problem(N, M, D, seed=N + M, ell=ell)
        for h in ('f', 'g'):
            out.append(('tests %d/%d/D%d %s' % (N, M, D, h), p['Z' + h], p['ell_' + h], p['var_' + h], p['u_%ss_sqrt' % h].reshape(-1), X))
    return out


if __name__ == '__main__':
    lines = ['relative error of the latent variance against 80-bit (48 points per case): W-form = var - sum A1^2 + sum s^2 A2^2, '
             'R-form = var + colsum(K o (Q W^T) A1)']
    for (name, Z, ellv, var, s, X) in cases(full=True):
        cond, ew, er = variance_errors(Z, ellv, var, s, X)
        lines.append('%-22s M %4d cond(Kuu) %.2e | W-form %.2e  R-form %.2e  ratio %.2f' % (name, Z.shape[0], cond, ew, er, er / ew))
        print(lines[-1], flush=True)
    with open(os.path.join(ROOT, 'profiles', 'rform_accuracy.log'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
