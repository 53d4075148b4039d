"""How far the predictive density's finite sum (include/zigp.h "predictive density") lies from the integral it
stands for, for Gauss-Hermite rules of 20, 64 and 128 nodes.  CPU only: the sum in float64 NumPy (tests/density_ref.py logp_np -- the
GPU kernel agrees with it to rounding, tests/test_gpu_density.py), the integral
    log  int N(g; gm, gv) N(y; link(g) fm, noise + link(g)^2 fv) dg
with mpmath.quad at 30 digits over gm +- 12 sqrt(gv) in 64 panels.  Two row sets:
  toy     every 5th row of data/toydata.mat under the notebook's model (9 inducing points per latent), fitted HERE with the CPU oracle
          (oracle/zigp_oracle_torch.py, 10000 Adam steps in the unconstrained parameters) -- rows a user would actually score;
  stress  fm {0.5, 3, 10} x fv {1e-4, 0.1} x gm {-2, 0, 1.5} x gv {1e-3, 0.3, 9} x y {0, 0.4, 3} at noise 0.01 -- 162 rows, among them
          confident predictions scored against a far-away y, whose mass sits in the far tail of q(g).
The window gm +- 12 sqrt(gv) TRUNCATES the truth: on ten stress rows (gv = 1e-3, fm = 10) mass lies outside it, and on five of them the
reported "truth" is the window's edge, 114 to 1487 nats below the integral (fm = 10, gm = 1.5, gv = 1e-3, y = 0: -3814 here, -2327.6 over
a range that holds the mass).  tools/density_centred_accuracy.py measures the same rows against that wider range.
Appends the table to profiles/density_accuracy.log (or the file named by DENSITY_ACC_LOG).

  python tools/density_accuracy.py
"""
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in ('tests', 'oracle', 'zero-inflated-gp_amd'):
    sys.path.insert(0, os.path.join(ROOT, q))
LOG = os.environ.get('DENSITY_ACC_LOG') or os.path.join(ROOT, 'profiles', 'density_accuracy.log')
QUADS = (20, 64, 128)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def integral(fm, fv, gm, gv, y, noise, dps=30, panels=64, width=12.0):
    import mpmath as mp
    out = []
    with mp.workdps(dps):
        c1, c0, r2 = mp.mpf(1) - mp.mpf('2e-3'), mp.mpf('1e-3'), mp.sqrt(2)
        for a, b, c, d, e in zip(fm, fv, gm, gv, y):
            a, b, c, d, e, s2 = (mp.mpf(float(v)) for v in (a, max(b, 0.0), c, max(d, 0.0), e, noise))
            sg = mp.sqrt(d)

            def f(g):
                ph = (1 + mp.erf(g / r2)) / 2 * c1 + c0
                s = s2 + ph * ph * b
                return mp.exp(-(g - c) ** 2 / (2 * d) - (e - ph * a) ** 2 / (2 * s)) / (2 * mp.pi * mp.sqrt(d * s))
            out.append(mp.log(mp.quad(f, mp.linspace(c - width * sg, c + width * sg, panels + 1))))
    return out


def toy_rows():
    """(fm, fv, gm, gv, y, noise) of every 5th toy row under the model fitted with the CPU oracle"""
    import scipy.io as sio
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    mat = sio.loadmat(os.path.join(ROOT, 'tests', 'golden', 'toydata.mat'))
    X, Y = np.asarray(mat['x'], dtype=np.float64), np.asarray(mat['y'], dtype=np.float64)
    Z = np.delete(np.linspace(X.min(), X.max(), 10, endpoint=False), 0).reshape(-1, 1)
    rs = np.random.RandomState(0)
    p = dict(Zf=Z.copy(), Zg=Z.copy(), u_fm=0.01 * rs.randn(9, 1), u_gm=0.01 * rs.randn(9, 1), u_fs_sqrt=np.ones((9, 1)), u_gs_sqrt=np.ones((9, 1)),
             ell_f=np.array([2.0]), ell_g=np.array([2.0]), var_f=1.0, var_g=5.0, noise=0.01)
    pos = ('u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')
    free = {k: (np.log(np.asarray(p[k], dtype=np.float64)) if k in pos else np.asarray(p[k], dtype=np.float64).copy()) for k in ot.PARAM_KEYS}
    m, v = {k: np.zeros_like(free[k]) for k in free}, {k: np.zeros_like(free[k]) for k in free}

    def constrained():
        q = {k: (np.exp(free[k]) if k in pos else free[k]) for k in free}
        return dict(q, var_f=float(q['var_f']), var_g=float(q['var_g']), noise=float(q['noise']))
    elbo = None
    for t in range(1, 10001):
        q = constrained()
        elbo, _, _, g = ot.elbo_and_grad(X, Y, q, 1e-6)
        for k in free:
            gk = np.asarray(g[k], dtype=np.float64).reshape(free[k].shape) * (np.asarray(q[k]).reshape(free[k].shape) if k in pos else 1.0)
            m[k] = 0.9 * m[k] + 0.1 * gk
            v[k] = 0.999 * v[k] + 0.001 * gk * gk
            free[k] = free[k] + 0.05 * (m[k] / (1 - 0.9 ** t)) / (np.sqrt(v[k] / (1 - 0.999 ** t)) + 1e-8)
    q = constrained()
    rows = [np.asarray(r).reshape(-1)[::5] for r in o.build_predict(X, q, 1e-6, 0.0)]
    return (rows[3], rows[4], rows[5], rows[6], Y.reshape(-1)[::5], q['noise']), float(elbo)


def stress_rows():
    g = np.array(list(itertools.product((0.5, 3.0, 10.0), (1e-4, 0.1), (-2.0, 0.0, 1.5), (1e-3, 0.3, 9.0), (0.0, 0.4, 3.0))))
    return tuple(np.ascontiguousarray(g[:, i]) for i in range(5)) + (0.01,)


def report(tag, rows):
    import density_ref as R
    fm, fv, gm, gv, y, noise = rows
    t0 = time.time()
    truth = integral(fm, fv, gm, gv, y, noise)
    tf = np.array([float(t) for t in truth])
    log('%s: %d rows, log density of the integral from %.1f to %.1f (median %.2f), %d rows below -1000  [mpmath.quad %.0f s]'
        % (tag, len(tf), tf.min(), tf.max(), np.median(tf), int(np.sum(tf < -1000)), time.time() - t0))
    log('  n_quad   median |err|   90th pct   max |err|   max |err| where the truth is above -1000   (nats)')
    for n in QUADS:
        x, w = R.rule(n)
        err = R.err_to(truth, R.logp_np(fm, fv, gm, gv, y, noise, x, w))
        ok = tf > -1000
        log('  %6d   %12.2e   %8.2e   %9.2e   %9.2e' % (n, np.median(err), np.percentile(err, 90), err.max(), err[ok].max() if ok.any() else float('nan')))
        i = int(np.argmax(err))
        log('           worst row: fm %.3g fv %.3g gm %.3g gv %.3g y %.3g, truth %.2f' % (fm[i], fv[i], gm[i], gv[i], y[i], tf[i]))


if __name__ == '__main__':
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/density_accuracy.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    rows, elbo = toy_rows()
    log('toy model fitted with the CPU oracle: ELBO %.3f after 10000 Adam steps, noise %.4g' % (elbo, rows[5]))
    report('toy', rows)
    report('stress', stress_rows())
