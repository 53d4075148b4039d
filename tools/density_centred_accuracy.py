"""How far the predictive density's finite sum lies from the integral it stands for, for the Gauss-Hermite rule centred on gm
(density_rows(centre='mean'), tests/density_ref.py logp_np) and for the same rule shifted and scaled to each row's mode
(centre='mode', tests/density_centred_ref.py centre_np + logp_centred_np), at 20, 32 and 64 nodes.  CPU only, from the references alone:
the GPU kernels agree with them to rounding (tests/test_gpu_density.py, tests/test_gpu_density_centred.py).

Rows: the 162-row stress grid of tools/density_accuracy.py at noise 0.01.  Truth: mpmath.quad at 30 digits over
[min(gm - 12 sg, -9), max(gm + 12 sg, 9)] in g (density_centred_ref.integral_mp) -- NOT the gm +- 12 sg window of
tools/density_accuracy.py, which cuts the mass off on the rows where it sits far from gm; the rows on which the two truths differ by
more than 1e-6 nats are listed.

Appends the table to profiles/density_centred_accuracy.log (or the file named by DENSITY_CENTRED_ACC_LOG).  With `golden` as its
argument it also rewrites tests/golden/density_centred_stress_integral.txt, the 30-digit integrals the tests read.

  python tools/density_centred_accuracy.py [golden]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in ('tests', 'tools'):
    sys.path.insert(0, os.path.join(ROOT, q))
LOG = os.environ.get('DENSITY_CENTRED_ACC_LOG') or os.path.join(ROOT, 'profiles', 'density_centred_accuracy.log')
QUADS = (20, 32, 64)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def main(write_golden):
    import mpmath as mp
    import density_ref as R
    import density_centred_ref as Q
    import density_accuracy as A
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/density_centred_accuracy.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    rows = Q.stress()
    zhat, tau = Q.centre_np(*rows, Q.NOISE)
    t0 = time.time()
    truth = Q.integral_mp(rows, zhat, tau)
    tf = np.array([float(t) for t in truth])
    log('stress: %d rows, noise %.3g, log density of the integral from %.1f to %.1f (median %.2f)  [mpmath.quad %.0f s]'
        % (len(tf), Q.NOISE, tf.min(), tf.max(), np.median(tf), time.time() - t0))
    log('search: zhat from %.3g to %.3g, tau from %.3g to %.3g (%d rows at tau_max %.2g)'
        % (zhat.min(), zhat.max(), tau.min(), tau.max(), int(np.sum(tau == Q.TAU_MAX)), Q.TAU_MAX))
    t0 = time.time()
    cut = np.array([float(t) for t in A.integral(*rows, Q.NOISE)])
    off = np.abs(cut - tf)
    log('truth of tools/density_accuracy.py (gm +- 12 sg only): %d rows differ by more than 1e-6 nats, by up to %.1f  [%.0f s]'
        % (int(np.sum(off > 1e-6)), off.max(), time.time() - t0))
    for i in np.nonzero(off > 1e-6)[0]:
        log('    fm %.3g fv %.3g gm %.3g gv %.3g y %.3g: window %.2f, integral %.2f' % (tuple(r[i] for r in rows) + (cut[i], tf[i])))
    log('  n_quad   gm-centred: median   90th pct        max   rows > 1e-2   mode-centred: median   90th pct        max   rows > 1e-2   (|error|, nats)')
    for n in QUADS:
        ru = Q.rule(n)
        e0 = R.err_to(truth, R.logp_np(*rows, Q.NOISE, *ru))
        e1 = R.err_to(truth, Q.logp_centred_np(rows, zhat, tau, ru))
        log('  %6d   %20.2e   %8.2e   %8.2e   %11d   %20.2e   %8.2e   %8.2e   %11d'
            % (n, np.median(e0), np.percentile(e0, 90), e0.max(), int(np.sum(e0 > 1e-2)),
               np.median(e1), np.percentile(e1, 90), e1.max(), int(np.sum(e1 > 1e-2))))
        i = int(np.argmax(e1))
        log('           mode-centred worst row: fm %.3g fv %.3g gm %.3g gv %.3g y %.3g, zhat %.4g tau %.4g, truth %.2f'
            % (tuple(r[i] for r in rows) + (zhat[i], tau[i], tf[i])))
        far = e0 > 1.0
        log('           rows where the gm-centred sum is more than 1 nat off: %d; the mode-centred sum is closer on %d of them'
            % (int(far.sum()), int(np.sum(e1[far] < e0[far]))))
    if write_golden:
        with open(Q.STRESS_TRUTH, 'w') as f:
            f.write('# log of the integral on the 162 stress rows (tests/density_centred_ref.py stress, integral_mp), 30 digits;\n')
            f.write('# written by tools/density_centred_accuracy.py golden.  fm fv gm gv y  log-integral\n')
            with mp.workdps(30):
                for i, t in enumerate(truth):
                    f.write('%g %g %g %g %g  %s\n' % (tuple(r[i] for r in rows) + (mp.nstr(t, 30),)))
        log('wrote %s' % os.path.relpath(Q.STRESS_TRUTH, ROOT))


if __name__ == '__main__':
    main(len(sys.argv) > 1 and sys.argv[1] == 'golden')
