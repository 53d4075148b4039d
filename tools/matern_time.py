"""The dense path with Matern latents on one box, same build: gradient step, value-only ELBO and predict_device at the cfg2 shape
(N = 1e5, M = 512, D = 3) for the kernel pairs (rbf, rbf), (matern32, matern32) and (matern52, matern52), in interleaved windows -- the
RBF pair is the yardstick of the same run, and the spread of its windows is the box's run-to-run noise.

  python tools/matern_time.py          driver: the timing step is a child process under its own `timeout`; everything is appended to
                                       profiles/matern_time.log (or to the file named by MATERN_LOG)
  python tools/matern_time.py time     the timing step (child)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('MATERN_LOG') or os.path.join(ROOT, 'profiles', 'matern_time.log')
N, M, D, REPS, WINDOWS = 100000, 512, 3, 20, 5
PAIRS = (('rbf', 'rbf'), ('matern32', 'matern32'), ('matern52', 'matern52'))


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def child_time():
    import torch
    import bench
    import zigp
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(Y).cuda()
    e.set_data_device(Xd, Yd)
    out = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    ps = {k: dict(p, kern_f=k[0], kern_g=k[1]) for k in PAIRS}
    passes = (('gradient step', lambda q: e.elbo(q)), ('value-only ELBO', lambda q: e.elbo(q, need_grad=False)),
              ('predict_device', lambda q: e.predict_device(q, Xd, out=out)))
    log('N=%d M=%d D=%d  %d interleaved windows of %d calls per kernel pair (ms per call)' % (N, M, D, WINDOWS, REPS))
    for label, fn in passes:
        for k in PAIRS:
            fn(ps[k]); fn(ps[k])                 # warm-up: tile lists, buffers (the K' panel), code objects
        ms = {k: [] for k in PAIRS}
        for _ in range(WINDOWS):
            for k in PAIRS:
                t0 = time.time()
                for _ in range(REPS):
                    fn(ps[k])                    # every call ends in the library's stream synchronisation
                ms[k].append((time.time() - t0) / REPS * 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        for k in PAIRS:
            log('  %-16s %-18s %8.3f (windows %s, spread %.3f)  %.3f x the RBF figure' % (
                label, '/'.join(k), med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]), med[k] / med[PAIRS[0]]))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/matern_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), 'time']
    rc = subprocess.call(cmd)
    if rc != 0:
        log('step failed (exit status %d): %s' % (rc, ' '.join(cmd[4:])))
    return rc


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time()
    else:
        sys.exit(driver())
