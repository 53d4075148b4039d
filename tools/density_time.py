"""What the density kernel costs over the predict pass it rides on, on one box, same build: ms per call of predict_device against
predict_density_device at the cfg2 shape (N = 1e5, M = 512, D = 3) for n_quad = 20, 64 and 256, in interleaved windows -- predict_device
is the yardstick of the same run, and the spread of its windows is the box's run-to-run noise.

  python tools/density_time.py          driver: the timing step is a child process under its own `timeout`; everything is appended to
                                        profiles/density_time.log (or to the file named by DENSITY_LOG)
  python tools/density_time.py time     the timing step (child)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('DENSITY_LOG') or os.path.join(ROOT, 'profiles', 'density_time.log')
N, M, D, REPS, WINDOWS = 100000, 512, 3, 20, 5
QUADS = (20, 64, 256)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def child_time():
    import torch
    import bench
    import zigp
    from zigp.quadrature import gauss_hermite
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    out9 = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    out3 = torch.empty((3, N), dtype=torch.float64, device='cuda:0')
    rules = {n: gauss_hermite(n) for n in QUADS}
    arms = [('predict_device', lambda: e.predict_device(p, Xd, out=out9))]
    arms += [('density n_quad=%d' % n, lambda n=n: e.predict_density_device(p, Xd, Yd, rule=rules[n], out=out3)) for n in QUADS]
    log('N=%d M=%d D=%d  %d interleaved windows of %d calls per arm (ms per call)' % (N, M, D, WINDOWS, REPS))
    for _, fn in arms:
        fn(); fn()                               # warm-up: tile lists, buffers, code objects
    ms = {k: [] for k, _ in arms}
    for _ in range(WINDOWS):
        for k, fn in arms:
            t0 = time.time()
            for _ in range(REPS):
                fn()                             # every call ends in the library's stream synchronisation
            ms[k].append((time.time() - t0) / REPS * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for k, _ in arms:
        log('  %-20s %8.3f (windows %s, spread %.3f)  %+.3f ms over predict_device' % (
            k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]), med[k] - med[arms[0][0]]))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/density_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
