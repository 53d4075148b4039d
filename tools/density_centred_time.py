"""What the mode-centred rule costs over the fixed one, on one box, same build: ms per call of predict_density_device with centre='mean'
against centre='mode' at the cfg2 shape (N = 1e5, M = 512, D = 3) for n_quad = 20, 64 and 256, in interleaved windows -- the fixed rule
is the yardstick of the same run, and the spread of its windows is the box's run-to-run noise.  The rows are those of the synthetic
cfg2 problem under its initial parameters: the search's cost depends on how far each row's mode lies from gm (one capped step per
unit of g), so this is the cost on THESE rows, not a bound.

  python tools/density_centred_time.py          driver: the timing step is a child process under its own `timeout`; everything is
                                                appended to profiles/density_centred_time.log (or to the file named by DENSITY_CENTRED_LOG)
  python tools/density_centred_time.py time     the timing step (child)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('DENSITY_CENTRED_LOG') or os.path.join(ROOT, 'profiles', 'density_centred_time.log')
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
    out3 = torch.empty((3, N), dtype=torch.float64, device='cuda:0')
    rules = {n: gauss_hermite(n) for n in QUADS}
    arms = []
    for n in QUADS:
        arms.append(('mean n_quad=%d' % n, lambda n=n: e.predict_density_device(p, Xd, Yd, rule=rules[n], out=out3)))
        arms.append(('mode n_quad=%d' % n, lambda n=n: e.predict_density_device(p, Xd, Yd, rule=rules[n], out=out3, centre='mode')))
    log('N=%d M=%d D=%d  %d interleaved windows of %d calls per arm (ms per call)' % (N, M, D, WINDOWS, REPS))
    _, _, c2 = e.predict_density_device(p, Xd, Yd, rule=rules[20], centre='mode', return_centre=True)
    c2 = c2.cpu().numpy()
    log('  centres of these rows: |zhat| median %.3g, max %.3g; tau from %.3g to %.3g' % (np.median(np.abs(c2[0])), np.abs(c2[0]).max(), c2[1].min(), c2[1].max()))
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
    for i, (k, _) in enumerate(arms):
        base = arms[i - i % 2][0]
        log('  %-20s %8.3f (windows %s, spread %.3f)%s' % (
            k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]),
            '  %+.3f ms over the fixed rule' % (med[k] - med[base]) if i % 2 else ''))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/density_centred_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
