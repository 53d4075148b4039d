"""The heads on the dense path beside the OnOff model on one box, same build: gradient step, value-only step and predict on device rows
for the Gaussian head, the Bernoulli head (DenseEngine.head_elbo / head_predict_device) and the OnOff model with Mg = Mf (elbo /
predict_device), at the cfg2 shape (N = 1e5, M = 512, D = 3) and the cfg3 shape (N = 1e6, M = 1024, D = 3), in interleaved windows of
one process -- the OnOff arm is the yardstick of the same run, and the spread of its windows is the box's run-to-run noise.
Expectation by flop count (stated, not asserted): a head step is about half an OnOff step plus the placeholder latent's share,
(128 / Mp)^2 of latent f's matrix work, plus its launches.

  python tools/dense_head_time.py          driver: each shape is a child process under its own `timeout`; everything is appended to
                                           profiles/dense_head_time.log (or to the file named by DENSE_HEAD_LOG)
  python tools/dense_head_time.py time SHAPE   the timing step (child); SHAPE = cfg2 or cfg3
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('DENSE_HEAD_LOG') or os.path.join(ROOT, 'profiles', 'dense_head_time.log')
SHAPES = dict(cfg2=(100000, 512, 3, 10, 5), cfg3=(1000000, 1024, 3, 2, 5))      # N, M, D, calls per window, windows
ARMS = ('onoff', 'gaussian', 'bernoulli')


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def child_time(shape):
    import torch
    import bench
    import zigp
    N, M, D, reps, windows = SHAPES[shape]
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    Yd = {'onoff': torch.from_numpy(Y).cuda(), 'gaussian': torch.from_numpy(Y).cuda(), 'bernoulli': torch.from_numpy((Y != 0) * 1.0).cuda()}
    ph = {k: p[k] for k in zigp.HEAD_PARAM_KEYS}
    out9 = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    out4 = torch.empty((4, N), dtype=torch.float64, device='cuda:0')

    def step(arm, need_grad):
        return e.elbo(p, need_grad=need_grad) if arm == 'onoff' else e.head_elbo(ph, arm, need_grad=need_grad)

    def predict(arm):
        return e.predict_device(p, Xd, out=out9) if arm == 'onoff' else e.head_predict_device(ph, Xd, arm, out=out4)

    passes = (('gradient step', lambda a: step(a, True)), ('value-only step', lambda a: step(a, False)), ('predict on device rows', predict))
    log('%s: N=%d M=%d D=%d  %d interleaved windows of %d calls per arm (ms per call; OnOff has Mg = Mf = %d)' % (shape, N, M, D, windows, reps, M))
    for label, fn in passes:
        ms = {a: [] for a in ARMS}
        for w in range(windows + 1):             # window 0 is the warm-up of every arm: tile lists, buffers, code objects
            for a in ARMS:
                if not label.startswith('predict'):
                    e.set_data_device(Xd, Yd[a])     # the labels of the arm (a pointer hand-over, outside the timed calls)
                t0 = time.time()
                for _ in range(reps):
                    fn(a)                        # every call ends in the library's stream synchronisation
                if w:
                    ms[a].append((time.time() - t0) / reps * 1e3)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        for a in ARMS:
            log('  %-22s %-10s %9.3f (windows %s, spread %.3f)  %.3f x the OnOff figure' % (
                label, a, med[a], ' '.join('%.3f' % v for v in ms[a]), max(ms[a]) - min(ms[a]), med[a] / med['onoff']))
    Mp = (M + 127) // 128 * 128
    log('  expectation by flop count: 0.5 + (128 / %d)^2 / 2 = %.3f of the OnOff figure, plus the placeholder latent\'s launches' % (
        Mp, 0.5 + 0.5 * (128.0 / Mp) ** 2))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/dense_head_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    worst = 0
    for shape, limit in (('cfg2', '240'), ('cfg3', '420')):
        cmd = ['timeout', '-k', '10', limit, sys.executable, os.path.abspath(__file__), 'time', shape]
        rc = subprocess.call(cmd)
        if rc != 0:
            log('step failed (exit status %d): %s' % (rc, ' '.join(cmd[4:])))
            return rc                            # nothing more is started on the GPU after a failed step
        worst = max(worst, rc)
    return worst


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'time':
        child_time(sys.argv[2])
    else:
        sys.exit(driver())
