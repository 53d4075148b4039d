"""What the predictive scores cost, on one box, same build: ms per call at the cfg2 shape (N = 1e5, M = 512, D = 3) of predict_device --
the pass the scores ride on -- against predict_scores_device asking for the CDF pair alone, the CDF pair plus 3 quantile levels
(0.05, 0.5, 0.95), and all of it with the CRPS, at n_quad = 20, 64 and 256, in interleaved windows.  predict_device is the yardstick, and the
spread of an arm's windows is the box's run-to-run noise.  The rows are those of the synthetic cfg2 problem under its initial parameters:
the quantile search's iteration count depends on the rows, so the quantile arms are the cost on THESE rows, not a bound.  The kernel gives
a row a whole wave, or half a wave where the rule has at most 32 nodes (csrc/zigp_score.hip): the n_quad = 20 arms are run a second time
with ZIGP_SCORE_WAVE_PER_ROW=1, which gives every rule a whole wave -- the measurement behind that choice.

  python tools/score_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended to
                                      profiles/score_time.log (or to the file named by SCORE_LOG)
  python tools/score_time.py time     the timing step (child)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('SCORE_LOG') or os.path.join(ROOT, 'profiles', 'score_time.log')
N, M, D, REPS, WINDOWS = 100000, 512, 3, 10, 5
QUADS = (20, 64, 256)
LEVELS = (0.05, 0.5, 0.95)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def child_time():
    import torch
    import bench
    import zigp
    from zigp.quadrature import gauss_hermite
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    out9 = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    rules = {n: gauss_hermite(n) for n in QUADS}
    kinds = (('cdf', dict(crps=False)), ('cdf+3q', dict(crps=False, levels=LEVELS)), ('cdf+3q+crps', dict(levels=LEVELS)))
    arms = [('predict_device', lambda: e.predict_device(p, Xd, out=out9))]
    def whole_wave(n, kw):                           # the same call with a whole wave per row (the library reads the variable at each call)
        os.environ['ZIGP_SCORE_WAVE_PER_ROW'] = '1'
        try:
            e.predict_scores_device(p, Xd, Yd, rule=rules[n], **kw)
        finally:
            del os.environ['ZIGP_SCORE_WAVE_PER_ROW']
    for n in QUADS:
        arms += [('%s n_quad=%d' % (k, n), lambda n=n, kw=kw: e.predict_scores_device(p, Xd, Yd, rule=rules[n], **kw)) for k, kw in kinds]
        if n <= 32:                                  # a rule this small runs two rows per wave: the other layout beside it
            arms += [('%s n_quad=%d wave/row' % (k, n), lambda n=n, kw=kw: whole_wave(n, kw)) for k, kw in kinds]
    log('this build  N=%d M=%d D=%d  %d interleaved windows of %d calls per arm (ms per call)' % (N, M, D, WINDOWS, REPS))
    for _, fn in arms:
        fn(); fn()                               # warm-up: tile lists, buffers, code objects
    ms = {k: [] for k, _ in arms}
    for _ in range(WINDOWS):
        for k, fn in arms:
            t0 = time.time()
            for _ in range(REPS):
                fn()                             # every call ends in the library's stream synchronisation
            ms[k].append((time.time() - t0) / REPS * 1e3)
    med = {k: median(v) for k, v in ms.items()}
    for k, _ in arms:
        line = '  %-32s %8.3f (windows %s, spread %.3f)' % (k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]))
        if k != 'predict_device':
            line += '  %+.3f ms over predict_device' % (med[k] - med['predict_device'])
        if k.endswith(' wave/row'):
            line += ', %+.3f ms over two rows per wave' % (med[k] - med[k[:-len(' wave/row')]])
        log(line)
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/score_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    cmd = ['timeout', '-k', '10', '420', sys.executable, os.path.abspath(__file__), 'time']
    rc = subprocess.call(cmd)
    if rc != 0:
        log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
    return rc


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time()
    else:
        sys.exit(driver())
