"""What the sample paths cost, on one box, same build: ms per sample_paths_device call at the cfg2 shape (N = 1e5, M = 512, D = 3) with
S = 16 sample paths and R = 512 and 2048 random features per latent, next to predict_device of the same run, in interleaved windows.
predict_device is the yardstick, and the spread of an arm's windows is the box's run-to-run noise.  path_rows_device with tables of the
same sizes is the path kernel and its table upload alone (no M x M stage, no weights): the achieved MFMA rate is taken from it, as
2 * 16 ceil(S / 16) * (M4 + R4) * N flops per latent over its time -- a lower bound on the kernel's own rate, the upload included.
The S = 64 arms run the kernel with one, two and four sample tiles per pass (ZIGP_PATH_TILES): the measurement behind that choice.

  python tools/paths_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended to
                                      profiles/paths_time.log (or to the file named by PATHS_LOG)
  python tools/paths_time.py time     the timing step (child)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('PATHS_LOG') or os.path.join(ROOT, 'profiles', 'paths_time.log')
N, M, D, REPS, WINDOWS = 100000, 512, 3, 10, 5
FEATURES = (512, 2048)


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
    from zigp import pathwise
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    out9 = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    rs = np.random.RandomState(0)

    def draws(R, S):
        return {t: pathwise.draw('rbf', R, D, M, S, rs) for t in 'fg'}

    def tables(R, S):
        return [dict(kind='rbf', Z=np.asarray(p['Z' + t]), ell=np.asarray(p['ell_' + t]), var=float(p['var_' + t]), V=rs.randn(M, S) * 1e-3,
                     omega=rs.randn(R, D), phase=rs.uniform(0, 2 * np.pi, R), amp=rs.randn(R, S)) for t in 'fg']

    def capped(cap, fn):                                 # the same call with at most `cap` sample tiles per pass (read at each call)
        os.environ['ZIGP_PATH_TILES'] = str(cap)
        try:
            fn()
        finally:
            del os.environ['ZIGP_PATH_TILES']

    arms, flops = [('predict_device', lambda: e.predict_device(p, Xd, out=out9))], {}
    for S, Rs, caps in ((16, FEATURES, (None,)), (64, (2048,), (1, 2, 4))):
        out3 = torch.empty((3, S, N), dtype=torch.float64, device='cuda:0')
        for R in Rs:
            dr, tb = draws(R, S), tables(R, S)
            for cap in caps:
                tag = 'S=%d R=%d' % (S, R) + ('' if cap is None else ' tiles/pass<=%d' % cap)
                sp = lambda dr=dr, S=S, out3=out3: e.sample_paths_device(p, Xd, n_samples=S, draws=dr, out=out3)
                rows = lambda tb=tb, S=S, out3=out3: e.path_rows_device(tb, Xd, S, out=out3)
                arms.append(('sample_paths_device ' + tag, sp if cap is None else (lambda cap=cap, sp=sp: capped(cap, sp))))
                arms.append(('path_rows_device ' + tag, rows if cap is None else (lambda cap=cap, rows=rows: capped(cap, rows))))
                flops['path_rows_device ' + tag] = 2.0 * 2 * 16 * ((S + 15) // 16) * (M + R) * N
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
        line = '  %-48s %8.3f (windows %s, spread %.3f)' % (k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]))
        if k in flops:
            line += '  MFMA rate >= %.2f TFLOP/s' % (flops[k] / (med[k] * 1e-3) / 1e12)
        elif k != 'predict_device':
            line += '  %.2f x predict_device' % (med[k] / med['predict_device'])
        log(line)
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/paths_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
