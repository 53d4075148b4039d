"""What the factored Kronecker path kernel buys, on one box, same build: ms per call at cfg5's row count (N = 105 280, D = (2, 1)) with
grids 32 x 32 and 10 x 100, S = 16 and 64 sample paths and R = 0 and 1024 random features, in interleaved windows.
  arm A  kron_path_rows_device: the factored kernel (M0 + M1 exponentials a row, then one multiply a grid point)
  arm B  path_rows_device on the expanded grid (M0 M1 exponentials a row): existing code, the yardstick
The spread of an arm's windows is the box's run-to-run noise.  At R = 0 arm A has to beat arm B by more than that spread at both grids
and both S; the R = 1024 figures are reported as measured (the cosines are the same work in both arms).  Both arms carry their table
upload.  Then the model call (S = 16, R = 1024) beside kron_predict of the same rows.  kron_predict has no device form: it takes host rows
and pays their transfer and that of its (9, N) result on every call, so the like-for-like arm is kron_sample_paths on host rows (which
brings a (3, 16, N) result back); kron_sample_paths_device, whose rows and result stay on the device, is shown next to them.

  python tools/kron_paths_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended to
                                           profiles/kron_paths_time.log (or to the file named by KRON_PATHS_LOG)
  python tools/kron_paths_time.py time     the timing step (child)
"""
import gc
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
LOG = os.environ.get('KRON_PATHS_LOG') or os.path.join(ROOT, 'profiles', 'kron_paths_time.log')
N, DIMS, REPS, WINDOWS = 105280, (2, 1), 10, 5
GRIDS = ((32, 32), (10, 100))


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def child_time():
    import torch
    import zigp
    import kron_nd
    import kronpaths_ref as kr
    from zigp import pathwise
    e = zigp.DenseEngine(0)
    rs = np.random.RandomState(0)
    X = np.hstack([rs.rand(N, 2) * 10.0, rs.rand(N, 1)])
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()

    def latent(grid, R, S):
        M0, M1 = grid
        return dict(Z=[rs.rand(M0, 2) * 10.0, rs.rand(M1, 1)], ell=[np.array([3.0, 3.5]), np.array([0.3])], var=[1.5, 1.2],
                    V=rs.randn(M0 * M1, S) * 1e-3, omega=rs.randn(R, 3), phase=rs.uniform(0, 2 * np.pi, R), amp=rs.randn(R, S), shift=0.0)

    arms, pairs = [], []
    for grid in GRIDS:
        for S in (16, 64):
            out = torch.empty((1, S, N), dtype=torch.float64, device='cuda:0')
            for R in (0, 1024):
                lat = latent(grid, R, S)
                dense = kr.expand(lat)
                tag = '%dx%d S=%d R=%d' % (grid[0], grid[1], S, R)
                arms.append(('A kron_path_rows_device ' + tag, lambda lat=lat, S=S, out=out: e.kron_path_rows_device([lat], Xd, S, DIMS, out=out)))
                arms.append(('B path_rows_device      ' + tag, lambda dense=dense, S=S, out=out: e.path_rows_device([dense], Xd, S, out=out)))
                pairs.append((tag, R, arms[-2][0], arms[-1][0], 2.0 * 16 * ((S + 15) // 16) * (grid[0] * grid[1] + R) * N))
    model = []
    for grid in GRIDS:
        Xp, Yp, p = kron_nd.make_kron_problem_nd(64, grid[0], grid[1], 2, 1, seed=5, c=0.5)
        S = 16
        d = {t: pathwise.draw('rbf', 1024, 3, grid[0] * grid[1], S, rs) for t in 'fg'}
        out3 = torch.empty((3, S, N), dtype=torch.float64, device='cuda:0')
        tag = '%dx%d' % grid
        arms.append(('kron_predict (host rows)      ' + tag, lambda p=p: e.kron_predict(p, X, jitter=1e-5)))
        arms.append(('kron_sample_paths (host rows) ' + tag + ' S=16 R=1024', lambda p=p, d=d: e.kron_sample_paths(p, X, n_samples=16, draws=d, jitter=1e-5)))
        arms.append(('kron_sample_paths_device      ' + tag + ' S=16 R=1024', lambda p=p, d=d, out3=out3: e.kron_sample_paths_device(p, Xd, n_samples=16, draws=d, jitter=1e-5, out=out3)))
        model.append((arms[-3][0], arms[-2][0], arms[-1][0]))
    log('this build  N=%d D=%s  %d interleaved windows of %d calls per arm (ms per call)' % (N, DIMS, WINDOWS, REPS))
    for _, fn in arms:
        fn(); fn()                               # warm-up: buffers, code objects
    ms = {k: [] for k, _ in arms}
    gc.collect()
    gc.disable()                                 # as timeit does: a collection of the interpreter's is not part of any arm
    for _ in range(WINDOWS):
        for k, fn in arms:
            reps = 3 if '(host rows)' in k else REPS
            t0 = time.time()
            for _ in range(reps):
                fn()                             # every call ends in the library's stream synchronisation
            ms[k].append((time.time() - t0) / reps * 1e3)
    med = {k: median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    for k, _ in arms:
        log('  %-52s %8.3f (windows %s, spread %.3f)' % (k, med[k], ' '.join('%.3f' % v for v in ms[k]), spread[k]))
    ok = True
    for tag, R, ka, kb, flops in pairs:
        gain, noise = med[kb] - med[ka], max(spread[ka], spread[kb])
        verdict = '' if R else ('  A beats B by more than the spread' if gain > noise else '  A DOES NOT beat B by more than the spread')
        if R == 0 and gain <= noise:
            ok = False
        log('  %-24s B / A = %5.2f  (B - A = %.3f ms, spread %.3f)  A: MFMA rate >= %.2f TFLOP/s%s' % (tag, med[kb] / med[ka], gain, noise,
                                                                                                        flops / (med[ka] * 1e-3) / 1e12, verdict))
    for kp, kh, kd in model:
        log('  %s = %.2f x %s (both on host rows); the device form, nothing but tables crossing: %.3f ms' % (kh.strip(), med[kh] / med[kp], kp.strip(), med[kd]))
    log('R = 0: the factored kernel %s the expanded-grid call at every grid and S' % ('beats' if ok else 'DOES NOT beat'))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/kron_paths_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
