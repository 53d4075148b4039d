"""What scoring the sample paths where they lie buys, on one box, same build: ms per call at cfg5's row count (N = 105 280, D = (2, 1),
grid 32 x 32), S = 16 and 64 members, in interleaved windows.
  arm a  kron_sample_paths_device alone (the (3, S, N) block stays on the device)
  arm b  kron_path_scores_device = arm a + ensemble_scores_device (totals, CRPS of the totals, energy), with one group and with 365 groups
  arm c  the status quo: kron_sample_paths on host rows (the block comes back over PCIe) + the same scores in vectorised NumPy
Then the scorer alone on a resident ensemble: the energy score (energy=True, nothing else) at S = 16 / 64 / 256 as a fraction of the
78.6 TFLOP/s fp64 vector rate -- the CALL's time (pairs kernel, chunk reduction, finish, one synchronisation), so a lower bound of the
kernel's rate; 3 flops per member pair and row (a subtraction and an fma) -- and the variogram (p = 0.5) at groups of 288 and 4096 rows.
No figure is fixed in advance; the spread of an arm's windows is the box's run-to-run noise.

  python tools/ensemble_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended to
                                         profiles/ensemble_time.log (or to the file named by ENSEMBLE_LOG)
  python tools/ensemble_time.py time     the timing step (child)
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
LOG = os.environ.get('ENSEMBLE_LOG') or os.path.join(ROOT, 'profiles', 'ensemble_time.log')
N, REPS, WINDOWS = 105280, 5, 3
GRID = (32, 32)
PEAK = 78.6e12


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def np_scores(E, y, off):
    """totals, CRPS of the totals and the energy score per group as a user would write them in NumPy (standard c = 1 / S^2)"""
    S = E.shape[0]
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        X, Y = E[:, lo:hi], y[lo:hi]
        T, To = X.sum(1), Y.sum()
        crps = np.abs(T - To).mean() - np.abs(T[:, None] - T[None, :]).sum() / (2.0 * S * S)
        d1 = np.sqrt(((X - Y) ** 2).sum(1)).mean()
        d2 = sum(np.sqrt(((X[:t] - X[t]) ** 2).sum(1)).sum() for t in range(1, S))
        out.append((crps, d1 - d2 / (S * S)))
    return out


def child_time():
    import torch
    import zigp
    import kron_nd
    from zigp import pathwise
    e = zigp.DenseEngine(0)
    rs = np.random.RandomState(0)
    X = np.hstack([rs.rand(N, 2) * 10.0, rs.rand(N, 1)])
    y = np.abs(rs.randn(N))
    Xd, yd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(y).cuda()
    off365 = np.linspace(0, N, 366).astype(np.int64)
    off1 = np.array([0, N])
    Xp, Yp, p = kron_nd.make_kron_problem_nd(64, GRID[0], GRID[1], 2, 1, seed=5, c=0.5)
    arms = []
    for S in (16, 64):
        d = {t: pathwise.draw('rbf', 1024, 3, GRID[0] * GRID[1], S, rs) for t in 'fg'}
        out3 = torch.empty((3, S, N), dtype=torch.float64, device='cuda:0')
        arms.append(('a kron_sample_paths_device            S=%d' % S, REPS,
                     lambda d=d, S=S, out3=out3: e.kron_sample_paths_device(p, Xd, n_samples=S, draws=d, jitter=1e-5, out=out3)))
        for name, off in (('1 group   ', off1), ('365 groups', off365)):
            arms.append(('b kron_path_scores_device %s S=%d' % (name, S), REPS,
                         lambda d=d, S=S, off=off: e.kron_path_scores_device(p, Xd, yd, groups=off, n_samples=S, draws=d, jitter=1e-5)))
            arms.append(('c host paths + NumPy      %s S=%d' % (name, S), 1,
                         lambda d=d, S=S, off=off: np_scores(e.kron_sample_paths(p, X, n_samples=S, draws=d, jitter=1e-5)['gf'], y, off)))
    alone = []
    for S in (16, 64, 256):
        E_t = yd[None, :] + 0.3 * torch.randn((S, N), dtype=torch.float64, device='cuda:0')
        k = 'energy alone, 1 group                 S=%d' % S
        arms.append((k, REPS, lambda E_t=E_t: e.ensemble_scores_device(E_t, yd, totals=False)))
        alone.append((k, 3.0 * (S + 1) * (S + 2) / 2 * N))
        if S == 16:
            for rows in (288, 4096):
                off = np.append(np.arange(0, N, rows), N).astype(np.int64)
                arms.append(('variogram p=0.5 alone, groups of %-5d S=%d' % (rows, S), REPS,
                             lambda E_t=E_t, off=off: e.ensemble_scores_device(E_t, yd, groups=off, energy=False, totals=False, variogram=0.5)))
    log('this build  N=%d grid %dx%d  %d interleaved windows (ms per call; arm c: one call per window)' % (N, GRID[0], GRID[1], WINDOWS))
    for _, _, fn in arms:
        fn()                                     # warm-up: buffers, code objects
    ms = {k: [] for k, _, _ in arms}
    gc.collect()
    gc.disable()
    for _ in range(WINDOWS):
        for k, reps, fn in arms:
            t0 = time.time()
            for _ in range(reps):
                fn()                             # every call ends in the library's stream synchronisation
            ms[k].append((time.time() - t0) / reps * 1e3)
    med = {k: median(v) for k, v in ms.items()}
    for k, _, _ in arms:
        log('  %-48s %10.3f (windows %s, spread %.3f)' % (k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k])))
    for S in (16, 64):
        a = med['a kron_sample_paths_device            S=%d' % S]
        for name in ('1 group   ', '365 groups'):
            b, c = med['b kron_path_scores_device %s S=%d' % (name, S)], med['c host paths + NumPy      %s S=%d' % (name, S)]
            log('  S=%d %s: scoring on the device adds %.3f ms to the paths; status quo / device = %.1f (%s)'
                % (S, name.strip(), b - a, c / b, 'b ahead of c' if b < c else 'b NOT ahead of c'))
    for k, flops in alone:
        log('  %s: >= %.2f TFLOP/s = %.1f %% of the 78.6 TFLOP/s fp64 vector rate (call time)' % (k.strip(), flops / (med[k] * 1e-3) / 1e12,
                                                                                               100.0 * flops / (med[k] * 1e-3) / PEAK))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/ensemble_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
