"""What a Matern factor costs on the Kronecker path, on one box, same build: ms per call at grids 32 x 32 and 10 x 100, D = (2, 1), a
minibatch of 1000 rows of a resident data set (the fit) and N = 105 280 rows (cfg5's full batch, predictions and paths), in interleaved
windows.  Four arms per call:
  rbf fused        every factor RBF: the fused register-resident kernels (what an RBF model runs)
  rbf panels       every factor RBF, set_kron_panels(True): the GEMM-panel path
  m32 time panels  Matern32 time factor on both latents (routed to the panels by its kind)
  m52 both panels  Matern52 on all four factors
Calls: a gradient step and a value-only step (kron_elbo on rows of the resident set), kron_predict (host rows: it has no device form),
kron_sample_paths_device at S = 16 with R = 0 and R = 1024.  The path calls have no fused form: their 'rbf fused' and 'rbf panels' arms
are the same code and show the noise.
The honest comparison for the KERNEL cost is Matern-on-panels against RBF-on-panels; the gap from there to the fused RBF step is what a
fused Matern instantiation would buy.  The spread of an arm's windows is the box's run-to-run noise.

  python tools/kron_matern_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended to
                                            profiles/kron_matern_time.log (or to the file named by KRON_MATERN_LOG)
  python tools/kron_matern_time.py time     the timing step (child)
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
LOG = os.environ.get('KRON_MATERN_LOG') or os.path.join(ROOT, 'profiles', 'kron_matern_time.log')
N, BATCH, WINDOWS = 105280, 1000, 5
GRIDS = ((32, 32), (10, 100))
ARMS = (('rbf fused', 'rbf', False), ('rbf panels', 'rbf', True), ('m32 time panels', ('rbf', 'matern32'), False),
        ('m52 both panels', 'matern52', False))


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
    from zigp import pathwise
    e = zigp.DenseEngine(0)
    log('this build  D=(2, 1)  minibatch %d of N=%d resident rows; predictions and paths at N rows; %d interleaved windows (ms per call)' % (BATCH, N, WINDOWS))
    for grid in GRIDS:
        X, Y, p = kron_nd.make_kron_problem_nd(N, grid[0], grid[1], 2, 1, seed=5, c=0.5)
        e.set_data(X, Y)
        Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        out3 = torch.empty((3, 16, N), dtype=torch.float64, device='cuda:0')
        rs = np.random.RandomState(1)
        calls = []
        for name, kinds, panels in ARMS:
            q = dict(p, kern_f=kinds, kern_g=kinds)
            k2 = pathwise.kron_kinds(kinds)
            d0 = {t: pathwise.kron_draw(k2, 0, 2, 1, grid[0], grid[1], 16, rs) for t in 'fg'}
            d1 = {t: pathwise.kron_draw(k2, 1024, 2, 1, grid[0], grid[1], 16, rs) for t in 'fg'}

            def wrap(fn, panels=panels):
                def run():
                    e.set_kron_panels(panels)
                    try:
                        return fn()
                    finally:
                        e.set_kron_panels(False)
                return run
            calls += [
                (('gradient step', name), 20, wrap(lambda q=q: e.kron_elbo(q, rows=(0, BATCH), jitter=1e-5, scale=N / BATCH))),
                (('value-only step', name), 20, wrap(lambda q=q: e.kron_elbo(q, rows=(0, BATCH), jitter=1e-5, scale=N / BATCH, need_grad=False))),
                (('kron_predict (host rows)', name), 2, wrap(lambda q=q: e.kron_predict(q, X, jitter=1e-5))),
                (('sample_paths_device S=16 R=0', name), 5, wrap(lambda q=q, d=d0: e.kron_sample_paths_device(q, Xd, n_samples=16, draws=d, jitter=1e-5, out=out3))),
                (('sample_paths_device S=16 R=1024', name), 5, wrap(lambda q=q, d=d1: e.kron_sample_paths_device(q, Xd, n_samples=16, draws=d, jitter=1e-5, out=out3))),
            ]
        for _, _, fn in calls:
            fn(); fn()                               # warm-up: buffers, code objects
        ms = {k: [] for k, _, _ in calls}
        gc.collect()
        gc.disable()
        for _ in range(WINDOWS):
            for k, reps, fn in calls:
                t0 = time.time()
                for _ in range(reps):
                    fn()                             # every call ends in the library's stream synchronisation
                ms[k].append((time.time() - t0) / reps * 1e3)
        gc.enable()
        log('grid %d x %d' % grid)
        med = {k: median(v) for k, v in ms.items()}
        for call in dict.fromkeys(k[0] for k, _, _ in calls):
            for name, _, _ in ARMS:
                v = ms[(call, name)]
                log('  %-34s %-16s %9.3f (windows %s, spread %.3f)' % (call, name, med[(call, name)], ' '.join('%.3f' % x for x in v), max(v) - min(v)))
            base, fused = med[(call, 'rbf panels')], med[(call, 'rbf fused')]
            log('  %-34s Matern32 time / RBF on panels = %.2f, Matern52 both / RBF on panels = %.2f; panels / fused (RBF) = %.2f'
                % (call, med[(call, 'm32 time panels')] / base, med[(call, 'm52 both panels')] / base, base / fused))
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/kron_matern_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    cmd = ['timeout', '-k', '10', '540', sys.executable, os.path.abspath(__file__), 'time']
    rc = subprocess.call(cmd)
    if rc != 0:
        log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
    return rc


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time()
    else:
        sys.exit(driver())
