"""What the fused Matern kernels buy (DenseEngine.set_kron_matern_fused), on one box, same build: the protocol of tools/kron_matern_time.py
-- ms per call at grids 32 x 32 and 10 x 100, D = (2, 1), a minibatch of 1000 rows of a resident data set and kron_predict of N = 105 280
host rows, interleaved windows -- with the arms
  rbf fused        every factor RBF on the fused kernels (what an RBF model runs)
  m32 time panels  Matern32 time factor on both latents, switch off: the GEMM panels
  m32 time fused   the same model, switch on: the _kinds kernels
  m52 both panels  Matern52 on all four factors, switch off
  m52 both fused   the same model, switch on
Calls: a gradient step and a value-only step (kron_elbo on rows of the resident set) and kron_predict.  Then the fit loop of the Matern32
time model per iteration: the device loop (zigp_kron_fit_steps, 200 iterations a call, switch on) against the host Adam loop (one
kron_stepper call + AdamGroups step per iteration) with the switch off (what such a model ran before) and on.
The claim to test: fused beats panels by more than the windows' spread on the minibatch gradient step at both grids.

  python tools/kron_matern_fused_time.py          driver: the GPU step is a child process under its own `timeout`; everything is appended
                                                  to profiles/kron_matern_fused_time.log (or to the file named by KRON_MATERN_LOG)
  python tools/kron_matern_fused_time.py time     the timing step (child)
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
LOG = os.environ.get('KRON_MATERN_LOG') or os.path.join(ROOT, 'profiles', 'kron_matern_fused_time.log')
N, BATCH, WINDOWS = 105280, 1000, 5
GRIDS = ((32, 32), (10, 100))
M32, M52 = ('rbf', 'matern32'), 'matern52'
ARMS = (('rbf fused', 'rbf', False), ('m32 time panels', M32, False), ('m32 time fused', M32, True), ('m52 both panels', M52, False),
        ('m52 both fused', M52, True))


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def fit_loops(e, X, Y, grid):
    """ms per iteration of the Matern32-time model's fit: device loop (switch on) and host loop (switch off, on), WINDOWS windows each"""
    from onofftf.model import init_params, engine_params, named_grads, set_kernels, KronDeviceFit
    from zigp.optim import AdamGroups

    def pset():
        ps = init_params(X[:4000], grid, grid, kmeans_seed=3, rng=np.random.RandomState(9))
        set_kernels(ps, M32)
        return ps

    rs = np.random.RandomState(4)
    scale = N / BATCH
    e.set_data(X, Y)
    out = {}
    e.set_kron_matern_fused(True)
    try:
        fit = KronDeviceFit(e, pset())
        seq = [int(r) for r in rs.randint(0, N - BATCH, size=200)]
        fit.steps(seq, BATCH, 1e-5, scale)            # warm-up
        v = []
        for _ in range(WINDOWS):
            t0 = time.time()
            fit.steps(seq, BATCH, 1e-5, scale)
            v.append((time.time() - t0) / len(seq) * 1e3)
        out['device loop, fused'] = v
    finally:
        e.set_kron_matern_fused(False)
    for name, on in (('host loop, panels', False), ('host loop, fused', True)):
        e.set_kron_matern_fused(on)
        try:
            ps = pset()
            opt, step = AdamGroups(ps), e.kron_stepper(engine_params(ps))
            seq = [int(r) for r in rs.randint(0, N - BATCH, size=30)]
            v = []
            for w in range(WINDOWS + 1):
                t0 = time.time()
                for rb in seq:
                    ed, kl, g = step(engine_params(ps), rows=(rb, rb + BATCH), jitter=1e-5, scale=scale)
                    opt.step(named_grads(g))
                if w:                                   # window 0 is the warm-up
                    v.append((time.time() - t0) / len(seq) * 1e3)
            out[name] = v
        finally:
            e.set_kron_matern_fused(False)
    for name, v in out.items():
        log('  %-34s %-18s %9.3f ms per iteration (windows %s, spread %.3f)' % ('fit loop, Matern32 time factor', name, median(v), ' '.join('%.3f' % x for x in v), max(v) - min(v)))
    log('  %-34s host panels / device fused = %.1f, host fused / device fused = %.1f'
        % ('fit loop, Matern32 time factor', median(out['host loop, panels']) / median(out['device loop, fused']),
           median(out['host loop, fused']) / median(out['device loop, fused'])))


def child_time():
    import zigp
    import kron_nd
    e = zigp.DenseEngine(0)
    log('this build  D=(2, 1)  minibatch %d of N=%d resident rows; kron_predict at N host rows; %d interleaved windows (ms per call)' % (BATCH, N, WINDOWS))
    for grid in GRIDS:
        X, Y, p = kron_nd.make_kron_problem_nd(N, grid[0], grid[1], 2, 1, seed=5, c=0.5)
        e.set_data(X, Y)
        calls = []
        for name, kinds, on in ARMS:
            q = dict(p, kern_f=kinds, kern_g=kinds)

            def wrap(fn, on=on):
                def run():
                    e.set_kron_matern_fused(on)
                    try:
                        return fn()
                    finally:
                        e.set_kron_matern_fused(False)
                return run
            calls += [
                (('gradient step', name), 20, wrap(lambda q=q: e.kron_elbo(q, rows=(0, BATCH), jitter=1e-5, scale=N / BATCH))),
                (('value-only step', name), 20, wrap(lambda q=q: e.kron_elbo(q, rows=(0, BATCH), jitter=1e-5, scale=N / BATCH, need_grad=False))),
                (('kron_predict (host rows)', name), 2, wrap(lambda q=q: e.kron_predict(q, X, jitter=1e-5))),
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
            rbf = med[(call, 'rbf fused')]
            log('  %-34s panels / fused: Matern32 time %.2f, Matern52 both %.2f; fused Matern / fused RBF: Matern32 time %.2f, Matern52 both %.2f'
                % (call, med[(call, 'm32 time panels')] / med[(call, 'm32 time fused')], med[(call, 'm52 both panels')] / med[(call, 'm52 both fused')],
                   med[(call, 'm32 time fused')] / rbf, med[(call, 'm52 both fused')] / rbf))
        fit_loops(e, X, Y, grid)
    e.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/kron_matern_fused_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
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
