"""Per-iteration time of minibatch Adam on the whitened dense models: the host loop (select_rows + zigp_elbo + a download + AdamGroups
in NumPy + an upload per iteration: what OnOffSVGP.optimize(method='adam') runs for whiten=True) against the loop on the device
(zigp.optim.WhiteDeviceFit -> zigp_fit_steps_mode: one synchronisation per ITERS iterations: optimize(..., device_loop=True)).

Four cases: the whitened diagonal q(u) and the full-covariance q(u) (q_diag=False), each at the toy shape (tests/golden/toydata.mat:
N = 450, D = 1, M = 50, batch 100) and at M = 1024, D = 3, batch 1024 (bench.synth, N = 100 000 resident rows).

  python tools/white_fit_time.py                     driver: one child process per case under its own `timeout`, chained (the first one
                                                     that fails ends the run); everything is appended to profiles/white_fit_time.log (or to
                                                     the file named by WHITE_FIT_LOG)
  python tools/white_fit_time.py case SHAPE MODEL    one case (child): SHAPE toy | m1024, MODEL diag | full

Both loops run in the same process on the same engine, interleaved: after one warm-up window each, WINDOWS (5) alternating windows of
ITERS (200) iterations; every window restarts from the same initial parameters, zero moments and the same row samples, so both do the
same iterations, and ends in the library's stream synchronisation.  Reported: the median over the windows in ms per iteration, the
windows themselves and their spread (max - min), and how far the two loops' last data terms are apart.  Profiler off.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('WHITE_FIT_LOG') or os.path.join(ROOT, 'profiles', 'white_fit_time.log')
ITERS, WINDOWS = int(os.environ.get('WHITE_FIT_ITERS', 200)), int(os.environ.get('WHITE_FIT_WINDOWS', 5))
KEYS = ('Zf', 'Zg', 'u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')
POSITIVE = KEYS[4:]


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def problem(shape):
    """(X, Y, parameter dict of the diagonal model, batch)"""
    import numpy as np
    if shape == 'toy':
        import scipy.io as sio
        mat = sio.loadmat(os.path.join(ROOT, 'tests', 'golden', 'toydata.mat'))
        X, Y = np.asarray(mat['x'], dtype=np.float64), np.asarray(mat['y'], dtype=np.float64)
        M = 50
        Z = np.linspace(X.min(), X.max(), M + 1, endpoint=False)[1:].reshape(-1, 1)
        rs = np.random.RandomState(1)
        p = dict(Zf=Z, Zg=Z.copy(), u_fm=0.01 * rs.randn(M), u_gm=0.01 * rs.randn(M), u_fs_sqrt=np.ones(M), u_gs_sqrt=np.ones(M),
                 ell_f=np.array([1.0]), ell_g=np.array([1.0]), var_f=1.0, var_g=5.0, noise=0.01)
        return X, Y, p, 100
    import bench
    X, Y, p = bench.synth(100000, 1024, 3)
    return X, Y, p, 1024


def make_pset(p, full, lr=0.01):
    import collections
    import numpy as np
    from zigp.optim import P, ParamSet
    from zigp.transforms import Log1pe, Identity, LowerTriangular
    q = collections.OrderedDict()
    for k in KEYS:
        v = np.atleast_1d(np.array(p[k], dtype=np.float64))
        if full and k in ('u_fs_sqrt', 'u_gs_sqrt'):      # the model's starting point: diag(s)
            q[k] = P(np.diag(v.reshape(-1)), LowerTriangular(v.size), learning_rate=lr, name=k)
        else:
            q[k] = P(v, Log1pe() if k in POSITIVE else Identity(), learning_rate=lr, name=k)
    return ParamSet(q)


def values(pset, full):
    out = {k: q.value for k, q in pset.params.items()}
    for k in ('var_f', 'var_g', 'noise'):
        out[k] = float(out[k].reshape(-1)[0])
    out['whiten'] = True
    if full:
        out['q_diag'] = False
    return out


def child_case(shape, model):
    import numpy as np
    import zigp
    from zigp.optim import AdamGroups, WhiteDeviceFit
    full = model == 'full'
    X, Y, p, batch = problem(shape)
    N, M = X.shape[0], np.asarray(p['Zf']).shape[0]
    eng = zigp.DenseEngine(0)
    eng.set_data(X, Y)
    rows = np.random.RandomState(3).randint(N, size=(ITERS, batch))
    scale = float(N) / batch

    def host():
        pset = make_pset(p, full)
        opt = AdamGroups(pset)
        last = None
        for i in range(ITERS):
            eng.select_rows(rows[i])
            ed, kl, g = eng.elbo(values(pset, full), jitter=1e-6, scale=scale)
            last = ed
            opt.step({k: np.atleast_1d(g[k]) for k in KEYS})
        eng.select_rows(None)
        return last

    def device():
        pset = make_pset(p, full)
        ed, kl = WhiteDeviceFit(eng, pset).steps(rows, batch, 1e-6, scale)
        return ed[-1]

    loops = (('host loop', host), ('device loop', device))
    last = [fn() for name, fn in loops]      # warm-up: code objects, buffers, tile lists of both loops
    ms = [[], []]
    for _ in range(WINDOWS):
        for k, (name, fn) in enumerate(loops):
            t0 = time.time()
            last[k] = fn()
            ms[k].append((time.time() - t0) / ITERS * 1e3)
    med = [sorted(v)[len(v) // 2] for v in ms]
    log('%s %s  N=%d M=%d D=%d batch %d  %d interleaved windows of %d iterations per loop (ms per iteration)'
        % (shape, model, N, M, X.shape[1], batch, WINDOWS, ITERS))
    for k, (name, fn) in enumerate(loops):
        log('  %-12s %8.4f  (windows %s; spread %.4f; last data term %.10e)'
            % (name, med[k], ' '.join('%.4f' % v for v in ms[k]), max(ms[k]) - min(ms[k]), last[k]))
    log('  host / device %.2f; difference %.4f ms per iteration; last data terms %.1e apart (relative)'
        % (med[0] / med[1], med[0] - med[1], abs(last[0] - last[1]) / abs(last[0])))
    eng.close()


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/white_fit_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    me = os.path.abspath(__file__)
    for shape, limit in (('toy', '120'), ('m1024', '300')):
        for model in ('diag', 'full'):      # chained: nothing more is started on the GPU after a step that failed
            cmd = ['timeout', '-k', '10', limit, sys.executable, me, 'case', shape, model]
            rc = subprocess.call(cmd)
            if rc != 0:
                log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
                return rc
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'case':
        child_case(sys.argv[2], sys.argv[3])
    else:
        sys.exit(driver())
