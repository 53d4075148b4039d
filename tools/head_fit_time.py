"""Per-iteration time of the heads' fit loop: fit_head(device_loop=True) of this tree (zigp_kron_head_fit_steps: one synchronisation per
100 iterations) against fit_head as the PARENT commit runs it (one zigp_kron_head_elbo call, one download and a NumPy Adam step per
iteration), on the pptr training set (tests/golden/pptr.npz, 105 280 rows), batch 1000, inducing grids 32 x 32 and 10 x 100, Gaussian and
Bernoulli head.

  python tools/head_fit_time.py                           driver: per shape two worker processes (this tree, the parent tree), each warmed
                                                          once, then WINDOWS alternating windows of ITERS iterations; everything is
                                                          appended to profiles/head_fit_ab.log (or the file named by HEAD_FIT_LOG)
  python tools/head_fit_time.py worker ROOT M0 M1 LIK DEV the worker: ROOT = a zero-inflated-gp_amd folder (package + built library), DEV =
                                                          1 passes device_loop=True; runs one window per line read from stdin

The parent tree (library and Python of the parent commit) is expected in build/parent (git-ignored), or where HEAD_FIT_PARENT points:
  mkdir -p build/parent && git archive <parent> zero-inflated-gp_amd include | tar -x -C build/parent
  (cd build/parent && python -c "import sys; sys.path.insert(0, 'zero-inflated-gp_amd'); from zigp import build; build.build(force=True)")
Every window ends in the library's stream synchronisation and re-starts from the same initial parameters and the same DataSet seed, so
both variants do the same iterations.  The figure to read: the difference of the two medians against the spread (max - min) of the
windows of either variant.  Profiler off.  A worker that ends early ends the run; nothing is retried.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.environ.get('HEAD_FIT_LOG') or os.path.join(ROOT, 'profiles', 'head_fit_ab.log')
PARENT = os.environ.get('HEAD_FIT_PARENT') or os.path.join(ROOT, 'build', 'parent', 'zero-inflated-gp_amd')
SHAPES = [((32, 32), 'gaussian'), ((32, 32), 'bernoulli'), ((10, 100), 'gaussian'), ((10, 100), 'bernoulli')]
BATCH, ITERS, WINDOWS = 1000, int(os.environ.get('HEAD_FIT_ITERS', 3000)), int(os.environ.get('HEAD_FIT_WINDOWS', 5))


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def worker(root, grid, lik, dev):
    sys.path.insert(0, root)
    import copy
    import logging
    import numpy as np
    import zigp
    from onofftf.heads import fit_head, init_head_params
    assert os.path.dirname(os.path.abspath(zigp.__file__)).startswith(os.path.abspath(root))
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'pptr.npz'))
    X, Y = d['Xtrain'].copy(), d['Ytrain']
    X[:, 2] /= 1000.0
    if lik == 'bernoulli':
        Y = (Y > 0) * 1.0
    pset0 = init_head_params(X, grid, lik, include_f_mu=(lik == 'bernoulli'), kmeans_seed=1, rng=np.random.RandomState(4))
    eng = zigp.reference_engine(0)
    logger = logging.getLogger('head_fit_time')
    logger.addHandler(logging.NullHandler())
    kw = dict(device_loop=True) if dev else {}
    print('ready', flush=True)
    for line in sys.stdin:
        n = int(line)
        pset, hist = copy.deepcopy(pset0), []
        t0 = time.time()
        fit_head(pset, lik, X, Y, n, BATCH, logger, eng=eng, history=hist, **kw)
        dt = time.time() - t0
        assert len(hist) == n and np.all(np.isfinite(hist))
        print('%.6f %.10e' % (dt / n * 1e3, hist[-1]), flush=True)
    eng.close()


def ask(p, n):
    p.stdin.write('%d\n' % n)
    p.stdin.flush()
    line = p.stdout.readline()
    if not line:
        raise RuntimeError('a worker ended early (exit status %s)' % p.wait())
    return [float(q) for q in line.split()]


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    if not os.path.exists(os.path.join(PARENT, 'lib', 'libzigp.so')):
        sys.exit('no parent build at %s (see the module docstring)' % PARENT)
    log('# tools/head_fit_time.py  %s  batch %d, %d windows of %d iterations per variant, alternating (ms per iteration)'
        % (time.strftime('%Y-%m-%d %H:%M:%S'), BATCH, WINDOWS, ITERS))
    me = os.path.abspath(__file__)
    roots = (('parent host loop', PARENT, 0), ('device loop', os.path.join(ROOT, 'zero-inflated-gp_amd'), 1))
    for grid, lik in SHAPES:
        ps = []
        try:
            for name, root, dev in roots:      # each worker under its own time limit
                ps.append(subprocess.Popen(['timeout', '-k', '10', '420', sys.executable, me, 'worker', root, str(grid[0]), str(grid[1]), lik, str(dev)],
                                           stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True))
            for p in ps:
                if p.stdout.readline().strip() != 'ready':
                    raise RuntimeError('a worker did not start (exit status %s)' % p.wait())
            for p in ps:
                ask(p, 300)                    # warm-up: code objects, buffers, the resident data set
            ms, last = [[], []], [None, None]
            for _ in range(WINDOWS):
                for k, p in enumerate(ps):
                    t, last[k] = ask(p, ITERS)
                    ms[k].append(t)
        except RuntimeError as e:
            log('%dx%d %s: %s -- stopping' % (grid[0], grid[1], lik, e))
            for p in ps:
                p.kill()
            return 1
        for p in ps:
            p.stdin.close()
            p.wait()
        med = [sorted(v)[len(v) // 2] for v in ms]
        spread = [max(v) - min(v) for v in ms]
        for k, (name, root, dev) in enumerate(roots):
            log('%dx%d %-9s %-16s %7.4f  (windows %s; spread %.4f; last cost %.8e)'
                % (grid[0], grid[1], lik, name, med[k], ' '.join('%.4f' % v for v in ms[k]), spread[k], last[k]))
        log('%dx%d %-9s difference %.4f ms per iteration (ratio %.2f), largest spread %.4f'
            % (grid[0], grid[1], lik, med[0] - med[1], med[0] / med[1], max(spread)))
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 7 and sys.argv[1] == 'worker':
        worker(sys.argv[2], (int(sys.argv[3]), int(sys.argv[4])), sys.argv[5], sys.argv[6] == '1')
    else:
        sys.exit(driver())
