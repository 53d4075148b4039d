"""What a Lloyd iteration costs on the device, on one box: ms per iteration of DenseEngine.kmeans_resident at the cfg2 shape
(N = 1e5, M = 512, D = 3), the cfg3 shape (1e6 x 1024 x 3), D = 8 (1e6 x 1024 x 8) and D = 64 (1e5 x 512 x 64), from uniform random
rows and M sampled rows as the start.  A call's fixed cost (buffers, the start's upload, the results' download) is taken out by
differencing: ms per iteration = (time at max_iter = 17 - time at max_iter = 1) / 16; the arm checks that neither call stopped early.
The kernel's share of the fp64 vector rate counts N M (3 D - 1) operations per iteration (a subtraction, a multiply or fma per
dimension, D - 1 of them adds folded into the fma) against 78.6 TFLOP/s = 256 CU x 2.4 GHz x 128 flop / clk / CU (the microarchitecture
guide lists no fp64 vector row; this is the project's figure, equal to the fp64 matrix rate).
The owner scan's share of an iteration comes from a second build, -DZIGP_KMEANS_NO_SCAN (tools/build_variant.sh kmeans_noscan
-DZIGP_KMEANS_NO_SCAN): the step kernel without the scan, so no update and no stop -- timing only.  Its arms run when that library
exists, in the same interleaved windows, in a child process of their own (a process loads one libzigp.so).
Beside it the host route: scipy.cluster.vq.vq plus a NumPy update (bincount per column), one pass, on this box's CPU.

  python tools/kmeans_time.py          driver: each GPU step is a child process under its own `timeout`; everything is appended to
                                       profiles/kmeans_time.log (or to the file named by KMEANS_LOG)
  python tools/kmeans_time.py time     the timing step (child; the library is the one ZIGP_LIB names, else the product build)
  python tools/kmeans_time.py host     the host route (child, no GPU)
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('KMEANS_LOG') or os.path.join(ROOT, 'profiles', 'kmeans_time.log')
VARIANT = os.path.join(ROOT, 'zero-inflated-gp_amd', 'lib', 'libzigp_kmeans_noscan.so')
SHAPES = (('cfg2', 100000, 512, 3), ('cfg3', 1000000, 1024, 3), ('D=8', 1000000, 1024, 8), ('D=64', 100000, 512, 64))
K1, K2, WINDOWS = 1, 17, 5
PEAK = 78.6e12


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def problem(N, M, D):
    rs = np.random.RandomState(N % 1000 + M + D)
    X = rs.rand(N, D)
    return X, np.ascontiguousarray(X[rs.choice(N, M, replace=False)])


def child_time():
    import zigp
    from zigp import _lib
    variant = os.path.abspath(_lib.LIB_PATH) == os.path.abspath(VARIANT)
    log('library %s  %d interleaved windows per shape, ms per iteration = (t[max_iter=%d] - t[max_iter=%d]) / %d'
        % ('-DZIGP_KMEANS_NO_SCAN (no owner scan, no update)' if variant else 'product build', WINDOWS, K2, K1, K2 - K1))
    e = zigp.DenseEngine(0)
    for name, N, M, D in SHAPES:
        X, C0 = problem(N, M, D)
        e.set_data(X, np.zeros(N))

        def run(K):
            t0 = time.time()
            _, info = e.kmeans_resident(M, init=C0, max_iter=K, return_info=True)      # ends in the library's stream synchronisation
            if not variant and info['n_iter'] != K:
                raise RuntimeError('%s stopped after %d of %d iterations: the difference would not be %d iterations' % (name, info['n_iter'], K, K2 - K1))
            return (time.time() - t0) * 1e3
        run(K1); run(K2)                        # warm-up: code objects, the pinned arena
        per = []
        for _ in range(WINDOWS):
            a, b = run(K1), run(K2)
            per.append((b - a) / (K2 - K1))
        ms = median(per)
        flops = float(N) * M * (3 * D - 1)
        log('  %-5s N=%-8d M=%-5d D=%-3d %9.3f ms / iteration (windows %s, spread %.3f)  %.2f TFLOP/s = %.3f of the fp64 vector rate'
            % (name, N, M, D, ms, ' '.join('%.3f' % v for v in per), max(per) - min(per), flops / (ms * 1e-3) / 1e12, flops / (ms * 1e-3) / PEAK))
    e.close()


def child_host():
    from scipy.cluster.vq import vq
    log('host route: scipy.cluster.vq.vq + NumPy update, one pass each (ms); %d CPUs visible, OMP_NUM_THREADS=%s (vq runs on one thread)'
        % (os.cpu_count(), os.environ.get('OMP_NUM_THREADS', 'unset')))
    for name, N, M, D in SHAPES[:2]:
        X, C0 = problem(N, M, D)
        t0 = time.time()
        lab, _ = vq(X, C0)
        t1 = time.time()
        cnt = np.bincount(lab, minlength=M)
        Cn = np.stack([np.bincount(lab, weights=X[:, k], minlength=M) for k in range(D)], axis=1) / np.maximum(cnt, 1)[:, None]
        t2 = time.time()
        log('  %-5s N=%-8d M=%-5d D=%-3d vq %9.1f  update %7.1f' % (name, N, M, D, (t1 - t0) * 1e3, (t2 - t1) * 1e3))


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/kmeans_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    steps = [(dict(), 'time', '300')]
    if os.path.exists(VARIANT):
        steps.append((dict(ZIGP_LIB=VARIANT), 'time', '300'))
    else:
        log('no %s: the owner scan\'s share is not measured in this run' % os.path.relpath(VARIANT, ROOT))
    steps.append((dict(), 'host', '300'))
    for env, what, limit in steps:
        cmd = ['timeout', '-k', '10', limit, sys.executable, os.path.abspath(__file__), what]
        rc = subprocess.call(cmd, env=dict(os.environ, **env))
        if rc != 0:
            log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
            return rc
    return 0


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time()
    elif len(sys.argv) >= 2 and sys.argv[1] == 'host':
        child_host()
    else:
        sys.exit(driver())
