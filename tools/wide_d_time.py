"""The dense path at input dimensions beyond 8 on one box, same build: gradient step, value-only ELBO and predict_device at the cfg2
shape (N = 1e5, M = 512) for D in {8, 9, 16, 32, 64}, in interleaved windows (D = 8 is the last dimension of the kernels specialised
per dimension, the yardstick of the same run); the gradient step of D >= 9 also with the inducing inputs of one coordinate spread
beyond KG_EXACT_SPREAD lengthscales, which selects the sliced per-row Kuf gradient instead of the moments product on the GEMM core;
and the per-kernel times of the wide kernels from a rocprofv3 kernel trace taken in a run of its own.

  python tools/wide_d_time.py                 driver: each GPU step is a child process under its own `timeout`, the steps are chained
                                              (the first one that fails ends the run); everything is appended to profiles/wide_d_time.log
                                              (or to the file named by WIDE_D_LOG)
  python tools/wide_d_time.py time            the timing step (child)
  python tools/wide_d_time.py traced D        the workload of the traced step: a few gradient steps at dimension D, both forms
  python tools/wide_d_time.py stats DIR D     per-kernel summary of that trace
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('WIDE_D_LOG') or os.path.join(ROOT, 'profiles', 'wide_d_time.log')
N, M, REPS, WINDOWS = 100000, 512, 20, 5
DIMS = (8, 9, 16, 32, 64)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def problem(D, spread=False):
    """bench.synth's generator at dimension D with lengthscales that keep Kuf away from 0 and 1 (ell ~ sqrt(D)); spread: coordinate 0 of
    the inducing inputs and of the data stretched over 4000 lengthscales (the per-row form of the Kuf gradient)"""
    import bench
    X, Y, p = bench.synth(N, M, D)
    d = np.arange(D)
    p['ell_f'] = 0.25 * np.sqrt(D) * (1 + 0.1 * (d % 5))
    p['ell_g'] = 0.33 * np.sqrt(D) * (1 + 0.05 * (d % 7))
    if spread:
        s = 4000.0 * p['ell_f'][0]
        X = X.copy()
        X[:, 0] *= s
        p = dict(p, Zf=p['Zf'].copy(), Zg=p['Zg'].copy())
        p['Zf'][:, 0] *= s
        p['Zg'][:, 0] *= s
    return np.ascontiguousarray(X), Y, p


def child_time():
    import torch
    import zigp
    e = zigp.DenseEngine(0)
    data = {}
    for D in DIMS:
        X, Y, p = problem(D)
        data[D] = (torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), p)
    out = torch.empty((9, N), dtype=torch.float64, device='cuda:0')

    def use(D):
        Xd, Yd, p = data[D]
        e.set_data_device(Xd, Yd)
        return Xd, p

    passes = (('gradient step', lambda Xd, p: e.elbo(p)), ('value-only ELBO', lambda Xd, p: e.elbo(p, need_grad=False)),
              ('predict_device', lambda Xd, p: e.predict_device(p, Xd, out=out)))
    log('N=%d M=%d  %d interleaved windows of %d calls per dimension (ms per call; D = 8 runs the kernels specialised per dimension)' % (
        N, M, WINDOWS, REPS))
    for label, fn in passes:
        for D in DIMS:
            Xd, p = use(D)
            fn(Xd, p); fn(Xd, p)                 # warm-up: tile lists, buffers, code objects
        ms = {D: [] for D in DIMS}
        for _ in range(WINDOWS):
            for D in DIMS:
                Xd, p = use(D)
                t0 = time.time()
                for _ in range(REPS):
                    fn(Xd, p)                    # every call ends in the library's stream synchronisation
                ms[D].append((time.time() - t0) / REPS * 1e3)
        med = {D: sorted(v)[len(v) // 2] for D, v in ms.items()}
        for D in DIMS:
            log('  %-16s D=%-2d %8.3f (windows %s, spread %.3f)  %.3f x the D = 8 figure' % (
                label, D, med[D], ' '.join('%.3f' % v for v in ms[D]), max(ms[D]) - min(ms[D]), med[D] / med[8]))
    # the sliced per-row Kuf gradient against the moments product, same dimension, interleaved
    for D in DIMS[1:]:
        Xs, Ys, ps = problem(D, spread=True)
        Xsd, Ysd = torch.from_numpy(Xs).cuda(), torch.from_numpy(Ys).cuda()
        arms = {'moments product': data[D], 'sliced per-row': (Xsd, Ysd, ps)}
        ms = {k: [] for k in arms}
        for k, (Xd, Yd, p) in arms.items():
            e.set_data_device(Xd, Yd); e.elbo(p); e.elbo(p)
        for _ in range(WINDOWS):
            for k, (Xd, Yd, p) in arms.items():
                e.set_data_device(Xd, Yd)
                t0 = time.time()
                for _ in range(REPS):
                    e.elbo(p)
                ms[k].append((time.time() - t0) / REPS * 1e3)
        for k in arms:
            v = ms[k]
            log('  gradient step    D=%-2d %-16s %8.3f (windows %s, spread %.3f)' % (D, k, sorted(v)[len(v) // 2], ' '.join('%.3f' % x for x in v), max(v) - min(v)))
    e.close()


def child_traced(D):
    import torch
    import zigp
    e = zigp.DenseEngine(0)
    for spread in (False, True):
        X, Y, p = problem(D, spread)
        e.set_data_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
        for _ in range(3):
            e.elbo(p)
    e.close()


def child_stats(d, D):
    import collections
    import csv
    import glob
    f = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)[0]
    t, n = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(f)):
        k = r['Kernel_Name'].split('(')[0]
        k = k[k.find('gemm_f64_kernel'):] if 'gemm_f64_kernel' in k else k[-48:]
        t[k] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        n[k] += 1
    log('D=%d kernel trace: 3 gradient steps with the moments product + 3 with the sliced per-row Kuf gradient' % D)
    for k in sorted(t, key=t.get, reverse=True)[:14]:
        log('  %-74s %5d launches  avg %9.1f us' % (k[:74], n[k], t[k] / n[k]))


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/wide_d_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    me = os.path.abspath(__file__)
    out = os.environ.get('WIDE_D_TRACE_DIR') or os.path.join(ROOT, 'collect_out', 'wide_d_trace')     # rocprofv3 output (git-ignored)
    steps = [['timeout', '-k', '10', '400', sys.executable, me, 'time']]
    for D in (16, 64):
        d = os.path.join(out, 'D%d' % D)
        steps.append(['timeout', '-k', '10', '240', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--',
                      sys.executable, me, 'traced', str(D)])
        steps.append(['timeout', '-k', '10', '60', sys.executable, me, 'stats', d, str(D)])
    for cmd in steps:                             # chained: nothing more is started on the GPU after a step that failed
        rc = subprocess.call(cmd)
        if rc != 0:
            log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
            return rc
    return 0


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time()
    elif len(sys.argv) >= 3 and sys.argv[1] == 'traced':
        child_traced(int(sys.argv[2]))
    elif len(sys.argv) >= 4 and sys.argv[1] == 'stats':
        child_stats(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(driver())
