"""Full-covariance (zigp_set_q_full, q_diag=False on the whitened model) against unwhitened diagonal passes of the dense path on one
box: gradient step, value-only ELBO and predict_device at cfg3 (N = 1e6, M = 1024, D = 3) and cfg2 (N = 1e5, M = 512), in interleaved
windows; then the per-kernel times of a full-covariance run from a rocprofv3 kernel trace taken in a run of its own.

  python tools/fullcov_time.py                 driver: each GPU step is a child process under its own `timeout`, the steps are chained
                                               (the first one that fails ends the run); everything is appended to profiles/fullcov_ab.log
                                               (or to the file named by FULLCOV_LOG)
  python tools/fullcov_time.py time cfg3       one timing step (child)
  python tools/fullcov_time.py traced cfg3     the workload of the traced step: a few full-covariance calls (run under rocprofv3 by the driver)
  python tools/fullcov_time.py stats DIR cfg3  per-kernel summary of that trace

The baseline is the unwhitened diagonal pass.  With FULLCOV_PARENT_LIB=<libzigp.so built from the parent commit> the driver adds a
timing step with ZIGP_LIB pointing there, whose "unwhitened" lines are the parent's numbers (its full-covariance lines fail by design
and are not run).  The chunk loop of a full-covariance call launches the unwhitened kernels on other operands (8 M^2 N per gradient
step, 4 M^2 N value-only / predict: flop ratio 1), so the expectation is parity plus the M x M additions (four split-K M^3 products
per latent and step, the staging / KL / assembly kernels) and the two 8 MB transfers per latent at M = 1024.
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('FULLCOV_LOG') or os.path.join(ROOT, 'profiles', 'fullcov_ab.log')
CFG = {'cfg3': (1000000, 1024, 3, 5), 'cfg2': (100000, 512, 3, 40)}      # N, M, D, calls per window
WINDOWS = 5


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def problem(name):
    import bench
    N, M, D, reps = CFG[name]
    X, Y, p = bench.synth(N, M, D)
    p['u_fs_sqrt'] = p['u_fs_sqrt'] * 0.8
    p['u_gs_sqrt'] = p['u_gs_sqrt'] * 1.2
    return N, M, reps, X, Y, p


def full(p, M):
    """the full-covariance point next to p: Lq = diag(s) + (0.1 / sqrt(M)) tril(randn, -1), as in the parity tests"""
    import numpy as np
    rs = np.random.RandomState(0)
    q = dict(p, whiten=True, q_diag=False)
    for k in ('u_fs_sqrt', 'u_gs_sqrt'):
        q[k] = np.diag(np.asarray(p[k], dtype=np.float64).reshape(-1)) + (0.1 / np.sqrt(M)) * np.tril(rs.randn(M, M), -1)
    return q


def child_time(name):
    import torch
    import zigp
    N, M, reps, X, Y, p = problem(name)
    e = zigp.DenseEngine(0)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    e.set_data_device(Xd, Yd)
    out = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    modes = (False,) if os.environ.get('FULLCOV_BASELINE_ONLY') else (False, True)
    q = {False: p, True: full(p, M)}
    passes = (('gradient step', lambda w: e.elbo(q[w]), 8.0, 8.0),
              ('value-only ELBO', lambda w: e.elbo(q[w], need_grad=False), 4.0, 4.0),
              ('predict_device', lambda w: e.predict_device(q[w], Xd, out=out), 4.0, 4.0))
    log('%s  N=%d M=%d  %d interleaved windows of %d calls per mode (ms per call)' % (name, N, M, WINDOWS, reps))
    for label, fn, fl_u, fl_w in passes:
        for w in modes:
            fn(w); fn(w)                         # warm-up: tile lists, buffers, code objects of both modes
        ms = {w: [] for w in modes}
        for _ in range(WINDOWS):
            for w in modes:
                t0 = time.time()
                for _ in range(reps):
                    fn(w)                        # every call ends in the library's stream synchronisation
                ms[w].append((time.time() - t0) / reps * 1e3)
        med = {w: sorted(v)[len(v) // 2] for w, v in ms.items()}
        spread = {w: max(v) - min(v) for w, v in ms.items()}
        fl = 2 * M * M * float(N)                # two latents x M^2 N
        log('  %-16s unwhitened %8.3f (windows %s, spread %.3f; %.1f TFLOP/s of %g M^2 N)' % (
            label, med[False], ' '.join('%.3f' % v for v in ms[False]), spread[False], fl_u * fl / med[False] / 1e9, fl_u))
        if True not in modes:
            continue
        log('  %-16s full-cov   %8.3f (windows %s, spread %.3f; %.1f TFLOP/s of %g M^2 N)' % (
            '', med[True], ' '.join('%.3f' % v for v in ms[True]), spread[True], fl_w * fl / med[True] / 1e9, fl_w))
        log('  %-16s ratio %.3f (flop ratio %.2f); difference %.3f ms per call' % ('', med[True] / med[False], fl_w / fl_u, med[True] - med[False]))
    e.close()


def child_traced(name):
    import torch
    import zigp
    N, M, reps, X, Y, p = problem(name)
    e = zigp.DenseEngine(0)
    Xd = torch.from_numpy(X).cuda()
    e.set_data_device(Xd, torch.from_numpy(Y).cuda())
    p = full(p, M)
    for _ in range(3):
        e.elbo(p)
        e.elbo(p, need_grad=False)
    e.close()


def child_stats(d, name):
    """Per-kernel time of the trace's top kernels."""
    import collections
    import csv
    import glob
    N, M, _, _ = CFG[name]
    f = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)[0]
    t, n = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(f)):
        k = r['Kernel_Name'].split('(')[0]
        k = k[k.find('gemm_f64_kernel'):] if 'gemm_f64_kernel' in k else k[-48:]
        t[k] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        n[k] += 1
    log('%s kernel trace: 3 full-covariance gradient steps + 3 value-only passes' % name)
    new = ('k_lq_stage', 'k_kl_white_full', 'k_sub_eye', 'k_dlq_assemble', 'k_pack_square')
    for k in sorted(t, key=t.get, reverse=True)[:12] + [k for k in t if any(q in k for q in new)]:
        line = '  %-74s %5d launches  avg %9.1f us' % (k[:74], n[k], t[k] / n[k])
        log(line)


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/fullcov_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    me = os.path.abspath(__file__)
    out = os.environ.get('FULLCOV_TRACE_DIR') or os.path.join(ROOT, 'collect_out', 'fullcov_trace')     # rocprofv3 output (git-ignored)
    steps = []
    for name in ('cfg3', 'cfg2'):
        steps.append(['timeout', '-k', '10', '240', sys.executable, me, 'time', name])
    parent = os.environ.get('FULLCOV_PARENT_LIB')
    if parent:                                    # the parent commit's unwhitened passes, same box, same session
        for name in ('cfg3', 'cfg2'):
            steps.append(['timeout', '-k', '10', '240', 'env', 'ZIGP_LIB=' + parent, 'FULLCOV_BASELINE_ONLY=1', sys.executable, me, 'time', name])
    for name in ('cfg3', 'cfg2'):
        d = os.path.join(out, name)
        steps.append(['timeout', '-k', '10', '240', 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--',
                      sys.executable, me, 'traced', name])
        steps.append(['timeout', '-k', '10', '60', sys.executable, me, 'stats', d, name])
    for cmd in steps:                             # chained: nothing more is started on the GPU after a step that failed
        rc = subprocess.call(cmd)
        if rc != 0:
            log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
            return rc
    return 0


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'time':
        child_time(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == 'traced':
        child_traced(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == 'stats':
        child_stats(sys.argv[2], sys.argv[3])
    else:
        sys.exit(driver())
