"""Whitened against unwhitened passes of the dense path on one box, same build: gradient step, value-only ELBO and predict_device at
cfg3 (N = 1e6, M = 1024, D = 3) and cfg2 (N = 1e5, M = 512), in interleaved windows; and the per-kernel rates of the two launches only a
whitened call has -- the upper-triangular J' = (W^T D) A and the store-less A = W K -- from a rocprofv3 kernel trace taken in a run of
its own.

  python tools/whiten_time.py                 driver: each GPU step is a child process under its own `timeout`, the steps are chained
                                              (the first one that fails ends the run); everything is appended to profiles/whiten_ab.log
                                              (or to the file named by WHITEN_LOG)
  python tools/whiten_time.py time cfg3       one timing step (child)
  python tools/whiten_time.py traced cfg3     the workload of the traced step: a few whitened calls (run under rocprofv3 by the driver)
  python tools/whiten_time.py stats DIR cfg3  per-kernel summary of that trace

Flop counts (algorithmic, per latent M^2 N per triangular product or rank-N update, 2 M^2 N for a full product):
  gradient step  unwhitened 8 M^2 N (A1, full J', rank-N) x 2 latents ... whitened 6 (A, triangular J', rank-N): expected ratio 0.75
  value-only / predict  4 (A1, A2) ... 2 (A): expected ratio 0.5
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('WHITEN_LOG') or os.path.join(ROOT, 'profiles', 'whiten_ab.log')
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
    p['u_fs_sqrt'] = p['u_fs_sqrt'] * 0.8       # s != 1: D = diag(s^2 - 1) is not the zero matrix (the launches are the same either way)
    p['u_gs_sqrt'] = p['u_gs_sqrt'] * 1.2
    return N, M, reps, X, Y, p


def child_time(name):
    import torch
    import zigp
    N, M, reps, X, Y, p = problem(name)
    e = zigp.DenseEngine(0)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    e.set_data_device(Xd, Yd)
    out = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    q = {False: p, True: dict(p, whiten=True)}
    passes = (('gradient step', lambda w: e.elbo(q[w]), 8.0, 6.0),
              ('value-only ELBO', lambda w: e.elbo(q[w], need_grad=False), 4.0, 2.0),
              ('predict_device', lambda w: e.predict_device(q[w], Xd, out=out), 4.0, 2.0))
    log('%s  N=%d M=%d  %d interleaved windows of %d calls per mode (ms per call)' % (name, N, M, WINDOWS, reps))
    for label, fn, fl_u, fl_w in passes:
        for w in (False, True):
            fn(w); fn(w)                         # warm-up: tile lists, buffers, code objects of both modes
        ms = {False: [], True: []}
        for _ in range(WINDOWS):
            for w in (False, True):
                t0 = time.time()
                for _ in range(reps):
                    fn(w)                        # every call ends in the library's stream synchronisation
                ms[w].append((time.time() - t0) / reps * 1e3)
        med = {w: sorted(v)[len(v) // 2] for w, v in ms.items()}
        spread = {w: max(v) - min(v) for w, v in ms.items()}
        fl = 2 * M * M * float(N)                # two latents x M^2 N
        log('  %-16s unwhitened %8.3f (windows %s, spread %.3f; %.1f TFLOP/s of %g M^2 N)' % (
            label, med[False], ' '.join('%.3f' % v for v in ms[False]), spread[False], fl_u * fl / med[False] / 1e9, fl_u))
        log('  %-16s whitened   %8.3f (windows %s, spread %.3f; %.1f TFLOP/s of %g M^2 N)' % (
            '', med[True], ' '.join('%.3f' % v for v in ms[True]), spread[True], fl_w * fl / med[True] / 1e9, fl_w))
        log('  %-16s ratio %.3f (flop ratio %.2f); faster by more than the spread of the windows: %s' % (
            '', med[True] / med[False], fl_w / fl_u, 'yes' if max(ms[True]) < min(ms[False]) else 'NO'))
    e.close()


def child_traced(name):
    import torch
    import zigp
    N, M, reps, X, Y, p = problem(name)
    e = zigp.DenseEngine(0)
    Xd = torch.from_numpy(X).cuda()
    e.set_data_device(Xd, torch.from_numpy(Y).cuda())
    p = dict(p, whiten=True)
    for _ in range(3):
        e.elbo(p)
        e.elbo(p, need_grad=False)
    e.close()


def child_stats(d, name):
    """Per-kernel time of the trace's top kernels; TFLOP/s (algorithmic flops over summed kernel time) for the two whitened-only launches."""
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
    log('%s kernel trace: 3 whitened gradient steps + 3 whitened value-only passes' % name)
    total = 3 * 2.0 * M * M * N                 # algorithmic flops of either whitened-only launch class over the run: 3 passes x 2 latents x M^2 N
    for k in sorted(t, key=t.get, reverse=True)[:12]:
        line = '  %-74s %5d launches  avg %9.1f us' % (k[:74], n[k], t[k] / n[k])
        if 'gemm_f64_kernel' in k and ('2, 8, zigp::EpiStore>' in k or '1, 8, zigp::EpiColsum>' in k):
            line += '  %.1f TFLOP/s (%s)' % (total / t[k] / 1e6, "J' upper-triangular" if 'EpiStore>' in k else 'A, store-less')
        log(line)


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/whiten_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    me = os.path.abspath(__file__)
    out = os.environ.get('WHITEN_TRACE_DIR') or os.path.join(ROOT, 'collect_out', 'whiten_trace')     # rocprofv3 output (git-ignored)
    steps = []
    for name in ('cfg3', 'cfg2'):
        steps.append(['timeout', '-k', '10', '240', sys.executable, me, 'time', name])
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
