"""What the predictive density costs, on one box, same build: ms per call at the cfg2 shape (N = 1e5, M = 512, D = 3) of predict_device --
the pass the density rides on -- against predict_density_device with centre='mean' and centre='mode' at n_quad = 20, 64 and 256, in
interleaved windows.  predict_device is the yardstick of the density kernel, the fixed rule that of the mode-centred one, and the spread
of an arm's windows is the box's run-to-run noise.  The rows are those of the synthetic cfg2 problem under its initial parameters: the
search's cost depends on how far each row's mode lies from gm (one capped step per unit of g), so the mode arms are the cost on THESE
rows, not a bound.

  python tools/density_time.py               driver: every GPU step is a child process under its own `timeout`, the steps are chained
                                             (the first one that fails ends the run); everything is appended to profiles/density_time.log
                                             (or to the file named by DENSITY_LOG)
  python tools/density_time.py time [FILE]   the timing step (child); FILE: the windows of every arm as JSON
  python tools/density_time.py bits FILE     the results of a fixed set of calls as an .npz file (child)

With DENSITY_PARENT_LIB=<libzigp.so built from the parent commit> the driver adds, with ZIGP_LIB pointing there, the same timing step
-- per arm the median of this build against the parent's of the same run, the margin being the parent's own window spread -- and a
"bits" step: one short child per library writes out3, centre2 and the sum of the calls in child_bits, and the driver compares the two
files array by array with np.array_equal.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
LOG = os.environ.get('DENSITY_LOG') or os.path.join(ROOT, 'profiles', 'density_time.log')
N, M, D, REPS, WINDOWS = 100000, 512, 3, 20, 5
QUADS = (20, 64, 256)


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


def median(v):
    return sorted(v)[len(v) // 2]


def child_time(dump=None):
    import torch
    import bench
    import zigp
    from zigp.quadrature import gauss_hermite
    e = zigp.DenseEngine(0)
    X, Y, p = bench.synth(N, M, D)
    Xd, Yd = torch.from_numpy(np.ascontiguousarray(X)).cuda(), torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    out9 = torch.empty((9, N), dtype=torch.float64, device='cuda:0')
    out3 = torch.empty((3, N), dtype=torch.float64, device='cuda:0')
    rules = {n: gauss_hermite(n) for n in QUADS}
    arms = [('predict_device', lambda: e.predict_device(p, Xd, out=out9))]
    for centre in ('mean', 'mode'):
        arms += [('%s n_quad=%d' % (centre, n), lambda n=n, centre=centre: e.predict_density_device(p, Xd, Yd, rule=rules[n], out=out3, centre=centre))
                 for n in QUADS]
    log('%s  N=%d M=%d D=%d  %d interleaved windows of %d calls per arm (ms per call)' % (
        'ZIGP_LIB=' + os.environ['ZIGP_LIB'] if os.environ.get('ZIGP_LIB') else 'this build', N, M, D, WINDOWS, REPS))
    _, _, c2 = e.predict_density_device(p, Xd, Yd, rule=rules[20], centre='mode', return_centre=True)
    c2 = c2.cpu().numpy()
    log('  centres of these rows: |zhat| median %.3g, max %.3g; tau from %.3g to %.3g' % (np.median(np.abs(c2[0])), np.abs(c2[0]).max(), c2[1].min(), c2[1].max()))
    for _, fn in arms:
        fn(); fn()                               # warm-up: tile lists, buffers, code objects
    ms = {k: [] for k, _ in arms}
    for _ in range(WINDOWS):
        for k, fn in arms:
            t0 = time.time()
            for _ in range(REPS):
                fn()                             # every call ends in the library's stream synchronisation
            ms[k].append((time.time() - t0) / REPS * 1e3)
    med = {k: median(v) for k, v in ms.items()}
    for k, _ in arms:
        line = '  %-20s %8.3f (windows %s, spread %.3f)' % (k, med[k], ' '.join('%.3f' % v for v in ms[k]), max(ms[k]) - min(ms[k]))
        if k != 'predict_device':
            line += '  %+.3f ms over predict_device' % (med[k] - med['predict_device'])
        if k.startswith('mode'):
            line += ', %+.3f ms over the fixed rule' % (med[k] - med[k.replace('mode', 'mean')])
        log(line)
    if dump:
        with open(dump, 'w') as f:
            json.dump(ms, f)
    e.close()


def child_bits(dump):
    """out3, centre2 and the sum of: the grid and stress rows of tests/density_centred_ref.py and the 257 rows of the block-boundary test
    (n_quad 1, 20, 256) under both centres, the head rows of tests/density_ref.py, and the dense call of the end-to-end tests"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import zigp
    from conftest import make_problem
    import density_ref as R
    import density_centred_ref as Q
    from test_gpu_density_centred import _rows
    e = zigp.DenseEngine(0)
    res = {}

    def keep(tag, r):
        for name, v in zip(('out3', 'sum', 'centre2'), r):
            res['%s %s' % (tag, name)] = np.asarray(v)

    sets = [('grid', Q.case_rows('grid'), (20, 64)), ('stress', Q.case_rows('stress'), (20, 64)), ('rows257', _rows(257, seed=7), (1, 20, 256))]
    for name, rows, quads in sets:
        for n in quads:
            keep('%s n_quad=%d mean' % (name, n), e.density_rows('onoff', *rows, Q.NOISE, rule=Q.rule(n)))
            keep('%s n_quad=%d mode' % (name, n), e.density_rows('onoff', *rows, Q.NOISE, rule=Q.rule(n), centre='mode', return_centre=True))
    for lik in ('gaussian', 'bernoulli'):
        fm, fv, y = R.head_grid(lik)
        keep(lik, e.density_rows(lik, fm, fv, None, None, y, R.NOISE))
    X, Y, p = make_problem(1350, 48, 3, seed=11, Mg=40, ell=0.4)
    e.set_chunk(1024)
    keep('predict_density mean', e.predict_density(p, X, Y, n_quad=20))
    keep('predict_density mode', e.predict_density(p, X, Y, n_quad=20, centre='mode', return_centre=True))
    e.close()
    np.savez(dump, **res)


def compare_bits(new, parent):
    a, b = np.load(new), np.load(parent)
    same = sorted(a.files) == sorted(b.files)
    if not same:
        log('  bits: the two builds wrote different sets of arrays')
    for k in a.files:
        eq = k in b.files and np.array_equal(a[k], b[k])
        same = same and eq
        log('  bits  %-40s %s  %s' % (k, 'x'.join(str(d) for d in a[k].shape) or 'scalar', 'equal' if eq else 'DIFFERENT'))
    log('  bits: every array equal to the parent build\'s' if same else '  bits: NOT every array is equal to the parent build\'s')
    return same


def compare_times(new, parent):
    a, b = json.load(open(new)), json.load(open(parent))
    ok = True
    log('  against the parent build (ms per call: median of this build, median of the parent, the parent\'s window spread max - min)')
    for k in a:
        spread = max(b[k]) - min(b[k])
        fine = median(a[k]) <= median(b[k]) + spread
        ok = ok and fine
        log('  %-20s %8.3f %8.3f  spread %.3f  %s' % (k, median(a[k]), median(b[k]), spread, 'within the spread' if fine else 'SLOWER by more than the spread'))
    return ok


def driver():
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    log('# tools/density_time.py  %s' % time.strftime('%Y-%m-%d %H:%M:%S'))
    me, parent = os.path.abspath(__file__), os.environ.get('DENSITY_PARENT_LIB')
    with tempfile.TemporaryDirectory() as tmp:
        f = {k: os.path.join(tmp, k) for k in ('time.json', 'time_parent.json', 'bits.npz', 'bits_parent.npz')}
        under = ['env', 'ZIGP_LIB=' + os.path.abspath(parent)] if parent else None
        steps = [['timeout', '-k', '10', '300', sys.executable, me, 'time', f['time.json']]]
        if parent:                                    # the parent commit's build, same box, same run
            steps.append(['timeout', '-k', '10', '300'] + under + [sys.executable, me, 'time', f['time_parent.json']])
            steps.append(['timeout', '-k', '10', '120', sys.executable, me, 'bits', f['bits.npz']])
            steps.append(['timeout', '-k', '10', '120'] + under + [sys.executable, me, 'bits', f['bits_parent.npz']])
        for cmd in steps:                             # chained: nothing more is started on the GPU after a step that failed
            rc = subprocess.call(cmd)
            if rc != 0:
                log('step failed (exit status %d), stopping: %s' % (rc, ' '.join(cmd[4:])))
                return rc
        if parent:
            ok = compare_times(f['time.json'], f['time_parent.json'])
            ok = compare_bits(f['bits.npz'], f['bits_parent.npz']) and ok
            return 0 if ok else 1
    return 0


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'time':
        child_time(sys.argv[2] if len(sys.argv) >= 3 else None)
    elif len(sys.argv) >= 3 and sys.argv[1] == 'bits':
        child_bits(sys.argv[2])
    else:
        sys.exit(driver())
