"""Host loop against device loop of the dense Adam fit (zigp_fit_steps), and the kernel timeline of a device call.

  python tools/dense_fit_timeline.py [compare] [point ...]
      ms per iteration of the host loop (select_rows + elbo + AdamGroups: OnOffSVGP.optimize(method='adam') with a callback) and of the
      device loop (DenseDeviceFit.steps, calls of 200 iterations), same model, same row samples.  Interleaved windows (host, device, host,
      ...), warmed; every window is at least 200 iterations and 0.5 s and ends synchronised (each elbo call and each fit call ends with the
      library's stream synchronisation).  Prints the median over the windows and their spread (max - min) / median.
      Points: toy9 toy50 (toydata.mat, N = 450; full batch and batch 100), m256 m512 m1024 (D = 3, 1e5 resident rows; batches of 1024 and
      8192), cfg2 (N = 1e5, M = 512, full batch).  Default: all of them.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/dense_fit_timeline.py run M BATCH
      one warmed device call of 200 iterations for the tracer; then
  python tools/dense_fit_timeline.py DIR
      prints one iteration from the middle of the call (kernels, durations, gaps) and the averages over the call by kernel.
"""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trace_report(d):
    f = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
    upd = [i for i, r in enumerate(rows) if 'k_dense_fit_update' in r['Kernel_Name']][-200:]     # the last call: the timed one
    name = lambda r: r['Kernel_Name'].split('(')[0][-48:]
    mid = len(upd) // 2
    a, b = upd[mid - 1] + 1, upd[mid] + 1
    t0 = int(rows[a]['Start_Timestamp'])
    prev = int(rows[a - 1]['End_Timestamp'])
    for r in rows[a:b]:
        s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
        print('%8.1f %8.1f  %6.1f us  (gap %6.1f)  %s' % ((s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, (s - prev) / 1e3, name(r)))
        prev = max(prev, e)
    n = len(upd) - 1
    span = (int(rows[upd[-1]]['End_Timestamp']) - int(rows[upd[0]]['End_Timestamp'])) / 1e3 / n
    per, cnt = {}, {}
    for r in rows[upd[0] + 1:upd[-1] + 1]:
        per[name(r)] = per.get(name(r), 0.0) + (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 / n
        cnt[name(r)] = cnt.get(name(r), 0) + 1
    print('per iteration over %d iterations: span %.1f us, %d launches, sum of kernel durations %.1f us (three streams: they overlap)'
          % (n, span, sum(cnt.values()) // n, sum(per.values())))
    for k, v in sorted(per.items(), key=lambda kv: -kv[1]):
        print('  %7.1f us  %5.1f x  %s' % (v, cnt[k] / n, k))


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import numpy as np
    import bench
    import zigp
    from zigp.optim import DenseDeviceFit
    import dense_fit_ref as R

    def toy(M):
        import scipy.io as sio
        mat = sio.loadmat(os.path.join(ROOT, 'tests', 'golden', 'toydata.mat'))
        X, Y = np.asarray(mat['x'], dtype=np.float64), np.asarray(mat['y'], dtype=np.float64)
        Z = np.linspace(X.min(), X.max(), M + 1, endpoint=False)[1:, None]
        ru = np.random.RandomState(2)
        return X, Y, dict(Zf=Z.copy(), Zg=Z.copy(), u_fm=0.01 * ru.randn(M, 1), u_gm=0.01 * ru.randn(M, 1), u_fs_sqrt=np.ones((M, 1)),
                          u_gs_sqrt=np.ones((M, 1)), ell_f=np.full(1, 2.0), ell_g=np.full(1, 2.0), var_f=1.0, var_g=5.0, noise=0.01)

    points = {'toy9': (lambda: toy(9), (None, 100)), 'toy50': (lambda: toy(50), (None, 100)),
              'm256': (lambda: bench.synth(100000, 256, 3), (1024, 8192)), 'm512': (lambda: bench.synth(100000, 512, 3), (1024, 8192)),
              'm1024': (lambda: bench.synth(100000, 1024, 3), (1024, 8192)), 'cfg2': (lambda: bench.synth(100000, 512, 3), (None,))}
    args = [a for a in sys.argv[1:] if a != 'compare']
    eng = zigp.DenseEngine(0)

    if args and args[0] == 'run':
        M, batch = int(args[1]), int(args[2])
        X, Y, p = bench.synth(100000, M, 3)
        eng.set_data(X, Y)
        fit = DenseDeviceFit(eng, R.make_pset(p, lr=1e-3))
        rows = np.random.RandomState(3).randint(X.shape[0], size=(200, batch))
        fit.steps(rows[:20], batch, 1e-6, X.shape[0] / batch)
        t0 = time.time()
        fit.steps(rows, batch, 1e-6, X.shape[0] / batch)
        print('M %d batch %d: %.3f ms per iteration (200 iterations, one call)' % (M, batch, (time.time() - t0) / 200 * 1e3))
        return

    print('%-22s %12s %12s %8s   %s' % ('point', 'host ms/it', 'device ms/it', 'ratio', 'spread host / device, windows x iterations'))
    for name in (args or list(points)):
        make, batches = points[name]
        X, Y, p = make()
        N = X.shape[0]
        eng.set_data(X, Y)
        for batch in batches:
            scale = 1.0 if batch is None else N / batch
            rs = np.random.RandomState(3)
            draw = (lambda n: None) if batch is None else (lambda n: rs.randint(N, size=(n, batch)))
            hp, dp = R.make_pset(p, lr=1e-3), R.make_pset(p, lr=1e-3)
            fit = DenseDeviceFit(eng, dp)

            def host(n):
                rows = draw(n)
                t0 = time.time()
                R.host_loop(eng, hp, rows, 1e-6, scale, n_steps=n)
                return (time.time() - t0) / n

            def device(n):
                rows = draw(n)
                t0 = time.time()
                for o in range(0, n, 200):
                    k = min(200, n - o)
                    fit.steps(None if rows is None else rows[o:o + k], batch or 0, 1e-6, scale, n_steps=k)
                return (time.time() - t0) / n

            n = {}
            for tag, fn in (('host', host), ('device', device)):      # warm-up, and the window length: >= 200 iterations and >= 0.5 s
                fn(20)
                n[tag] = max(200, int(np.ceil(0.5 / fn(200) / 200.0)) * 200)
            th, td = [], []
            for _ in range(3):
                th.append(host(n['host']))
                td.append(device(n['device']))
            mh, md = np.median(th), np.median(td)
            print('%-22s %12.4f %12.4f %8.2f   %.1f %% / %.1f %%, 3 x %d / 3 x %d'
                  % ('%s %s' % (name, 'full batch' if batch is None else 'batch %d' % batch), mh * 1e3, md * 1e3, mh / md,
                     (max(th) - min(th)) / mh * 100, (max(td) - min(td)) / md * 100, n['host'], n['device']), flush=True)
            eng.select_rows(None)


if __name__ == '__main__':
    if len(sys.argv) > 1 and os.path.isdir(sys.argv[1]):
        trace_report(sys.argv[1])
    else:
        main()
