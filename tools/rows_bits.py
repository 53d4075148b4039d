"""The bits of the row calls that tools/density_time.py's `bits` step does not cover -- scores, sample paths and predict -- for a comparison
between two builds of libzigp.so (ZIGP_LIB selects the library, zigp/_lib.py).

  python tools/rows_bits.py FILE.npz           every output array of a fixed list of small calls (N <= 300, M <= 32, D = 2), written to FILE.npz
  python tools/rows_bits.py A.npz B.npz        compares the two files array by array with numpy.array_equal; exit status 1 unless all are equal

The calls: score_rows 'onoff' at 20 and 40 nodes (half a wave and a whole wave per row) with 3 levels, score_rows 'gaussian',
predict_scores and predict_scores_device, path_rows with one and with two latents at S = 17, sample_paths and sample_paths_device under
the three parametrisations (diagonal, whitened, whitened with a full covariance), predict and predict_device.  Run each dump as one GPU
step under its own `timeout`, the two chained with `&&`.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'zero-inflated-gp_amd'))
N, M, MG, D, S = 300, 32, 24, 2, 17
LEVELS = (0.05, 0.5, 0.95)


def problem(rs):
    X = rs.rand(N, D)
    Y = np.where(rs.rand(N) > 0.4, np.sin(5 * X[:, 0]) + 0.1 * rs.randn(N), 0.0)
    p = dict(Zf=rs.rand(M, D), Zg=rs.rand(MG, D), u_fm=0.5 * rs.randn(M), u_gm=0.5 * rs.randn(MG), u_fs_sqrt=0.3 + rs.rand(M),
             u_gs_sqrt=0.3 + rs.rand(MG), ell_f=np.array([0.3, 0.35]), ell_g=np.array([0.4, 0.45]), var_f=1.0, var_g=5.0, noise=0.01,
             mean_a=np.array([0.2, -0.1]), mean_b=0.3)
    full = dict(p, whiten=True, q_diag=False, u_fs_sqrt=np.tril(0.1 * rs.randn(M, M), -1) + np.diag(0.3 + rs.rand(M)),
                u_gs_sqrt=np.tril(0.1 * rs.randn(MG, MG), -1) + np.diag(0.3 + rs.rand(MG)))
    return X, Y, {'diag': p, 'white': dict(p, whiten=True), 'white_full': full}


def path_latent(rs, kind, Mh, R):
    ell = np.array([0.4, 0.5])
    return dict(kind=kind, Z=rs.rand(Mh, D), ell=ell, var=1.5, V=rs.randn(Mh, S), omega=rs.randn(R, D) / ell, phase=rs.uniform(0, 2 * np.pi, R),
                amp=rs.randn(R, S) * np.sqrt(3.0 / R), lin=rs.randn(D), shift=-0.3)


def dump(path):
    import torch
    import zigp
    from zigp import pathwise
    rs = np.random.RandomState(17)
    X, Y, models = problem(rs)
    rows = (rs.randn(N), 0.05 + rs.rand(N), 1.5 * rs.randn(N), 0.05 + 2.0 * rs.rand(N), rs.randn(N) * (rs.rand(N) > 0.3))
    lats = [path_latent(rs, 'rbf', 9, 13), path_latent(rs, 'matern52', 32, 6)]
    draws = {t: pathwise.draw('rbf', 21, D, m, S, rs) for t, m in (('f', M), ('g', MG))}
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    e = zigp.DenseEngine(0)
    res = {}

    def keep(tag, r):
        for name, v in r.items():
            if v is not None and name != 'draws':
                res['%s %s' % (tag, name)] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    p = models['diag']
    for n in (20, 40):
        keep('score_rows onoff n_quad=%d' % n, e.score_rows('onoff', *rows, p['noise'], n_quad=n, levels=LEVELS))
    keep('score_rows gaussian', e.score_rows('gaussian', rows[0], rows[1], None, None, rows[4], p['noise'], levels=LEVELS))
    keep('predict_scores', e.predict_scores(p, X, Y, n_quad=20, levels=LEVELS))
    keep('predict_scores_device', e.predict_scores_device(p, Xd, Yd, n_quad=20, levels=LEVELS))
    keep('path_rows 1 latent', dict(out=e.path_rows(lats[:1], X, S)))
    keep('path_rows 2 latents', dict(out=e.path_rows(lats, X, S)))
    for name, q in models.items():
        keep('sample_paths %s' % name, e.sample_paths(q, X, n_samples=S, draws=draws))
        keep('sample_paths_device %s' % name, e.sample_paths_device(q, Xd, n_samples=S, draws=draws))
    keep('predict', dict(out9=e.predict(p, X)))
    keep('predict_device', dict(out9=e.predict_device(p, Xd)))
    e.close()
    np.savez(path, **res)
    print('rows_bits: %d arrays of %s written to %s' % (len(res), os.environ.get('ZIGP_LIB') or 'this build', path))


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    same = sorted(a.files) == sorted(b.files)
    if not same:
        print('  bits: the two files hold different sets of arrays')
    for k in a.files:
        eq = k in b.files and np.array_equal(a[k], b[k])
        same = same and eq
        print('  bits  %-44s %-10s %s' % (k, 'x'.join(str(d) for d in a[k].shape) or 'scalar', 'equal' if eq else 'DIFFERENT'))
    print('  bits: every array of %s equal to that of %s' % (fa, fb) if same else '  bits: NOT every array is equal')
    return same


if __name__ == '__main__':
    if len(sys.argv) == 2:
        dump(sys.argv[1])
    elif len(sys.argv) == 3:
        sys.exit(0 if compare(sys.argv[1], sys.argv[2]) else 1)
    else:
        sys.exit(__doc__)
