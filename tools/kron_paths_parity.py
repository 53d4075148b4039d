"""The Kronecker path weights with and without a refinement step, measured: zigp_kron_sample_paths against the NumPy restatement
(tests/kronpaths_ref.py, per-factor Cholesky and triangular solves) on the model fixtures of tests/test_gpu_kron_paths.py, next to the path
bound min(max(1e-9, 1e-13 c), 1e-6), c = cond(K0) cond(K1).  Each plane is normalised by its largest entry.  The product library has no
step; a variant build has V += K0^-1 (rhs - K0 V K1) K1^-1 compiled in:

  tools/build_variant.sh kron_refine -DZIGP_KRON_PATH_REFINE
  python tools/kron_paths_parity.py        one child process per library (the product build, then the variant where it exists), each
                                           under its own `timeout`; appends to profiles/kron_paths_parity.log (or to KRON_PATHS_LOG)
  python tools/kron_paths_parity.py run    the measuring step (child): the library that ZIGP_LIB names, else the product build
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for q in ('', 'zero-inflated-gp_amd', 'tests', 'oracle'):
    sys.path.insert(0, os.path.join(ROOT, q))
LOG = os.environ.get('KRON_PATHS_LOG') or os.path.join(ROOT, 'profiles', 'kron_paths_parity.log')


def log(line):
    print(line, flush=True)
    with open(LOG, 'a') as f:
        f.write(line + '\n')


VARIANT = os.path.join(ROOT, 'zero-inflated-gp_amd', 'lib', 'libzigp_kron_refine.so')


def child():
    import zigp
    import kron_nd
    import kronpaths_ref as kr
    e = zigp.DenseEngine(0)
    for name in kr.MODEL_CASES:
        X, Y, p = kron_nd.problem(name)
        bound, c = kr.path_bound(p, ('f', 'g'), kr.MODEL_JITTER)
        got = e.kron_sample_paths(p, X, n_samples=kr.MODEL_S, draws=kr.model_draws(name), jitter=kr.MODEL_JITTER, g_offset=-1.0, f_mu=0.25)
        ref = kr.model_ref(name, -1.0, 0.25)
        log('  %-8s %10.2e %10.2e   %s' % (name, c, bound, ' '.join('%.2e' % kr.plane_err(got[k], ref[k]) for k in ('f', 'g', 'gf'))))
    e.close()


def main():
    import subprocess
    log('# tools/kron_paths_parity.py  %s   R = 200, S = 20, jitter 1e-05' % time.strftime('%Y-%m-%d %H:%M:%S'))
    for label, lib in (('the product build: no refinement step', None), ('-DZIGP_KRON_PATH_REFINE: with the step', VARIANT)):
        if lib and not os.path.exists(lib):
            log('(no %s: the variant was not built)' % os.path.relpath(lib, ROOT))
            continue
        log('== %s ==' % label)
        log('  %-8s %10s %10s   %s' % ('case', 'cond prod', 'bound', 'f g gf'))
        env = dict(os.environ)
        if lib:
            env['ZIGP_LIB'] = lib
        rc = subprocess.call(['timeout', '-k', '10', '150', sys.executable, os.path.abspath(__file__), 'run'], env=env)
        if rc != 0:
            log('step failed (exit status %d), stopping' % rc)
            return rc
    return 0


if __name__ == '__main__':
    if len(sys.argv) >= 2 and sys.argv[1] == 'run':
        child()
    else:
        sys.exit(main())
