"""CPU-side proof that the fixtures of tests/test_gpu_kron_nd.py are fit to be judged at the project's 1e-6 parity tolerance: what
the REFERENCE alone does on every case of kron_nd.CASES, before any GPU result is looked at.

* op-order floor <= 1e-8: the factored algebra the engine evaluates, computed on the CPU with the oracle's own np.linalg.inv, lies that
  close to the literal dense oracle on the predictive means and variances -- two decades under 1e-6;
* max cond(K_p + jitter) <= 1e5 (<= 1e3 for the fixtures of the device fit loops, the conditioning at which their tolerances were
  measured: tests/test_gpu_onofftf.py::test_device_fit_loop_equals_host_adam_loop);
* 40 % to 80 % exact zeros in Y;
* every gradient block of the oracle is non-zero in every input dimension (a dead dimension would hide an indexing error);
* the oracle's own error at the shifted inputs of the shifted-input test is <= 1e-9.
A case that misses gets another lengthscale factor `c` in kron_nd.CASES; none is dropped from the GPU tests."""
import numpy as np
import pytest

import kron_nd as K

pytestmark = pytest.mark.filterwarnings(K.READ_ONLY_NOTE)


@pytest.mark.parametrize('name', list(K.CASES))
def test_fixture_floor_conditioning_zeros_and_live_gradients(name):
    X, Y, p = K.problem(name)
    k = K.CASES[name]
    assert 300 <= X.shape[0] <= 700 and X.shape[0] % 16 and X.shape[1] == sum(k['D'])
    assert [Z.shape for Z in p['Zf']] == [(k['f'][0], k['D'][0]), (k['f'][1], k['D'][1])]
    floor, cond = K.fixture_floor_and_cond(X, p, ref=K.oracle_predict(name, 0.0))
    zeros = float(np.mean(Y == 0.0))
    print('%-9s D %s f %s g %s N %d c %s: op-order floor %.2e, max cond(K_p + jitter) %.2e, zeros %.2f'
          % (name, k['D'], k['f'], k['g'] or 'same', X.shape[0], k['c'], floor, cond, zeros))
    assert floor <= 1e-8, floor
    assert cond <= 1e5, cond
    assert 0.4 <= zeros <= 0.8, zeros
    g = K.oracle_grad(name)[3]
    for key in ('Zf', 'Zg', 'ell_f', 'ell_g'):
        for q in range(2):
            a = np.abs(np.asarray(g[key][q])).reshape(-1, k['D'][q])      # Z: (M, D); ell: (1, D)
            assert a.shape[1] == k['D'][q] and np.all(a.max(0) > 0.0), (key, q, a.max(0))
    for key in ('var_f', 'var_g'):
        for q in range(2):
            assert abs(float(np.squeeze(g[key][q]))) > 0.0, (key, q)
    for key in ('u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'noise'):
        assert np.max(np.abs(np.asarray(g[key]))) > 0.0, key


@pytest.mark.parametrize('name', list(K.FIT_CASES))
def test_fit_fixture_conditioning(name):
    """the fixtures of the device fit loops (6 x 5 and 10 x 50 grids): cond(K_p + jitter) <= 1e3, floor <= 1e-8 on the first 400 rows"""
    X, Y, p = K.fit_problem(name)
    floor, cond = K.fixture_floor_and_cond(X[:400], p)
    zeros = float(np.mean(Y == 0.0))
    print('fit %-4s D %s grid %s: op-order floor %.2e, max cond(K_p + jitter) %.2e, zeros %.2f' % (name, K.FIT_CASES[name]['D'], K.FIT_CASES[name]['f'], floor, cond, zeros))
    assert cond <= 1e3 and floor <= 1e-8 and 0.4 <= zeros <= 0.8, (cond, floor, zeros)


def test_oracle_at_shifted_inputs():
    """kron_nd.SHIFT = 3.0 is added to every column of X and Z of case d21-mix.  The oracle's rbf_K expands the square
    (|x/l|^2 + |z/l|^2 - 2 (x/l)(z/l)^T, onofftf/main.py:41-51) and so loses digits as the inputs move away from 0; the same literal
    oracle with the kernel taken from the DIFFERENCES (x - z) / l is the yardstick.  On the nine predictive quantities the two lie
    1.7e-10 apart at shift 3 (4.3e-12 unshifted), 4.7e-9 at 10, 2.5e-8 at 30 and 3.5e-7 at 100 (longitude-sized): 3 is the largest of
    these at which the oracle's own error is <= 1e-9, so that is the shift at which a GPU result can be judged at 1e-6."""
    import zigp_oracle as o
    assert K.SHIFT == 3.0
    X, Y, p = K.problem(K.SHIFT_CASE, shift=K.SHIFT)
    X0, _, p0 = K.problem(K.SHIFT_CASE)
    assert np.array_equal(X, X0 + K.SHIFT) and all(np.array_equal(a, b + K.SHIFT) for t in ('Zf', 'Zg') for a, b in zip(p[t], p0[t]))
    Z, ell = p['Zf'][0], p['ell_f'][0]
    e_k = K._relerr(o.rbf_K(Z, X[:, :2], ell, 2.0), K.rbf_K_difference_form(Z, X[:, :2], ell, 2.0))
    ref = K.oracle_predict(K.SHIFT_CASE, 0.0, shift=K.SHIFT)
    expanded = o.rbf_K
    o.rbf_K = K.rbf_K_difference_form
    try:
        diff = o.kron_build_predict(X, p, K.JITTER, 0.0)
    finally:
        o.rbf_K = expanded
    errs = [K._relerr(ref[i], diff[i]) for i in range(9)]
    print('shift %g: rbf_K expanded vs difference form %.2e; predictive quantities %s' % (K.SHIFT, e_k, ' '.join('%.1e' % e for e in errs)))
    assert e_k <= 1e-9 and max(errs) <= 1e-9, (e_k, errs)
    floor, cond = K.fixture_floor_and_cond(X, p, ref=ref)
    assert floor <= 1e-8 and cond <= 1e5, (floor, cond)
