"""Host side of the dense device fit loop (zigp_fit_steps): the C-ABI symbols, and zigp.optim.DenseDeviceFit against a stand-in engine
whose fit_steps is the CPU oracle (torch autograd) plus NumPy Adam.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_problem
import dense_fit_ref as R


def test_fit_steps_symbols_exist_and_reject_a_null_context():
    from zigp import _lib
    lib = _lib.load()
    assert _lib.DENSE_FIT_BLOCKS == 11 and C.sizeof(_lib.zigp_fit_opts) == 11 * 8 + 2 * 11 * 4 + 2 * 4 + 3 * 8
    s, o = _lib.zigp_params(), _lib.zigp_fit_opts()
    x = np.zeros(4)
    rc = lib.zigp_fit_steps(None, C.byref(s), C.byref(o), x.ctypes.data, x.ctypes.data, x.ctypes.data, 4, 0, 1, None, 0, 1e-6, 1.0, 1, None, None)
    assert rc == _lib.ZIGP_EARG
    assert lib.zigp_fit_steps_applied(None) == _lib.ZIGP_EARG


class OracleFitEngine:
    """engine.fit_steps restated on the CPU oracle; records what it was called with"""

    def __init__(self, X, Y):
        self.X, self.Y = X, Y
        self.calls = []
        self.fail_at = None

    def fit_steps(self, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6, scale=1.0,
                  beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        import zigp
        import zigp_oracle_torch as ot
        self.calls.append(dict(shape=dict(shape), x=x.copy(), lr=list(lr), positive=list(positive), trainable=list(trainable),
                               ell_size=tuple(ell_size), t0=t0, n_steps=n_steps))

        def eg(Xb, Yb, p, jit, sc):
            elbo, data, kl, g = ot.elbo_and_grad(Xb, Yb, p, jit, scale=sc)
            return sc * data, kl, g

        k = n_steps if self.fail_at is None else self.fail_at
        ed, kl = R.ref_fit_steps(eg, self.X, self.Y, shape, x, m, v, lr, positive, trainable, ell_size, t0, k, rows=rows, batch=batch,
                                 jitter=jitter, scale=scale, beta1=beta1, beta2=beta2, eps=eps)
        if self.fail_at is not None:
            e = zigp.NotPositiveDefiniteError('Cholesky failed in step %d' % k)
            e.steps_applied, e.elbo_data, e.kl = k, ed, kl
            raise e
        return ed, kl


def test_dense_device_fit_layout_folding_fixed_blocks_failure_count_and_outside_changes():
    """DenseDeviceFit hands zigp_fit_steps the ParamSet of OnOffSVGP in the block order and sizes of include/zigp.h: checked by running
    the oracle-backed stand-in next to the host loop (select_rows + elbo + AdamGroups on the same oracle, same row samples).  Covered:
    block order and sizes, a scalar lengthscale (ell_size = 1, gradient = sum over the columns), fixed blocks (trainable = 0: x, m, v and
    .value untouched), t advancing by steps_applied when a call fails, an assignment to a .value taken up by the next call."""
    import zigp
    from zigp.optim import DenseDeviceFit, DENSE_FIT_KEYS
    X, Y, p = make_problem(300, 7, 2, seed=3, Mg=5, ell=0.4)
    lr = {k: 0.002 * (1 + i) for i, k in enumerate(DENSE_FIT_KEYS)}
    mk = lambda: R.make_pset(p, scalar_ell=(True, False), fixed=('Zf', 'noise'), lr=lr)
    rows = np.random.RandomState(5).randint(300, size=(4, 64))
    scale = 300.0 / 64.0

    host = mk()
    hist_h = R.host_loop(R.OracleEngine(X, Y), host, rows, 1e-6, scale)

    eng = OracleFitEngine(X, Y)
    dev = mk()
    fit = DenseDeviceFit(eng, dev)
    assert fit.shape == dict(Mf=7, Mg=5, D=2) and fit.sizes == [14, 10, 7, 5, 7, 5, 1, 2, 1, 1, 1] and fit.ell_size == (1, 2)
    assert fit.positive == [False, False, False, False, True, True, True, True, True, True, True]
    assert fit.trainable == [False, True, True, True, True, True, True, True, True, True, False]
    assert fit.lr == [lr[k] for k in DENSE_FIT_KEYS]
    x0 = fit.x.copy()
    ed, kl = fit.steps(rows, 64, 1e-6, scale)
    assert fit.t == 4 and eng.calls[0]['t0'] == 0 and eng.calls[0]['n_steps'] == 4
    assert np.allclose(np.stack([ed, kl], 1), hist_h, rtol=1e-12, atol=0)
    for k in DENSE_FIT_KEYS:
        a, b = dev.params[k].value.reshape(-1), host.params[k].value.reshape(-1)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), k
    assert dev.params['u_fm'].value.shape == (7, 1) and np.max(np.abs(dev.params['u_fm'].value - p['u_fm'])) > 1e-3     # it did move
    # fixed blocks: value, x, m, v untouched
    assert np.array_equal(dev.params['Zf'].value, p['Zf']) and float(dev.params['noise'].value[0]) == p['noise']
    o = np.concatenate([[0], np.cumsum(fit.sizes)])
    for b in (0, 10):
        assert np.array_equal(fit.x[o[b]:o[b + 1]], x0[o[b]:o[b + 1]]) and not fit.m[o[b]:o[b + 1]].any() and not fit.v[o[b]:o[b + 1]].any()
    assert fit.m[o[1]:o[2]].any() and fit.v[o[6]:o[7]].any()
    # a failure in step 2 of 5: two updates applied, t advances by two, the exception carries their history
    eng.fail_at = 2
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        fit.steps(np.random.RandomState(6).randint(300, size=(5, 64)), 64, 1e-6, scale)
    assert fit.t == 6 and ei.value.steps_applied == 2 and len(ei.value.elbo_data) == 2 and eng.calls[-1]['t0'] == 4
    assert np.array_equal(dev.params['u_gm'].value.reshape(-1), fit.x[o[3]:o[4]])      # the ParamSet holds the state after those two updates
    # an assignment from outside is the next call's starting point; so are a parameter fixed in between and a new learning rate
    eng.fail_at = None
    dev.params['u_gm'].value = np.full_like(dev.params['u_gm'].value, 0.75)
    dev.params['var_g'].fixed = True
    dev.params['Zg'].learning_rate = 0.5
    fit.steps(None, 0, 1e-6, 1.0, n_steps=1)
    c = eng.calls[-1]
    assert np.all(c['x'][o[3]:o[4]] == 0.75) and c['trainable'][9] is False and c['lr'][1] == 0.5 and c['t0'] == 6 and fit.t == 7
    # a parameter that has gone NaN is still the value this object wrote
    fit.x[o[2]:o[3]] = np.nan
    fit.sync_params()
    assert not fit._stale()
    fit.resync(reset=True)
    assert fit.t == 0 and not fit.m.any()


def test_dense_device_fit_refuses_what_the_device_loop_does_not_do():
    from zigp.optim import DenseDeviceFit, P
    from zigp.transforms import Log1pe
    X, Y, p = make_problem(50, 4, 2, seed=1)
    ps = R.make_pset(p)
    ps.params['mean_b'] = P(np.zeros(1))
    with pytest.raises(ValueError, match='mean-function'):
        DenseDeviceFit(None, ps)
    ps = R.make_pset(p)
    ps.params['noise'].transform = Log1pe(lower=1e-3)
    with pytest.raises(ValueError, match='lower'):
        DenseDeviceFit(None, ps)

    class Exp:
        pass
    ps = R.make_pset(p)
    ps.params['var_f'].transform = Exp()
    with pytest.raises(ValueError, match='unsupported transform'):
        DenseDeviceFit(None, ps)


def test_two_host_runs_measure_stands_on_a_well_conditioned_problem():
    """The GPU test's yardstick, exercised here with the oracle standing in for the engine: two host runs that differ by a seeded +-1 ulp
    on every free-state element after every step stay within 1e-9 / 8 of each other on the problem the GPU test uses (lengthscales chosen
    for cond(Kuu) ~ 1e2 ... 1e4), so that 8 d is a bound that can show something."""
    import zigp_oracle as o
    X, Y, p = dense_problem()
    cond = [np.linalg.cond(o.rbf_K(p['Z' + t], None, p['ell_' + t], p['var_' + t]) + 1e-6 * np.eye(p['Z' + t].shape[0])) for t in 'fg']
    print('cond(Kuu) f %.2e g %.2e' % tuple(cond))
    assert 1e2 <= max(cond) <= 1e4
    rows = np.random.RandomState(11).randint(X.shape[0], size=(25, 512))
    scale = X.shape[0] / 512.0
    a, b = R.make_pset(p), R.make_pset(p)
    ha = R.host_loop(R.OracleEngine(X, Y), a, rows, 1e-6, scale)
    hb = R.host_loop(R.OracleEngine(X, Y), b, rows, 1e-6, scale, nudge_seed=1)
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    print('25 steps: d_par %.2e d_hist %.2e' % (d_par, d_hist))
    assert 0 < 8 * max(d_par, d_hist) <= 1e-9


def dense_problem():
    """the 200-step problem of test_gpu_dense_fit.py: N = 3000, Mf = 96, Mg = 70, D = 3, lengthscales for cond(Kuu) ~ 1e2 ... 1e4"""
    return make_problem(3000, 96, 3, seed=17, Mg=70, ell=0.12)
