"""Host side of the dense device fit loop for the whitened models (zigp_fit_steps_mode): the C-ABI symbol and its constants,
zigp.optim.WhiteDeviceFit against a recording stand-in engine whose fit_steps_mode is the CPU reference (whiten_ref / fullcov_ref: torch
autograd) plus NumPy Adam, the NumPy restatement against AdamGroups, and the two-host-runs yardstick of the GPU test.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import make_problem
import dense_fit_ref as R
import white_fit_ref as W
from test_cpu_dense_fit import dense_problem

MODES = [W.WHITE, W.WHITE_FULL]


def test_fit_steps_mode_symbol_exists_rejects_a_null_context_and_its_constants_match_the_header():
    from zigp import _lib
    lib = _lib.load()
    s, o = _lib.zigp_params(), _lib.zigp_fit_opts()
    x = np.zeros(4)
    for mode in (_lib.FIT_DIAG, _lib.FIT_WHITE, _lib.FIT_WHITE_FULL):
        rc = lib.zigp_fit_steps_mode(None, mode, C.byref(s), C.byref(o), x.ctypes.data, x.ctypes.data, x.ctypes.data, 4, 0, 1, None, 0, 1e-6, 1.0, 1,
                                     None, None)
        assert rc == _lib.ZIGP_EARG
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'zigp.h')).read()
    got = {k: int(v) for k, v in re.findall(r'#define\s+(ZIGP_FIT_(?:DIAG|WHITE|WHITE_FULL))\s+(\d+)', hdr)}
    assert got == dict(ZIGP_FIT_DIAG=_lib.FIT_DIAG, ZIGP_FIT_WHITE=_lib.FIT_WHITE, ZIGP_FIT_WHITE_FULL=_lib.FIT_WHITE_FULL)
    assert (W.WHITE, W.WHITE_FULL) == (_lib.FIT_WHITE, _lib.FIT_WHITE_FULL)


class RefFitEngine:
    """engine.fit_steps_mode restated on the CPU references; records what it was called with.  It has no fit_steps: a WhiteDeviceFit
    that called it would fail."""

    def __init__(self, X, Y):
        self.X, self.Y = X, Y
        self.calls = []
        self.fail_at = None

    def fit_steps_mode(self, mode, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6, scale=1.0,
                       beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        import zigp
        self.calls.append(dict(mode=mode, shape=dict(shape), x=x.copy(), lr=list(lr), positive=list(positive), trainable=list(trainable),
                               ell_size=tuple(ell_size), t0=t0, n_steps=n_steps))
        k = n_steps if self.fail_at is None else self.fail_at
        ed, kl = W.ref_fit_steps(mode, W.ref_elbo_grad(mode), self.X, self.Y, shape, x, m, v, lr, positive, trainable, ell_size, t0, k, rows=rows,
                                 batch=batch, jitter=jitter, scale=scale, beta1=beta1, beta2=beta2, eps=eps)
        if self.fail_at is not None:
            e = zigp.NotPositiveDefiniteError('Cholesky failed in step %d' % k)
            e.steps_applied, e.elbo_data, e.kl = k, ed, kl
            raise e
        return ed, kl


@pytest.mark.parametrize('mode', MODES)
def test_white_device_fit_layout_triangular_blocks_fixed_blocks_failure_count_and_outside_changes(mode):
    """WhiteDeviceFit hands zigp_fit_steps_mode the ParamSet of a whitened OnOffSVGP in the block order and sizes of include/zigp.h: checked
    by running the reference-backed stand-in next to the host loop (select_rows + elbo + AdamGroups on the same reference, same row
    samples).  Covered: the mode, block order and sizes (mode 2: M (M + 1) / 2), the triangular free vector = LowerTriangular.backward(value)
    and an exactly zero upper triangle after sync_params, a scalar lengthscale, fixed blocks, t advancing by steps_applied when a call
    fails, an assignment to a .value taken up by the next call."""
    import zigp
    from zigp.optim import WhiteDeviceFit, DENSE_FIT_KEYS
    X, Y, p0 = make_problem(300, 7, 2, seed=3, Mg=5, ell=0.4)
    p = W.problem(p0, mode, lq_seed=1, negative=1)
    lr = {k: 0.002 * (1 + i) for i, k in enumerate(DENSE_FIT_KEYS)}
    mk = lambda: W.make_pset(p, mode, scalar_ell=(True, False), fixed=('Zf', 'noise'), lr=lr, trailing_axis=True)
    rows = np.random.RandomState(5).randint(300, size=(4, 64))
    scale = 300.0 / 64.0

    host = mk()
    hist_h = R.host_loop(W.RefEngine(X, Y, mode), host, rows, 1e-6, scale)

    eng = RefFitEngine(X, Y)
    dev = mk()
    fit = WhiteDeviceFit(eng, dev)
    full = mode == W.WHITE_FULL
    assert fit.mode == mode and fit.full == full
    assert fit.shape == dict(Mf=7, Mg=5, D=2) and fit.ell_size == (1, 2)
    assert fit.sizes == [14, 10, 7, 5, 28 if full else 7, 15 if full else 5, 1, 2, 1, 1, 1]
    assert fit.positive == [False, False, False, False, not full, not full, True, True, True, True, True]
    assert fit.trainable == [False, True, True, True, True, True, True, True, True, True, False]
    assert fit.lr == [lr[k] for k in DENSE_FIT_KEYS]
    o = np.concatenate([[0], np.cumsum(fit.sizes)])
    assert fit.x.size == o[-1] == fit.m.size == fit.v.size
    if full:
        for b, k in ((4, 'u_fs_sqrt'), (5, 'u_gs_sqrt')):
            q = dev.params[k]
            assert np.array_equal(fit.x[o[b]:o[b + 1]], q.transform.backward(q.value))
            M = q.value.shape[0]
            assert np.array_equal(fit.x[o[b]:o[b + 1]], np.concatenate([q.value[i, :i + 1, 0] for i in range(M)]))     # row-major lower triangle
    x0 = fit.x.copy()
    ed, kl = fit.steps(rows, 64, 1e-6, scale)
    assert fit.t == 4 and eng.calls[0]['t0'] == 0 and eng.calls[0]['n_steps'] == 4 and eng.calls[0]['mode'] == mode
    assert np.allclose(np.stack([ed, kl], 1), hist_h, rtol=1e-12, atol=0)
    for k in DENSE_FIT_KEYS:
        a, b = dev.params[k].value.reshape(-1), host.params[k].value.reshape(-1)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), k
    assert dev.params['u_fm'].value.shape == (7, 1) and np.max(np.abs(dev.params['u_fm'].value - p['u_fm'])) > 1e-3     # it did move
    if full:
        for k, M in (('u_fs_sqrt', 7), ('u_gs_sqrt', 5)):
            val = dev.params[k].value
            assert val.shape == (M, M, 1) and not np.triu(val[:, :, 0], 1).any() and np.max(np.abs(val[:, :, 0] - np.tril(p[k]))) > 1e-4
    # fixed blocks: value, x, m, v untouched
    assert np.array_equal(dev.params['Zf'].value, p['Zf']) and float(dev.params['noise'].value[0]) == p['noise']
    for b in (0, 10):
        assert np.array_equal(fit.x[o[b]:o[b + 1]], x0[o[b]:o[b + 1]]) and not fit.m[o[b]:o[b + 1]].any() and not fit.v[o[b]:o[b + 1]].any()
    assert fit.m[o[4]:o[5]].any() and fit.v[o[5]:o[6]].any()
    # a failure in step 2 of 5: two updates applied, t advances by two, the exception carries their history
    eng.fail_at = 2
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        fit.steps(np.random.RandomState(6).randint(300, size=(5, 64)), 64, 1e-6, scale)
    assert fit.t == 6 and ei.value.steps_applied == 2 and len(ei.value.elbo_data) == 2 and eng.calls[-1]['t0'] == 4
    assert np.array_equal(dev.params['u_gm'].value.reshape(-1), fit.x[o[3]:o[4]])
    # outside changes: an assignment (mode 2: to a factor, garbage above the diagonal included), a parameter fixed, a new learning rate
    eng.fail_at = None
    dev.params['u_gm'].value = np.full_like(dev.params['u_gm'].value, 0.75)
    if full:
        new = np.tril(0.1 * np.ones((5, 5))) + np.eye(5) + np.triu(9.0 * np.ones((5, 5)), 1)
        dev.params['u_gs_sqrt'].value = new[:, :, None]
    dev.params['var_g'].fixed = True
    dev.params['Zg'].learning_rate = 0.5
    fit.steps(None, 0, 1e-6, 1.0, n_steps=1)
    c = eng.calls[-1]
    assert np.all(c['x'][o[3]:o[4]] == 0.75) and c['trainable'][9] is False and c['lr'][1] == 0.5 and c['t0'] == 6 and fit.t == 7
    if full:
        assert np.array_equal(c['x'][o[5]:o[6]], new[np.tril_indices(5)])
        assert not np.triu(dev.params['u_gs_sqrt'].value[:, :, 0], 1).any()       # sync_params restored the exact zeros
    fit.x[o[2]:o[3]] = np.nan
    fit.sync_params()
    assert not fit._stale()
    fit.resync(reset=True)
    assert fit.t == 0 and not fit.m.any()


def test_white_device_fit_refuses_what_the_device_loop_does_not_do():
    from zigp.optim import WhiteDeviceFit, P
    from zigp.transforms import Log1pe, Identity, LowerTriangular
    X, Y, p0 = make_problem(50, 4, 2, seed=1)
    for mode in MODES:
        p = W.problem(p0, mode)
        ps = W.make_pset(p, mode)
        ps.params['mean_b'] = P(np.zeros(1))
        with pytest.raises(ValueError, match='mean-function'):
            WhiteDeviceFit(None, ps)
        ps = W.make_pset(p, mode)
        ps.params['noise'].transform = Log1pe(lower=1e-3)
        with pytest.raises(ValueError, match='lower'):
            WhiteDeviceFit(None, ps)

        class Exp:
            pass
        ps = W.make_pset(p, mode)
        ps.params['var_f'].transform = Exp()
        with pytest.raises(ValueError, match='unsupported transform'):
            WhiteDeviceFit(None, ps)
    # one latent full, the other diagonal
    pf = W.problem(p0, W.WHITE_FULL)
    ps = W.make_pset(pf, W.WHITE_FULL)
    ps.params['u_gs_sqrt'] = P(np.asarray(p0['u_gs_sqrt'], dtype=np.float64), Log1pe())
    with pytest.raises(ValueError, match='both'):
        WhiteDeviceFit(None, ps)
    # a diagonal q(u) that is not Log1pe(1e-6); a factor of the wrong size
    ps = W.make_pset(W.problem(p0, W.WHITE), W.WHITE)
    ps.params['u_fs_sqrt'].transform = Identity()
    ps.params['u_gs_sqrt'].transform = Identity()
    with pytest.raises(ValueError, match='Log1pe'):
        WhiteDeviceFit(None, ps)
    ps = W.make_pset(W.problem(p0, W.WHITE), W.WHITE)
    ps.params['u_fs_sqrt'].transform = Log1pe(lower=1e-4)
    with pytest.raises(ValueError, match='lower'):
        WhiteDeviceFit(None, ps)
    ps = W.make_pset(pf, W.WHITE_FULL)
    ps.params['u_fs_sqrt'] = P(np.eye(3), LowerTriangular(3))
    with pytest.raises(ValueError, match='LowerTriangular'):
        WhiteDeviceFit(None, ps)


@pytest.mark.parametrize('mode', MODES)
def test_one_step_of_the_restatement_is_one_adam_groups_step(mode):
    """white_fit_ref.ref_fit_steps, one step from t0 = 0 with zero moments, against AdamGroups.step on the same ParamSet with the same
    gradient: free vectors, moments and constrained values to 1e-14 of each block's largest entry."""
    from zigp.optim import AdamGroups, DENSE_FIT_KEYS
    X, Y, p0 = make_problem(200, 6, 2, seed=4, Mg=4, ell=0.4)
    p = W.problem(p0, mode, lq_seed=2, negative=1)
    lr = {k: 0.004 * (1 + i) for i, k in enumerate(DENSE_FIT_KEYS)}
    pset = W.make_pset(p, mode, scalar_ell=(False, True), fixed=('Zg',), lr=lr)
    x, sizes, lrs, positive, trainable = W.flat_state(pset)
    shape = dict(Mf=6, Mg=4, D=2)
    assert sizes == W.block_sizes(mode, shape, (2, 1))
    m, v = np.zeros_like(x), np.zeros_like(x)
    o = np.concatenate([[0], np.cumsum(sizes)])
    # both start from the same free vector exactly: the constrained values are its images (forward(backward(value)) is the value to rounding only)
    for b, k in enumerate(DENSE_FIT_KEYS):
        pset.params[k].set_free(x[o[b]:o[b + 1]].copy())      # (Identity.forward returns its argument: no view into x)
    opt = AdamGroups(pset)
    for b, k in enumerate(DENSE_FIT_KEYS):
        if trainable[b]:
            opt.x[k] = x[o[b]:o[b + 1]].copy()
    eg = W.ref_elbo_grad(mode)
    ed, kl = W.ref_fit_steps(mode, eg, X, Y, shape, x, m, v, lrs, positive, trainable, (2, 1), 0, 1, jitter=1e-6, scale=1.5)
    e2, k2, g = W.RefEngine(X, Y, mode).elbo(R.values(pset), jitter=1e-6, scale=1.5)
    assert e2 == ed[0] and k2 == kl[0]
    opt.step(R.fold(pset, g))
    for b, k in enumerate(DENSE_FIT_KEYS):
        sl = slice(o[b], o[b + 1])
        if not trainable[b]:
            assert k not in opt.x and not m[sl].any()
            continue
        for got, want in ((x[sl], opt.x[k]), (m[sl], opt.m[k]), (v[sl], opt.v[k])):
            assert got.shape == want.shape
            assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want)), (k, np.max(np.abs(got - want)))
        assert np.max(np.abs(pset.params[k].transform.forward(x[sl]).reshape(-1) - pset.params[k].value.reshape(-1))) <= 1e-14 * np.max(np.abs(pset.params[k].value))


@pytest.mark.parametrize('mode', MODES)
def test_two_host_runs_measure_stands_on_the_gpu_test_s_problems(mode):
    """The GPU test's yardstick with the CPU references standing in for the engine: on make_problem(3000, 96, 3, seed=17, Mg=70, ell=0.12),
    25 steps of 512 rows, two host runs that differ by a seeded +-1 ulp per element and step end d_par = 1.8e-13 (whitened) / 2.2e-13
    (full, make_lq(seed=3)) apart, d_hist = 5.6e-15 / 1.3e-14: 8 d is a bound that can show something."""
    X, Y, p0 = dense_problem()
    p = W.problem(p0, mode, lq_seed=3)
    rows = np.random.RandomState(11).randint(X.shape[0], size=(25, 512))
    scale = X.shape[0] / 512.0
    a, b = W.make_pset(p, mode), W.make_pset(p, mode)
    ha = R.host_loop(W.RefEngine(X, Y, mode), a, rows, 1e-6, scale)
    hb = R.host_loop(W.RefEngine(X, Y, mode), b, rows, 1e-6, scale, nudge_seed=1)
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    print('mode %d, 25 steps: d_par %.2e d_hist %.2e' % (mode, d_par, d_hist))
    assert 0 < 8 * max(d_par, d_hist) <= 1e-9
