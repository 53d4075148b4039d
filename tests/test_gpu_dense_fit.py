"""GPU tests of the dense fit loop on the device (zigp_fit_steps, DenseEngine.fit_steps, zigp.optim.DenseDeviceFit,
OnOffSVGP.optimize(method='adam')).

Two yardsticks:
* one step against the reference restated on the CPU: oracle/zigp_oracle_torch.elbo_and_grad (torch autograd) on the gathered rows,
  chained through the Log1pe transform and stepped by NumPy Adam (dense_fit_ref.ref_fit_steps), at the project's gradient bar (1e-6 of a
  block's largest entry, tests/test_gpu_dense.py) and its ELBO bar (1e-7 data term, 1e-8 KL);
* many steps against the host loop the device loop replaces (select_rows + elbo + AdamGroups on the same engine, same row samples).  Its
  tolerance is derived from the yardstick itself: the host loop is run a second time with every free-state element moved by a seeded
  +-1 ulp after every step, d = how far the two host runs end apart (worst parameter block relative to the block's largest entry; worst
  relative difference over the ELBO history), and the device loop must lie within max(8 d, 1e-13) of the clean host run -- 8: at every
  step the device's softplus and sigmoid may each differ from NumPy's by up to 2 ulp, in the value and in the chain factor (4), times 2
  for the per-row form of the Kuf-cotangent reductions every fit step uses; 1e-13 ~ 2 eps x n_steps.  8 d <= 1e-9 is required of the
  200-step problem (else it is too ill-conditioned to show anything): its lengthscales give cond(Kuu) ~ 1e3 (checked without a GPU in
  test_cpu_dense_fit.py with the oracle standing in for the engine: d ~ 4e-12 after 200 steps).
"""
import numpy as np
import pytest

from conftest import make_problem
import dense_fit_ref as R
from test_cpu_dense_fit import dense_problem

pytestmark = pytest.mark.gpu


def _bound(d):
    return max(8.0 * d, 1e-13)


def _oracle_eg(Xb, Yb, p, jitter, scale):
    import zigp_oracle_torch as ot
    elbo, data, kl, g = ot.elbo_and_grad(Xb, Yb, p, jitter, scale=scale)
    return scale * data, kl, g


def _flat_state(pset):
    from zigp.optim import DENSE_FIT_KEYS
    ps = [pset.params[k] for k in DENSE_FIT_KEYS]
    return (np.concatenate([q.free() for q in ps]), [q.value.size for q in ps], [float(q.learning_rate) for q in ps],
            [type(q.transform).__name__ == 'Log1pe' for q in ps], [not q.fixed for q in ps])


@pytest.mark.parametrize('D,scalar_ell,fixed', [(3, (False, False), ()), (2, (True, True), ('Zf', 'noise'))])
def test_one_step_matches_the_reference_restatement(engine, D, scalar_ell, fixed):
    """One zigp_fit_steps step on 512 sampled rows (with repeats) of make_problem(3000, 96, D, Mg=70), scale N / 512, a different learning
    rate per block: from t0 = 0 with zero moments, and from t0 = 37 with given non-zero m and v.  m per block to 1e-6 of the block's
    largest entry, x to 1e-6 of the largest move of its block, the history entry to 1e-7 (data term) / 1e-8 (KL)."""
    from zigp.optim import DENSE_FIT_KEYS
    X, Y, p = make_problem(3000, 96, D, Mg=70)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    lr = {k: 0.003 * (1 + i) for i, k in enumerate(DENSE_FIT_KEYS)}
    pset = R.make_pset(p, scalar_ell=scalar_ell, fixed=fixed, lr=lr)
    x0, sizes, lrs, positive, trainable = _flat_state(pset)
    ell_size = (sizes[6], sizes[7])
    shape = dict(Mf=96, Mg=70, D=D)
    rows = np.random.RandomState(4).randint(3000, size=512)
    assert len(np.unique(rows)) < 512
    scale = 3000.0 / 512.0
    rs = np.random.RandomState(8)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for t0, m0, v0 in ((0, np.zeros_like(x0), np.zeros_like(x0)), (37, 0.3 * rs.randn(x0.size), 0.2 * rs.rand(x0.size) + 1e-3)):
        xr, mr, vr = x0.copy(), m0.copy(), v0.copy()
        ed_r, kl_r = R.ref_fit_steps(_oracle_eg, X, Y, shape, xr, mr, vr, lrs, positive, trainable, ell_size, t0, 1, rows=rows, batch=512,
                                     jitter=1e-6, scale=scale)
        x, m, v = x0.copy(), m0.copy(), v0.copy()
        ed, kl = engine.fit_steps(shape, x, m, v, lrs, positive, trainable, ell_size, t0, 1, rows=rows, batch=512, jitter=1e-6, scale=scale)
        assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == 1
        print('t0 %d: elbo_data %.10e (ref %.10e) kl %.10e (ref %.10e)' % (t0, ed[0], ed_r[0], kl[0], kl_r[0]))
        assert abs(ed[0] - ed_r[0]) <= 1e-7 * abs(ed_r[0]) and abs(kl[0] - kl_r[0]) <= 1e-8 * abs(kl_r[0])
        for b, k in enumerate(DENSE_FIT_KEYS):
            sl = slice(offs[b], offs[b + 1])
            if not trainable[b]:
                assert np.array_equal(x[sl], x0[sl]) and np.array_equal(m[sl], m0[sl]) and np.array_equal(v[sl], v0[sl]), k
                continue
            em = np.max(np.abs(m[sl] - mr[sl])) / np.max(np.abs(mr[sl]))
            move = np.max(np.abs(xr[sl] - x0[sl]))
            ex = np.max(np.abs(x[sl] - xr[sl])) / move
            ev = np.max(np.abs(v[sl] - vr[sl])) / np.max(np.abs(vr[sl]))
            print('  %-10s m relerr %.2e  x err / largest move %.2e (move %.2e)  v relerr %.2e' % (k, em, ex, move, ev))
            assert em < 1e-6 and ex < 1e-6 and ev < 2e-6, (k, em, ex, ev)
    engine.select_rows(None)


def _three_runs(engine, mk, rows, jitter, scale, calls, n_steps=None):
    """clean host run, nudged host run, device run in `calls` calls; returns (d_par, d_hist, e_par, e_hist, device pset)"""
    from zigp.optim import DenseDeviceFit
    a, b, dv = mk(), mk(), mk()
    ha = R.host_loop(engine, a, rows, jitter, scale, n_steps=n_steps)
    hb = R.host_loop(engine, b, rows, jitter, scale, n_steps=n_steps, nudge_seed=1)
    fit = DenseDeviceFit(engine, dv)
    hist, o = [], 0
    for n in calls:
        if rows is None:
            ed, kl = fit.steps(None, 0, jitter, scale, n_steps=n)
        else:
            ed, kl = fit.steps(rows[o:o + n], rows.shape[1], jitter, scale)
        assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == n
        hist.append(np.stack([ed, kl], 1))
        o += n
    hd = np.concatenate(hist)
    assert fit.t == sum(calls)
    return R.block_distance(b, a), R.hist_distance(hb, ha), R.block_distance(dv, a), R.hist_distance(hd, ha), dv


def test_200_steps_in_three_calls_match_the_host_loop(engine):
    """200 minibatch steps (512 rows each) in calls of 80 + 80 + 40 against the host loop on the same row samples.
    Measured on an MI355X: the two host runs end d = 6.3e-13 (parameters) / 8.1e-13 (ELBO history) apart, the device loop 3.2e-13 / 8.6e-13
    from the clean host run (bounds 5.1e-12 / 6.5e-12); the largest move of a variational mean is 1.12.  The test prints its figures."""
    X, Y, p = dense_problem()
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    rows = np.random.RandomState(11).randint(X.shape[0], size=(200, 512))
    scale = X.shape[0] / 512.0
    d_par, d_hist, e_par, e_hist, dv = _three_runs(engine, lambda: R.make_pset(p), rows, 1e-6, scale, (80, 80, 40))
    moved = max(np.max(np.abs(dv.params[k].value - p[k])) for k in ('u_fm', 'u_gm'))
    print('200 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e) | '
          'largest move of a u: %.3f' % (d_par, d_hist, e_par, _bound(d_par), e_hist, _bound(d_hist), moved))
    assert 8 * max(d_par, d_hist) <= 1e-9, 'the problem is too ill-conditioned for this comparison to show anything'
    assert moved > 1e-2
    assert e_par <= _bound(d_par) and e_hist <= _bound(d_hist)


def test_full_batch_adam_over_the_active_rows_in_several_chunks(engine):
    """rows = NULL: 20 full-batch steps over 40 000 active rows (a zigp_select_rows selection of a 45 000-row resident set) at M = 256 with
    zigp_set_chunk(16384): three chunks per step.  Same comparison, same bound; the selection is honoured and left as found."""
    X, Y, p = make_problem(45000, 256, 3, seed=23, ell=0.085)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    sel = np.random.RandomState(2).permutation(45000)[:40000]
    engine.select_rows(sel)
    assert engine.N == 40000
    before = engine.elbo(p, jitter=1e-6)
    d_par, d_hist, e_par, e_hist, dv = _three_runs(engine, lambda: R.make_pset(p, lr=0.005), None, 1e-6, 1.0, (20,), n_steps=20)
    print('full batch, 20 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e)'
          % (d_par, d_hist, e_par, _bound(d_par), e_hist, _bound(d_hist)))
    assert e_par <= _bound(d_par) and e_hist <= _bound(d_hist)
    assert engine.N == 40000
    after = engine.elbo(p, jitter=1e-6)
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(before[2][k], after[2][k]) for k in before[2])
    # the selection mattered: the whole resident set gives another number
    engine.select_rows(None)
    assert engine.elbo(p, jitter=1e-6, need_grad=False)[0] != before[0]
    engine.set_chunk(16384)


def test_cholesky_failure_in_step_0_leaves_the_state_alone(engine):
    """Two coincident inducing points of g, jitter 0: ZIGP_ENOTPD with the step and the latent in the message, the state bit-unchanged,
    zigp_fit_steps_applied = 0, an empty history.  (An error-code path through the Cholesky status word; the step enqueued behind the
    failed one runs and its update is skipped.)"""
    import zigp
    X, Y, p = make_problem(2000, 40, 2, seed=5, Mg=30, ell=0.3)
    p['Zg'][7] = p['Zg'][3]
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    pset = R.make_pset(p)
    x0, sizes, lrs, positive, trainable = _flat_state(pset)
    x, m, v = x0.copy(), np.full_like(x0, 0.25), np.full_like(x0, 0.5)
    rows = np.random.RandomState(1).randint(2000, size=(2, 256))
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        engine.fit_steps(dict(Mf=40, Mg=30, D=2), x, m, v, lrs, positive, trainable, (2, 2), 5, 2, rows=rows, batch=256, jitter=0.0, scale=2000 / 256.0)
    print(str(ei.value))
    assert 'step 0' in str(ei.value) and 'latent g' in str(ei.value)
    assert ei.value.steps_applied == 0 and len(ei.value.elbo_data) == 0 and len(ei.value.kl) == 0
    assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == 0
    assert np.array_equal(x, x0) and np.all(m == 0.25) and np.all(v == 0.5)
    # the context is usable afterwards
    p['Zg'][7] += 0.05
    assert np.isfinite(engine.elbo(p, jitter=1e-6, need_grad=False)[0])


def _toy(minibatch_size, seed=1):
    import os
    import scipy.io as sio
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    mat = sio.loadmat(os.path.join(os.path.dirname(__file__), 'golden', 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(seed)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=1.), onoffgpf.kernels.RBF(1, lengthscales=1., variance=5.),
                  OnOffLikelihood(), Z, Z.copy(), minibatch_size=minibatch_size)
    m.likelihood.variance = 0.01
    return m


def test_model_adam_runs_on_the_device_and_sees_the_host_loop_s_minibatches():
    """OnOffSVGP(minibatch_size=100).optimize(method='adam', maxiter=450): three fit_steps calls (200 + 200 + 50), no elbo call, the 450
    row samples the host loop draws from _rng, and the end state within max(8 d, 1e-13) of a twin stepped with a callback (= the host
    loop), d from a second host run on the same samples nudged by +-1 ulp per step.  With a callback no fit_steps call happens."""
    from zigp.optim import DENSE_FIT_KEYS
    dev, twin, third = _toy(100), _toy(100), _toy(100)
    calls, elbos = [], []
    eng = dev._engine
    fit_steps, elbo = eng.fit_steps, eng.elbo
    eng.fit_steps = lambda *a, **k: (calls.append((a[9], np.array(k['rows']).reshape(a[9], -1))), fit_steps(*a, **k))[1]
    eng.elbo = lambda *a, **k: (elbos.append(1), elbo(*a, **k))[1]
    dev.optimize(method='adam', maxiter=450, learning_rate=0.01)
    assert [c[0] for c in calls] == [200, 200, 50] and not elbos
    rows_dev = np.concatenate([c[1] for c in calls])
    # the twin: a callback keeps it on the host loop
    seen, tcalls = [], []
    teng = twin._engine
    sel, tfit = teng.select_rows, teng.fit_steps
    teng.select_rows = lambda idx=None: (seen.append(None if idx is None else np.array(idx)), sel(idx))[1]
    teng.fit_steps = lambda *a, **k: (tcalls.append(1), tfit(*a, **k))[1]
    twin.optimize(method='adam', maxiter=450, learning_rate=0.01, callback=lambda it, e: None)
    assert not tcalls and len(seen) == 450
    assert np.array_equal(rows_dev, np.stack(seen))
    # d: the same loop on the same samples, nudged
    ps3 = third._pset()
    for q in ps3.params.values():
        q.learning_rate = 0.01
    third._make_resident()
    R.host_loop(third._engine, ps3, rows_dev, 1e-6, 450.0 / 100.0, nudge_seed=1)
    d = R.block_distance(ps3, twin._pset())
    e = R.block_distance(dev._pset(), twin._pset())
    print('model, 450 steps: two host runs d %.3e | device - host %.3e (bound %.3e)' % (d, e, _bound(d)))
    assert e <= _bound(d)
    assert set(dev._pset().params) == set(DENSE_FIT_KEYS)
    assert np.isfinite(dev.compute_log_likelihood())


def test_a_fit_call_changes_nothing_for_the_calls_that_follow(engine):
    """zigp_elbo and zigp_predict on the same context return bit for bit what they returned before a fit call; the selection stays."""
    X, Y, p = make_problem(5000, 150, 3, seed=9, Mg=100, ell=0.2)
    engine.set_chunk(2048)
    engine.set_data(X, Y)
    sel = np.random.RandomState(3).randint(5000, size=3000)
    engine.select_rows(sel)
    e0 = engine.elbo(p, jitter=1e-6, scale=5000 / 3000.0)
    pr0 = engine.predict(p, X[:700], jitter=1e-6)
    pset = R.make_pset(p)
    x, sizes, lrs, positive, trainable = _flat_state(pset)
    m, v = np.zeros_like(x), np.zeros_like(x)
    rows = np.random.RandomState(4).randint(5000, size=(3, 1500))
    engine.fit_steps(dict(Mf=150, Mg=100, D=3), x, m, v, lrs, positive, trainable, (3, 3), 0, 3, rows=rows, batch=1500, jitter=1e-6, scale=5000 / 1500.0)
    engine.fit_steps(dict(Mf=150, Mg=100, D=3), x, m, v, lrs, positive, trainable, (3, 3), 3, 2, rows=None, jitter=1e-6, scale=5000 / 3000.0)
    assert engine.N == 3000
    e1 = engine.elbo(p, jitter=1e-6, scale=5000 / 3000.0)
    pr1 = engine.predict(p, X[:700], jitter=1e-6)
    assert e0[0] == e1[0] and e0[1] == e1[1] and all(np.array_equal(e0[2][k], e1[2][k]) for k in e0[2])
    assert np.array_equal(pr0, pr1)
    engine.select_rows(None)
    engine.set_chunk(16384)


def test_fit_steps_argument_checks(engine):
    X, Y, p = make_problem(1500, 20, 2, seed=2, Mg=12)
    engine.set_data(X, Y)
    pset = R.make_pset(p)
    x, sizes, lrs, positive, trainable = _flat_state(pset)
    m, v = np.zeros_like(x), np.zeros_like(x)
    shape = dict(Mf=20, Mg=12, D=2)
    rows = np.zeros((1, 64), dtype=np.int64)
    ok = lambda **kw: engine.fit_steps(kw.pop('shape', shape), kw.pop('x', x.copy()), kw.pop('m', m.copy()), kw.pop('v', v.copy()), lrs, positive, trainable,
                                       kw.pop('ell_size', (2, 2)), kw.pop('t0', 0), 1, rows=kw.pop('rows', rows), batch=64, jitter=1e-6)
    ok()
    with pytest.raises(ValueError, match='n_free'):
        ok(x=np.zeros(x.size + 1), m=np.zeros(x.size + 1), v=np.zeros(x.size + 1))
    with pytest.raises(ValueError, match='out of range'):
        ok(rows=np.full((1, 64), 1500, dtype=np.int64))
    with pytest.raises(ValueError, match='ell_size'):
        ok(ell_size=(2, 3))
    with pytest.raises(ValueError):
        ok(t0=-1)
    with pytest.raises(ValueError, match='D'):
        ok(shape=dict(Mf=20, Mg=12, D=3))
    engine.elbo(dict(p, mean_b=0.5), jitter=1e-6, need_grad=False)      # leaves a Constant mean function on the context
    with pytest.raises(ValueError, match='mean function'):
        ok()
    engine.elbo(p, jitter=1e-6, need_grad=False)
    ok()
