"""GPU tests of the heads' fit loop on the device (zigp_kron_head_fit_steps, DenseEngine.kron_head_fit_steps,
onofftf.heads.HeadDeviceFit, fit_head(device_loop=True)) and of zigp_kron_head_elbo_rows.

Two yardsticks, as for the dense loop (tests/test_gpu_dense_fit.py):
* one step against the reference restated on the CPU: oracle/zigp_oracle_torch.kron_head_elbo_and_grad (torch autograd) on the step's
  rows, chained through the Log1pe transform and stepped by NumPy Adam (head_fit_ref.ref_head_fit_steps), at the project's gradient bar
  (1e-6 of a block's largest entry) and its ELBO bars (1e-7 data term; 1e-7 KL, the heads' own KL bar in tests/test_gpu_heads.py);
* 60 steps against the host loop the device loop replaces (kron_head_elbo + AdamGroups on the same engine, same rows).  The tolerance
  comes from the yardstick: the host loop is run a second time with every free-state element moved by a seeded +-1 ulp after every
  step, d = how far the two host runs end apart, and the device loop must lie within max(8 d, 1e-13) of the clean host run
  (head_fit_ref.bound).  8 d <= 1e-7 is required (an order under the 1e-6 gradient bar: beyond it the comparison shows nothing); with
  the oracle standing in for the engine d is <= 6e-14 at (6, 5), <= 4e-11 at (32, 32) and <= 1.2e-9 at (10, 100) on these inputs.
"""
import numpy as np
import pytest

import head_fit_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('grid', [(6, 5), (10, 40)])
def test_one_step_matches_the_reference_restatement(engine, grid, lik):
    """One zigp_kron_head_fit_steps step on rows [700, 1200) of the resident set, a different learning rate per block, f_ind/z_1 fixed:
    from t0 = 0 with zero moments and from t0 = 37 with given non-zero m and v.  (10, 40) runs the larger-grid kernels below their
    capacity.  m per block to 1e-6 of the block's largest entry, x to 1e-6 of the largest move of its block, v to 2e-6, the history entry
    to 1e-7 (data term and KL); untrainable blocks (the fixed one, the head's absent noise / f_mu) bit-unchanged."""
    from onofftf.heads import HEAD_FIT_BLOCK_NAMES
    X, Y, mk = R.head_problem(grid, lik)
    engine.set_data(X, Y)
    pset = mk()
    for i, k in enumerate(HEAD_FIT_BLOCK_NAMES):
        if k in pset.params:
            pset.params[k].learning_rate = 0.003 * (1 + i)
    pset.params['f_ind/z_1'].fixed = True
    x0, lr, positive, trainable, shape = R.flat_state(pset)
    assert trainable[1] is False and sum(trainable) == 8      # the fixed block and the head's absent one (f_mu / noise) are not trained
    offs = np.concatenate([[0], np.cumsum(R.block_sizes(shape))])
    rs = np.random.RandomState(8)
    for t0, m0, v0 in ((0, np.zeros_like(x0), np.zeros_like(x0)), (37, 0.3 * rs.randn(x0.size), 0.2 * rs.rand(x0.size) + 1e-3)):
        xr, mr, vr = x0.copy(), m0.copy(), v0.copy()
        ed_r, kl_r = R.ref_head_fit_steps(R.oracle_eg(lik), X, Y, shape, xr, mr, vr, lr, positive, trainable, t0, [700], R.BATCH, jitter=R.JITTER,
                                          scale=R.SCALE)
        x, m, v = x0.copy(), m0.copy(), v0.copy()
        ed, kl = engine.kron_head_fit_steps(shape, lik, x, m, v, lr, positive, trainable, t0, [700], R.BATCH, jitter=R.JITTER, scale=R.SCALE)
        assert int(engine.lib.zigp_kron_fit_steps_applied(engine.ctx)) == 1
        print('%s %s t0 %d: elbo_data %.10e (ref %.10e) kl %.10e (ref %.10e)' % (grid, lik, t0, ed[0], ed_r[0], kl[0], kl_r[0]))
        assert abs(ed[0] - ed_r[0]) <= 1e-7 * abs(ed_r[0]) and abs(kl[0] - kl_r[0]) <= 1e-7 * abs(kl_r[0])
        for b, k in enumerate(HEAD_FIT_BLOCK_NAMES):
            sl = slice(offs[b], offs[b + 1])
            if not trainable[b]:
                assert np.array_equal(x[sl], x0[sl]) and np.array_equal(m[sl], m0[sl]) and np.array_equal(v[sl], v0[sl]), k
                continue
            em = np.max(np.abs(m[sl] - mr[sl])) / np.max(np.abs(mr[sl]))
            move = np.max(np.abs(xr[sl] - x0[sl]))
            ex = np.max(np.abs(x[sl] - xr[sl])) / move
            ev = np.max(np.abs(v[sl] - vr[sl])) / np.max(np.abs(vr[sl]))
            print('  %-22s m relerr %.2e  x err / largest move %.2e (move %.2e)  v relerr %.2e' % (k, em, ex, move, ev))
            assert em < 1e-6 and ex < 1e-6 and ev < 2e-6, (k, em, ex, ev)


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('grid', [(6, 5), (32, 32), (10, 100)])
def test_60_steps_in_three_calls_match_the_host_loop(engine, grid, lik):
    """60 minibatch steps (500 rows of 3000) in calls of 20 + 20 + 20, one host wrap-around batch mid-way, against the host loop on the
    same rows: parameters and history within max(8 d, 1e-13) of the clean host run, d from the +-1-ulp-nudged host run; 8 d <= 1e-7; a
    variational mean moved by more than 1e-2.  The test prints its figures."""
    from onofftf.heads import HeadDeviceFit
    X, Y, mk = R.head_problem(grid, lik)
    seq, wi = R.rows_with_a_wrap(60)
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    a, b, dv = mk(), mk(), mk()
    u0 = a.params['f_ind/value'].value.copy()
    ha = R.host_loop(engine, a, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps)
    hb = R.host_loop(engine, b, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps, nudge_seed=1)
    engine.set_data(X, Y)
    fit = HeadDeviceFit(engine, dv, lik)
    hist = []
    for lo in (0, 20, 40):
        part = seq[lo:lo + 20]
        ed, kl = fit.steps(part, R.BATCH, R.JITTER, R.SCALE, *(wraps if -1 in part else (None, None)))
        assert int(engine.lib.zigp_kron_fit_steps_applied(engine.ctx)) == 20
        hist.append(np.stack([ed, kl], 1))
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    e_par, e_hist = R.block_distance(dv, a), R.hist_distance(np.concatenate(hist), ha)
    moved = float(np.max(np.abs(dv.params['f_ind/value'].value - u0)))
    print('grid %s %s, 60 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e) | '
          'largest move of u: %.3f' % (grid, lik, d_par, d_hist, e_par, R.bound(d_par), e_hist, R.bound(d_hist), moved))
    assert 8 * max(d_par, d_hist) <= 1e-7, 'the problem is too ill-conditioned for this comparison to show anything'
    assert moved > 1e-2 and fit.t == 60
    assert e_par <= R.bound(d_par) and e_hist <= R.bound(d_hist)


def test_cholesky_failure_in_step_0_leaves_the_state_alone(engine):
    """Two coincident spatial inducing points, jitter 0: ZIGP_ENOTPD whose message names step 0 and this call, the state bit-unchanged,
    zigp_kron_fit_steps_applied = 0, an empty history; the context is usable afterwards."""
    import zigp
    from onofftf.heads import HeadDeviceFit, head_engine_params
    X, Y, mk = R.head_problem((6, 5), 'gaussian')
    engine.set_data(X, Y)
    ps = mk()
    z = ps.params['f_ind/z_0'].value
    z[5] = z[2]
    fit = HeadDeviceFit(engine, ps, 'gaussian')
    fit.m[:] = 0.25
    fit.v[:] = 0.5
    x0 = fit.x.copy()
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        fit.steps([0, 500, 1000], R.BATCH, 0.0, R.SCALE)
    print(str(ei.value))
    assert 'step 0' in str(ei.value) and 'zigp_kron_head_fit_steps' in str(ei.value)
    assert ei.value.steps_applied == 0 and len(ei.value.elbo_data) == 0 and len(ei.value.kl) == 0
    assert int(engine.lib.zigp_kron_fit_steps_applied(engine.ctx)) == 0 and fit.t == 0
    assert np.array_equal(fit.x, x0) and np.all(fit.m == 0.25) and np.all(fit.v == 0.5)
    good = mk()
    assert np.isfinite(engine.kron_head_elbo(head_engine_params(good), X[:300], Y[:300], 'gaussian', jitter=R.JITTER, need_grad=False)[0])


def test_a_head_fit_call_changes_nothing_for_the_calls_that_follow(engine):
    """kron_elbo (two latents), kron_head_elbo and kron_head_predict on the same context return bit for bit what they returned before a
    head fit call; the resident data set stays."""
    from test_gpu_kron import make_kron_problem
    from onofftf.heads import HeadDeviceFit, head_engine_params, head_f_mu
    Xo, Yo, po = make_kron_problem(400, 6, 7, seed=9)
    X, Y, mk = R.head_problem((10, 40), 'bernoulli')
    engine.set_data(X, Y)
    ph, fmu = head_engine_params(mk()), 0.2
    before = (engine.kron_elbo(po, Xo, Yo, jitter=1e-5, scale=2.0), engine.kron_head_elbo(ph, X[:600], Y[:600], 'bernoulli', scale=5.0, f_mu=fmu),
              engine.kron_head_predict(ph, X[:300], 'bernoulli', f_mu=fmu), engine.kron_head_elbo(ph, lik='bernoulli', rows=(100, 700), f_mu=fmu))
    for lik, grid in (('bernoulli', (10, 40)), ('gaussian', (6, 5))):
        fit = HeadDeviceFit(engine, R.head_problem(grid, lik)[2](), lik)
        fit.steps([0, 1200, 2500], R.BATCH, R.JITTER, R.SCALE)
    after = (engine.kron_elbo(po, Xo, Yo, jitter=1e-5, scale=2.0), engine.kron_head_elbo(ph, X[:600], Y[:600], 'bernoulli', scale=5.0, f_mu=fmu),
             engine.kron_head_predict(ph, X[:300], 'bernoulli', f_mu=fmu), engine.kron_head_elbo(ph, lik='bernoulli', rows=(100, 700), f_mu=fmu))

    def same(g0, g1):
        return all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
                   for k in g0 for a, b in (zip(g0[k], g1[k]) if isinstance(g0[k], list) else [(g0[k], g1[k])]))

    for i in (0, 1, 3):
        assert before[i][0] == after[i][0] and before[i][1] == after[i][1] and same(before[i][2], after[i][2]), i
    assert np.array_equal(before[2], after[2])


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('grid', [(6, 5), (10, 100), (40, 40)])
def test_head_elbo_on_resident_rows_equals_the_host_array_call(engine, grid, lik):
    """kron_head_elbo(rows=(lo, hi)) = the same call on the host arrays X[lo:hi], Y[lo:hi], bit for bit: the fused kernels at both
    capacities and, at 40 x 40, the panel path (rows copied device to device)."""
    from onofftf.heads import head_engine_params
    X, Y, mk = R.head_problem(grid, lik)
    engine.set_data(X, Y)
    p = head_engine_params(mk())
    lo, hi = 333, 1110
    a = engine.kron_head_elbo(p, X[lo:hi], Y[lo:hi], lik, jitter=R.JITTER, scale=3.5, f_mu=0.1)
    b = engine.kron_head_elbo(p, lik=lik, jitter=R.JITTER, scale=3.5, f_mu=0.1, rows=(lo, hi))
    assert a[0] == b[0] and a[1] == b[1]
    for k in a[2]:
        for u, w in (zip(a[2][k], b[2][k]) if isinstance(a[2][k], list) else [(a[2][k], b[2][k])]):
            assert np.array_equal(np.asarray(u), np.asarray(w)), k
    with pytest.raises(ValueError, match='row range'):
        engine.kron_head_elbo(p, lik=lik, rows=(2900, 3001))
    with pytest.raises(ValueError, match='not both'):
        engine.kron_head_elbo(p, X[:10], Y[:10], lik, rows=(0, 10))


def test_head_fit_steps_argument_checks(engine):
    """ValueError with the cause named, nothing applied: lik = 'onoff', a wrong n_free, a row range past the resident set, a 40 x 40 grid."""
    X, Y, mk = R.head_problem((6, 5), 'gaussian')
    engine.set_data(X, Y)
    x, lr, positive, trainable, shape = R.flat_state(mk())
    big = dict(M0f=40, M1f=40, D0=2, D1=1)

    def call(shape=shape, lik='gaussian', n_free=x.size, row_begin=(0,), t0=0):
        state = [np.resize(x, n_free).copy(), np.full(n_free, 0.25), np.full(n_free, 0.5)]
        held = [a.copy() for a in state]
        try:
            engine.kron_head_fit_steps(shape, lik, held[0], held[1], held[2], lr, positive, trainable, t0, list(row_begin), R.BATCH, jitter=R.JITTER,
                                       scale=R.SCALE)
        finally:
            call.unchanged = all(np.array_equal(a, b) for a, b in zip(held, state))

    call()
    assert not call.unchanged and int(engine.lib.zigp_kron_fit_steps_applied(engine.ctx)) == 1
    for match, kw in (("'gaussian' or 'bernoulli'", dict(lik='onoff')),
                      ('n_free', dict(n_free=x.size + 1)),
                      ('row range', dict(row_begin=(0, R.N_ROWS - R.BATCH + 1))),           # rows [2501, 3001): one past the resident set
                      ('beyond the fused', dict(shape=big, n_free=sum(R.block_sizes(big))))):
        with pytest.raises(ValueError, match=match):
            call(**kw)
        assert call.unchanged, match
    assert int(engine.lib.zigp_kron_fit_steps_applied(engine.ctx)) == 0      # a refused call applied nothing
    with pytest.raises(ValueError):
        call(t0=-1)
    call()
    assert not call.unchanged


def test_svgp_end_to_end_runs_its_loop_on_the_device(tmp_path, engine):
    """scripts.svgp.svgp on the pptr fixture, 150 iterations at a 10 x 20 grid with the default device loop: two fit calls or more and no
    kron_head_elbo call (counted on the engine object), 150 history entries that decrease (mean of the last 20 against the first 20);
    device_loop=False makes no fit call."""
    from scripts.svgp import svgp
    from test_gpu_onofftf import _pptr
    Xtr, Ytr, Xte, Yte = _pptr()
    counts = dict(fit=0, elbo=0)
    fit_steps, elbo = engine.kron_head_fit_steps, engine.kron_head_elbo
    engine.kron_head_fit_steps = lambda *a, **k: (counts.__setitem__('fit', counts['fit'] + 1), fit_steps(*a, **k))[1]
    engine.kron_head_elbo = lambda *a, **k: (counts.__setitem__('elbo', counts['elbo'] + 1), elbo(*a, **k))[1]
    try:
        hist = []
        np.random.seed(0)
        out = svgp(Xtr, Ytr, Xte[:2000], Yte[:2000], str(tmp_path) + '/', num_iter=150, num_inducing_f=(10, 20), engine=engine, kmeans_seed=1,
                   history=hist)
        assert counts['fit'] >= 2 and counts['elbo'] == 0
        assert len(hist) == 150 and np.mean(hist[-20:]) < np.mean(hist[:20])
        assert np.isfinite(out['test_rmse'])
        counts.update(fit=0, elbo=0)
        h2 = []
        svgp(Xtr[:5000], Ytr[:5000], Xte[:200], Yte[:200], None, num_iter=3, num_inducing_f=(10, 20), engine=engine, kmeans_seed=1, history=h2,
             device_loop=False)
        assert counts['fit'] == 0 and counts['elbo'] == 3 and len(h2) == 3
    finally:
        del engine.kron_head_fit_steps, engine.kron_head_elbo
