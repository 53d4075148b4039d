"""GPU tests of the dense fit loop on the device for the whitened models (zigp_fit_steps_mode, DenseEngine.fit_steps_mode,
zigp.optim.WhiteDeviceFit, OnOffSVGP.optimize(method='adam', device_loop=True)); mode 1 = ZIGP_FIT_WHITE (whitened, diagonal q(u)),
mode 2 = ZIGP_FIT_WHITE_FULL (whitened, full-covariance q(u)).

The two yardsticks of test_gpu_dense_fit.py, with the same bars and the same derivation (that file's docstring):
* one step against the reference restated on the CPU: whiten_ref / fullcov_ref.elbo_and_grad (torch autograd) on the gathered rows, chained
  through the transforms and stepped by NumPy Adam (white_fit_ref.ref_fit_steps): m and x to 1e-6 of the block's largest entry / largest
  move, v to 2e-6, data term 1e-7, KL 1e-8;
* many steps against the host loop the device loop replaces (select_rows + elbo + AdamGroups on the same engine, same row samples): the
  device run must lie within max(8 d, 1e-13) of the clean host run, d = how far a second host run nudged by a seeded +-1 ulp per element
  and step ends from it, in parameters and in the ELBO history; 8 d <= 1e-9 is required of the 200-step problem (checked without a GPU in
  test_cpu_white_fit.py).
"""
import numpy as np
import pytest

from conftest import make_problem
import dense_fit_ref as R
import white_fit_ref as W
from test_cpu_dense_fit import dense_problem

pytestmark = pytest.mark.gpu
MODES = [W.WHITE, W.WHITE_FULL]


def _bound(d):
    return max(8.0 * d, 1e-13)


ONE_STEP_CASES = [
    # mode, D, scalar_ell, fixed, Mf, Mg, ell
    (W.WHITE, 3, (False, False), (), 96, 70, 0.3),
    (W.WHITE, 2, (True, True), ('Zf', 'noise'), 96, 70, 0.3),
    (W.WHITE_FULL, 3, (False, False), (), 96, 70, 0.3),
    (W.WHITE_FULL, 2, (True, True), ('Zf', 'noise', 'u_gs_sqrt'), 96, 70, 0.3),
    # Mp = 256: the triangular M x M products (Lq Lq^T, C1 Lq) and the triangular pack cross a 128-block boundary.  Lengthscale 0.2:
    # cond(Kuu) = 3e5 / 1.4e6, so that the project's gradient bar max(1e-6, 1e-13 cond) is the 1e-6 used here (0.3 gives 2e8)
    (W.WHITE_FULL, 3, (False, False), (), 150, 130, 0.2),
]


@pytest.mark.parametrize('mode,D,scalar_ell,fixed,Mf,Mg,ell', ONE_STEP_CASES)
def test_one_step_matches_the_reference_restatement(engine, mode, D, scalar_ell, fixed, Mf, Mg, ell):
    """One zigp_fit_steps_mode step on 512 sampled rows (with repeats) of make_problem(3000, Mf, D, Mg=Mg), scale N / 512, a different
    learning rate per block: from t0 = 0 with zero moments, and from t0 = 37 with given non-zero m and v.  Mode 2: factors from
    make_lq(negative=2) -- negative diagonal entries are legal.  Fixed blocks must be bit-untouched."""
    from zigp.optim import DENSE_FIT_KEYS
    X, Y, p0 = make_problem(3000, Mf, D, Mg=Mg, ell=ell)
    p = W.problem(p0, mode, negative=2)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    lr = {k: 0.003 * (1 + i) for i, k in enumerate(DENSE_FIT_KEYS)}
    pset = W.make_pset(p, mode, scalar_ell=scalar_ell, fixed=fixed, lr=lr)
    x0, sizes, lrs, positive, trainable = W.flat_state(pset)
    ell_size = (sizes[6], sizes[7])
    shape = dict(Mf=Mf, Mg=Mg, D=D)
    assert sizes == W.block_sizes(mode, shape, ell_size)
    if mode == W.WHITE_FULL:
        assert sum(np.diag(p[k]).min() < 0 for k in W.S_KEYS) == 2
    rows = np.random.RandomState(4).randint(3000, size=512)
    assert len(np.unique(rows)) < 512
    scale = 3000.0 / 512.0
    rs = np.random.RandomState(8)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    eg = W.ref_elbo_grad(mode)
    for t0, m0, v0 in ((0, np.zeros_like(x0), np.zeros_like(x0)), (37, 0.3 * rs.randn(x0.size), 0.2 * rs.rand(x0.size) + 1e-3)):
        xr, mr, vr = x0.copy(), m0.copy(), v0.copy()
        ed_r, kl_r = W.ref_fit_steps(mode, eg, X, Y, shape, xr, mr, vr, lrs, positive, trainable, ell_size, t0, 1, rows=rows, batch=512,
                                     jitter=1e-6, scale=scale)
        x, m, v = x0.copy(), m0.copy(), v0.copy()
        ed, kl = engine.fit_steps_mode(mode, shape, x, m, v, lrs, positive, trainable, ell_size, t0, 1, rows=rows, batch=512, jitter=1e-6,
                                       scale=scale)
        assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == 1
        print('mode %d t0 %d: elbo_data %.10e (ref %.10e) kl %.10e (ref %.10e)' % (mode, t0, ed[0], ed_r[0], kl[0], kl_r[0]))
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


def test_mode_diag_is_fit_steps_bit_for_bit(engine):
    """ZIGP_FIT_DIAG against zigp_fit_steps over 5 steps of 512 rows on make_problem(3000, 96, 3, Mg=70), the context's whiten flag off:
    x, m, v and the history are bit-identical."""
    from zigp import _lib
    X, Y, p = make_problem(3000, 96, 3, Mg=70)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    engine.set_whiten(False)
    engine.set_q_full(False)
    pset = R.make_pset(p)
    x0, sizes, lrs, positive, trainable = W.flat_state(pset)
    shape = dict(Mf=96, Mg=70, D=3)
    rows = np.random.RandomState(6).randint(3000, size=(5, 512))
    out = []
    for call in (lambda *a, **k: engine.fit_steps(*a, **k), lambda *a, **k: engine.fit_steps_mode(_lib.FIT_DIAG, *a, **k)):
        x, m, v = x0.copy(), np.zeros_like(x0), np.zeros_like(x0)
        ed, kl = call(shape, x, m, v, lrs, positive, trainable, (3, 3), 0, 5, rows=rows, batch=512, jitter=1e-6, scale=3000 / 512.0)
        assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == 5
        out.append((x, m, v, ed, kl))
    assert np.max(np.abs(out[0][0] - x0)) > 1e-3
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def _three_runs(engine, mode, mk, rows, jitter, scale, calls, n_steps=None):
    """clean host run, nudged host run, device run in `calls` calls; returns (d_par, d_hist, e_par, e_hist, device pset)"""
    from zigp.optim import WhiteDeviceFit
    a, b, dv = mk(), mk(), mk()
    host = W.ModeEngine(engine, mode)
    ha = R.host_loop(host, a, rows, jitter, scale, n_steps=n_steps)
    hb = R.host_loop(host, b, rows, jitter, scale, n_steps=n_steps, nudge_seed=1)
    fit = WhiteDeviceFit(engine, dv)
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


@pytest.mark.parametrize('mode', MODES)
def test_200_steps_in_three_calls_match_the_host_loop(engine, mode):
    """200 minibatch steps (512 rows each) in calls of 80 + 80 + 40 against the host loop on the same row samples, on
    make_problem(3000, 96, 3, seed=17, Mg=70, ell=0.12) (mode 2: factors from make_lq(seed=3)).
    Not run on an MI355X yet: no measured figures (d of the two host runs, the device loop's distance) exist for this test; on the CPU
    references the two host runs end d_par = 1.8e-13 / 2.2e-13 apart after 25 steps (test_cpu_white_fit.py).
    The test prints its figures."""
    X, Y, p0 = dense_problem()
    p = W.problem(p0, mode, lq_seed=3)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    rows = np.random.RandomState(11).randint(X.shape[0], size=(200, 512))
    scale = X.shape[0] / 512.0
    d_par, d_hist, e_par, e_hist, dv = _three_runs(engine, mode, lambda: W.make_pset(p, mode), rows, 1e-6, scale, (80, 80, 40))
    moved = max(np.max(np.abs(dv.params[k].value - p[k])) for k in ('u_fm', 'u_gm'))
    print('mode %d, 200 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e) | '
          'largest move of a u: %.3f' % (mode, d_par, d_hist, e_par, _bound(d_par), e_hist, _bound(d_hist), moved))
    assert 8 * max(d_par, d_hist) <= 1e-9, 'the problem is too ill-conditioned for this comparison to show anything'
    assert moved > 1e-2
    assert e_par <= _bound(d_par) and e_hist <= _bound(d_hist)
    if mode == W.WHITE_FULL:
        for k in W.S_KEYS:
            assert not np.triu(dv.params[k].value, 1).any()


@pytest.mark.parametrize('mode', MODES)
def test_full_batch_adam_over_the_selected_rows_in_several_chunks(engine, mode):
    """rows = NULL: 10 full-batch steps over 40 000 active rows (a zigp_select_rows selection of a 45 000-row resident set) at M = 256 with
    zigp_set_chunk(16384): three chunks per step.  Same comparison, same bound; the selection is honoured and left as found.
    Not run on an MI355X yet."""
    X, Y, p0 = make_problem(45000, 256, 3, seed=23, ell=0.085)
    p = W.problem(p0, mode, lq_seed=5)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    sel = np.random.RandomState(2).permutation(45000)[:40000]
    engine.select_rows(sel)
    assert engine.N == 40000
    d_par, d_hist, e_par, e_hist, dv = _three_runs(engine, mode, lambda: W.make_pset(p, mode, lr=0.005), None, 1e-6, 1.0, (10,), n_steps=10)
    print('mode %d, full batch, 10 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e '
          '(bound %.3e)' % (mode, d_par, d_hist, e_par, _bound(d_par), e_hist, _bound(d_hist)))
    assert e_par <= _bound(d_par) and e_hist <= _bound(d_hist)
    assert engine.N == 40000
    engine.select_rows(None)
    engine.set_chunk(16384)


@pytest.mark.parametrize('mode', MODES)
def test_cholesky_failure_in_step_0_leaves_the_state_alone(engine, mode):
    """Two coincident inducing points of g, jitter 0: ZIGP_ENOTPD with the step, the latent and the pivot, the state bit-unchanged,
    zigp_fit_steps_applied = 0, an empty history.  (An error-code path through the Cholesky status word; the step enqueued behind the
    failed one runs and its update is skipped.)"""
    import zigp
    X, Y, p0 = make_problem(2000, 40, 2, seed=5, Mg=30, ell=0.3)
    p0['Zg'][7] = p0['Zg'][3]
    p = W.problem(p0, mode)
    engine.set_chunk(16384)
    engine.set_data(X, Y)
    pset = W.make_pset(p, mode)
    x0, sizes, lrs, positive, trainable = W.flat_state(pset)
    x, m, v = x0.copy(), np.full_like(x0, 0.25), np.full_like(x0, 0.5)
    rows = np.random.RandomState(1).randint(2000, size=(2, 256))
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        engine.fit_steps_mode(mode, dict(Mf=40, Mg=30, D=2), x, m, v, lrs, positive, trainable, (2, 2), 5, 2, rows=rows, batch=256, jitter=0.0,
                              scale=2000 / 256.0)
    print(str(ei.value))
    assert 'step 0' in str(ei.value) and 'latent g' in str(ei.value) and 'pivot' in str(ei.value)
    assert int(engine.lib.zigp_last_info(engine.ctx)) > 0
    assert ei.value.steps_applied == 0 and len(ei.value.elbo_data) == 0 and len(ei.value.kl) == 0
    assert int(engine.lib.zigp_fit_steps_applied(engine.ctx)) == 0
    assert np.array_equal(x, x0) and np.all(m == 0.25) and np.all(v == 0.5)
    # the context is usable afterwards
    p['Zg'][7] += 0.05
    assert np.isfinite(engine.elbo(p, jitter=1e-6, need_grad=False)[0])


def test_fit_steps_mode_argument_checks(engine):
    X, Y, p0 = make_problem(1500, 20, 2, seed=2, Mg=12)
    engine.set_data(X, Y)
    shape = dict(Mf=20, Mg=12, D=2)
    rows = np.zeros((1, 64), dtype=np.int64)
    st = {}
    for mode in MODES:
        pset = W.make_pset(W.problem(p0, mode), mode)
        st[mode] = W.flat_state(pset)

    def call(mode, layout=None, **kw):
        x, sizes, lrs, positive, trainable = st[mode if layout is None else layout]
        x = kw.pop('x', x.copy())
        return engine.fit_steps_mode(mode, shape, x, np.zeros_like(x), np.zeros_like(x), lrs, kw.pop('positive', positive), trainable, (2, 2), 0, 1,
                                     rows=rows, batch=64, jitter=1e-6), x

    for mode in MODES:
        out, x = call(mode)
        assert np.all(np.isfinite(out)) and not np.array_equal(x, st[mode][0])
    for bad in (3, -1, 17):
        with pytest.raises(ValueError, match='unknown mode'):
            call(bad, layout=W.WHITE)
    # positive on a full block
    pos = list(st[W.WHITE_FULL][3])
    pos[5] = True
    with pytest.raises(ValueError, match='positive'):
        call(W.WHITE_FULL, positive=pos)
    # the diagonal model's n_free for mode 2, and the other way round
    with pytest.raises(ValueError, match='n_free'):
        call(W.WHITE_FULL, layout=W.WHITE)
    with pytest.raises(ValueError, match='n_free'):
        call(W.WHITE, layout=W.WHITE_FULL)
    # a zero diagonal entry of Lq_g (row 4: entry 4 * 5 / 2 + 4 of block 5): refused, the state untouched
    sizes = st[W.WHITE_FULL][1]
    o = np.concatenate([[0], np.cumsum(sizes)])
    xz = st[W.WHITE_FULL][0].copy()
    xz[o[5] + 4 * 5 // 2 + 4] = 0.0
    keep = xz.copy()
    with pytest.raises(ValueError, match='zero diagonal'):
        call(W.WHITE_FULL, x=xz)
    assert np.array_equal(xz, keep)
    # a zero BELOW the diagonal is fine
    xz = st[W.WHITE_FULL][0].copy()
    xz[o[5] + 4 * 5 // 2 + 3] = 0.0
    call(W.WHITE_FULL, x=xz)
    # what zigp_fit_steps refuses stays refused: a mean function on the context
    engine.elbo(dict(p0, mean_b=0.5), jitter=1e-6, need_grad=False)
    with pytest.raises(ValueError, match='mean function'):
        call(W.WHITE)
    engine.elbo(p0, jitter=1e-6, need_grad=False)
    call(W.WHITE)


def test_the_call_leaves_the_context_alone(engine):
    """With set_whiten(False) a mode-2 fit call followed by an unwhitened engine.elbo gives the numbers it gave before the call, bit for
    bit, and zigp_get_whiten / zigp_get_q_full are unchanged; with both flags on, no mode is refused and the flags stay on."""
    from zigp import _lib
    X, Y, p0 = make_problem(5000, 150, 3, seed=9, Mg=100, ell=0.2)
    engine.set_chunk(2048)
    engine.set_data(X, Y)
    engine.set_whiten(False)
    engine.set_q_full(False)
    e0 = engine.elbo(p0, jitter=1e-6)
    pr0 = engine.predict(p0, X[:700], jitter=1e-6)
    shape = dict(Mf=150, Mg=100, D=3)
    rows = np.random.RandomState(4).randint(5000, size=(3, 1500))
    state = {}
    for mode in MODES:
        pset = W.make_pset(W.problem(p0, mode, negative=1), mode)
        state[mode] = W.flat_state(pset)
        x, sizes, lrs, positive, trainable = state[mode]
        x = x.copy()
        engine.fit_steps_mode(mode, shape, x, np.zeros_like(x), np.zeros_like(x), lrs, positive, trainable, (3, 3), 0, 3, rows=rows, batch=1500,
                              jitter=1e-6, scale=5000 / 1500.0)
        assert engine.get_whiten() is False and engine.get_q_full() is False
        assert int(engine.lib.zigp_get_whiten(engine.ctx)) == 0 and int(engine.lib.zigp_get_q_full(engine.ctx)) == 0
        e1 = engine.elbo(p0, jitter=1e-6)
        pr1 = engine.predict(p0, X[:700], jitter=1e-6)
        assert e0[0] == e1[0] and e0[1] == e1[1] and all(np.array_equal(e0[2][k], e1[2][k]) for k in e0[2])
        assert np.array_equal(pr0, pr1)
    # the flags are not read either: with both on, every mode runs and gives what it gave with both off
    xd, sizes, lrs, positive, trainable = W.flat_state(R.make_pset(p0))
    ref = {}
    for flags_on in (False, True):
        engine.set_whiten(flags_on)
        engine.set_q_full(flags_on)
        for mode, (x0, lr_, pos_, tr_) in ((_lib.FIT_DIAG, (xd, lrs, positive, trainable)),
                                           (W.WHITE_FULL, (state[W.WHITE_FULL][0],) + tuple(state[W.WHITE_FULL][2:]))):
            x, m, v = x0.copy(), np.zeros_like(x0), np.zeros_like(x0)
            ed, kl = engine.fit_steps_mode(mode, shape, x, m, v, lr_, pos_, tr_, (3, 3), 0, 2, rows=rows[:2], batch=1500, jitter=1e-6,
                                           scale=5000 / 1500.0)
            assert engine.get_whiten() is flags_on and engine.get_q_full() is flags_on
            if flags_on:
                assert all(np.array_equal(a, b) for a, b in zip(ref[mode], (x, m, v, ed, kl)))
            else:
                ref[mode] = (x, m, v, ed, kl)
    engine.set_whiten(False)
    engine.set_q_full(False)
    engine.set_chunk(16384)


def _toy(q_diag, minibatch_size=100, seed=1, mean_function=None):
    import os
    import scipy.io as sio
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    mat = sio.loadmat(os.path.join(os.path.dirname(__file__), 'golden', 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    Z = np.linspace(1, 9, 9)[:, None]
    np.random.seed(seed)
    m = OnOffSVGP(X, Y, onoffgpf.kernels.RBF(1, lengthscales=1.), onoffgpf.kernels.RBF(1, lengthscales=1., variance=5.),
                  OnOffLikelihood(), Z, Z.copy(), minibatch_size=minibatch_size, whiten=True, q_diag=q_diag, mean_function=mean_function)
    m.likelihood.variance = 0.01
    return m


@pytest.mark.parametrize('q_diag', [True, False])
def test_model_adam_with_device_loop_runs_on_the_device_and_matches_the_host_loop(q_diag):
    """OnOffSVGP(whiten=True[, q_diag=False], minibatch_size=100).optimize(method='adam', maxiter=60, device_loop=True): one fit_steps_mode
    call of 60 steps, no elbo call, the row samples the host loop draws from _rng, and the end state within max(8 d, 1e-13) of a twin run
    with device_loop=False, d from a second host run on the same samples nudged by +-1 ulp per step.  Without device_loop (today's rule)
    and with device_loop=False no device loop is called.
    Not run on an MI355X yet."""
    from zigp import _lib
    from zigp.optim import DENSE_FIT_KEYS
    mode = W.WHITE if q_diag else W.WHITE_FULL
    dev, twin, third, plain = _toy(q_diag), _toy(q_diag), _toy(q_diag), _toy(q_diag)
    calls, elbos = [], []
    eng = dev._engine
    fsm, elbo, fs = eng.fit_steps_mode, eng.elbo, eng.fit_steps
    eng.fit_steps_mode = lambda *a, **k: (calls.append((a[0], a[10], np.array(k['rows']).reshape(a[10], -1))), fsm(*a, **k))[1]
    eng.fit_steps = lambda *a, **k: (calls.append(('fit_steps',)), fs(*a, **k))[1]
    eng.elbo = lambda *a, **k: (elbos.append(1), elbo(*a, **k))[1]
    u0 = {k: dev._pset().params[k].value.copy() for k in ('u_fm', 'u_gm')}
    dev.optimize(method='adam', maxiter=60, learning_rate=0.01, device_loop=True)
    assert [(c[0], c[1]) for c in calls] == [(mode, 60)] and not elbos
    assert mode == (_lib.FIT_WHITE if q_diag else _lib.FIT_WHITE_FULL)
    rows_dev = calls[0][2]
    # the twin: device_loop=False keeps it on the host loop
    for model, kw in ((twin, dict(device_loop=False)), (plain, {})):
        seen, tcalls = [], []
        teng = model._engine
        sel, tfm, tfs = teng.select_rows, teng.fit_steps_mode, teng.fit_steps
        teng.select_rows = lambda idx=None, seen=seen, sel=sel: (seen.append(None if idx is None else np.array(idx)), sel(idx))[1]
        teng.fit_steps_mode = lambda *a, tcalls=tcalls, tfm=tfm, **k: (tcalls.append(1), tfm(*a, **k))[1]
        teng.fit_steps = lambda *a, tcalls=tcalls, tfs=tfs, **k: (tcalls.append(1), tfs(*a, **k))[1]
        model.optimize(method='adam', maxiter=60 if kw else 3, learning_rate=0.01, **kw)
        assert not tcalls and len(seen) == (60 if kw else 3)
        if kw:
            assert np.array_equal(rows_dev, np.stack(seen))
    # d: the same loop on the same samples, nudged
    ps3 = third._pset()
    for q in ps3.params.values():
        q.learning_rate = 0.01
    third._make_resident()
    R.host_loop(W.ModeEngine(third._engine, mode), ps3, rows_dev, 1e-6, 450.0 / 100.0, nudge_seed=1)
    d = R.block_distance(ps3, twin._pset())
    e = R.block_distance(dev._pset(), twin._pset())
    moved = max(np.max(np.abs(dev._pset().params[k].value - u0[k])) for k in ('u_fm', 'u_gm'))
    print('model q_diag=%s, 60 steps: two host runs d %.3e | device - host %.3e (bound %.3e) | moved %.3e' % (q_diag, d, e, _bound(d), moved))
    assert e <= _bound(d)
    assert set(dev._pset().params) == set(DENSE_FIT_KEYS)
    if not q_diag:
        for k in W.S_KEYS:
            val = dev._pset().params[k].value
            assert val.shape == (9, 9, 1) and not np.triu(val[:, :, 0], 1).any() and np.tril(val[:, :, 0], -1).any()
    assert np.isfinite(dev.compute_log_likelihood())


def test_model_device_loop_refuses_a_callback_and_a_mean_function():
    import onoffgpf
    m = _toy(True)
    with pytest.raises(ValueError, match='callback'):
        m.optimize(method='adam', maxiter=2, device_loop=True, callback=lambda it, e: None)
    m = _toy(False, mean_function=onoffgpf.mean_functions.Constant())
    with pytest.raises(ValueError, match='mean function'):
        m.optimize(method='adam', maxiter=2, device_loop=True)
    # the unwhitened diagonal model takes the same switch
    import test_gpu_dense_fit as T
    u = T._toy(100)
    with pytest.raises(ValueError, match='callback'):
        u.optimize(method='adam', maxiter=2, device_loop=True, callback=lambda it, e: None)
    calls = []
    fs = u._engine.fit_steps
    u._engine.fit_steps = lambda *a, **k: (calls.append(a[9]), fs(*a, **k))[1]
    u.optimize(method='adam', maxiter=5, device_loop=True)
    assert calls == [5]
    calls.clear()
    u.optimize(method='adam', maxiter=2, device_loop=False)
    assert not calls
