"""GPU parity of the Kronecker path at every factor dimension (1 to 8 per factor) and kernel variant, against the LITERAL dense oracle
(oracle/zigp_oracle*.py).  tests/test_gpu_kron.py runs 2 + 1 columns only; the cases here (kron_nd.CASES) walk the three forms of the
squared distance in the K tile, the four instantiations of the small-grid kernels, one launch per latent when the block counts differ,
the 15 moment columns of D = 7, the larger-grid kernels, and the GEMM-panel path that D = 8 or a larger grid falls through to (the id
of a case names its route; zigp_kronf.hip kf_plan decides it).  tests/test_cpu_kron_nd.py holds the reference's own floor on every case
at 1e-8 and cond(K_p) at 1e5 (1e3 for the fit loops), which is what makes the tolerances below -- the project's own, unchanged -- valid.
Every test prints its figures (pytest -s)."""
import numpy as np
import pytest

import kron_nd as K
from conftest import relerr

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings(K.READ_ONLY_NOTE)]

PRED_NAMES = ('gfmean', 'gfvar', 'gfmeanu', 'fmean', 'fvar', 'gmean', 'gvar', 'ephi_g', 'evar_phi_g')
KERN_KEYS = ('Zf', 'Zg', 'ell_f', 'ell_g', 'var_f', 'var_g')
VEC_KEYS = ('u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'noise')


def _flat(res):
    """every array of a kron_elbo / kron_head_elbo result (value, KL, gradient blocks) as (label, array)"""
    out = [('value', np.asarray(res[0])), ('kl', np.asarray(res[1]))]
    for k in sorted(res[2]):
        v = res[2][k]
        for q, a in enumerate(v) if isinstance(v, list) else [(None, v)]:
            out.append(((k, q), np.asarray(a, dtype=np.float64)))
    return out


def _bit_identical(a, b):
    fa, fb = _flat(a), _flat(b)
    assert [k for k, _ in fa] == [k for k, _ in fb]
    for (k, x), (_, y) in zip(fa, fb):
        assert np.array_equal(x, y), k


def _check_grads(tag, dims, g, g_r, keys_kern, keys_vec, tol=1e-6):
    """every block to tol of its largest reference entry; the Z and lengthscale blocks also per input dimension (a column's largest
    error over the column's largest reference: block-wide, the largest dimension would hide a wrong small one)"""
    worst = 0.0
    for k in keys_kern:
        for q in range(2):
            a, b = np.asarray(g[k][q], dtype=np.float64).reshape(-1), np.asarray(g_r[k][q], dtype=np.float64).reshape(-1)
            e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
            line = '  %s grad %s[%d] relerr %.2e (max |ref| %.3e)' % (tag, k, q, e, np.max(np.abs(b)))
            ed = []
            if not k.startswith('var'):
                a2, b2 = a.reshape(-1, dims[q]), b.reshape(-1, dims[q])
                ed = list(np.max(np.abs(a2 - b2), 0) / np.maximum(np.max(np.abs(b2), 0), 1e-300))
                line += '  per dimension ' + ' '.join('%.1e' % x for x in ed)
            print(line)
            worst = max([worst, e] + ed)
            assert e < tol, (k, q, e)
            assert all(x < tol for x in ed), (k, q, ed)
    for k in keys_vec:
        a, b = np.asarray(g[k], dtype=np.float64).reshape(-1), np.asarray(g_r[k], dtype=np.float64).reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        print('  %s grad %s relerr %.2e' % (tag, k, e))
        worst = max(worst, e)
        assert e < tol, (k, e)
    return worst


@pytest.mark.parametrize('name', list(K.CASES))
def test_predict_matches_literal_oracle(engine, name):
    X, Y, p = K.problem(name)
    for goff in (0.0, -1.0):
        out = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=goff)
        ref = K.oracle_predict(name, goff)
        errs = [relerr(out[i], ref[i]) for i in range(9)]
        print('%s g_offset %g: %s' % (name, goff, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs))))
        assert max(errs) < 1e-6, (name, goff, errs)


@pytest.mark.parametrize('name', list(K.CASES))
def test_elbo_and_gradient_match_literal_oracle(engine, name):
    X, Y, p = K.problem(name)
    scale = K.case_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    e_r, d_r, kl_r, g_r = K.oracle_grad(name)
    print('%s elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e' % (name, ed - kl, e_r, abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r)))
    assert abs(ed - scale * d_r) <= 1e-7 * abs(scale * d_r)
    assert abs(kl - kl_r) <= 1e-7 * abs(kl_r)
    worst = _check_grads(name, K.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS)
    print('%s worst gradient figure %.2e' % (name, worst))


@pytest.mark.parametrize('name', K.FUSED)
def test_fused_and_panel_paths_agree(engine, name):
    """the fused kernels against the GEMM-panel path on identical inputs, with the bounds of
    test_gpu_kron.py::test_kron_fused_and_panel_paths_agree; a rerun of the fused call returns the same bits"""
    X, Y, p = K.problem(name)
    a = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=3.0)
    a2 = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=3.0)
    pa = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
    pa2 = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
    engine.set_kron_panels(True)
    try:
        b = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=3.0)
        pb = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
    finally:
        engine.set_kron_panels(False)
    _bit_identical(a, a2)
    assert np.array_equal(pa, pa2)
    ev, ek = abs(a[0] - b[0]) / abs(b[0]), abs(a[1] - b[1]) / abs(b[1])
    eg = max([relerr(a[2][k], b[2][k]) for k in VEC_KEYS] + [relerr(a[2][k][q], b[2][k][q]) for k in KERN_KEYS for q in range(2)])
    ep = max(relerr(pa[i], pb[i]) for i in range(9))
    print('%s fused vs panels: value %.1e kl %.1e gradients %.1e predictions %.1e' % (name, ev, ek, eg, ep))
    assert ev <= 1e-8 and ek <= 1e-9
    for k in VEC_KEYS:
        assert relerr(a[2][k], b[2][k]) < 1e-7, k
    for k in KERN_KEYS:
        for q in range(2):
            assert relerr(a[2][k][q], b[2][k][q]) < 1e-7, (k, q)
    for i in range(9):
        assert relerr(pa[i], pb[i]) < 1e-6, i


def test_resident_rows_equal_host_minibatch(engine):
    """kron_elbo(rows=(lo, hi)) of a resident data set with 6, 14, 14 and 16 columns against the same rows passed from the host: the
    same bits in every returned array; a parameter set whose D0 + D1 is not the resident D is refused"""
    for name in ('d42', 'd77', 'L77', 'p88'):
        X, Y, p = K.problem(name)
        N = X.shape[0]
        engine.set_data(X, Y)
        assert engine.D == sum(K.CASES[name]['D'])
        for lo, hi in ((0, N), (5, N - 3)):
            assert (lo, hi) == (0, N) or (lo % 16 and hi % 16)
            a = engine.kron_elbo(p, X[lo:hi], Y[lo:hi], jitter=K.JITTER, scale=2.5)
            b = engine.kron_elbo(p, rows=(lo, hi), jitter=K.JITTER, scale=2.5)
            _bit_identical(a, b)
        print('%s: rows of %d resident columns == host minibatch' % (name, engine.D))
    Xo, Yo, po = K.problem('d42')                      # 6 columns against the 16 resident ones of p88
    with pytest.raises(ValueError, match="differs from the data's D"):
        engine.kron_elbo(po, rows=(0, 100), jitter=K.JITTER)
    _bit_identical(engine.kron_elbo(p, rows=(5, N - 3), jitter=K.JITTER, scale=2.5), b)


@pytest.mark.parametrize('name', ['d77', 'L32'])
def test_shard_additivity_many_tiles(engine, name):
    """5000 rows (313 tiles: several per wave): two uneven halves, the KL counted once, add up to the whole batch -- bounds of
    test_gpu_kron.py::test_kron_shard_additivity_many_tiles"""
    X, Y, p = K.problem(name, N=5000)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=1.0)
    a = engine.kron_elbo(p, X[:2203], Y[:2203], jitter=K.JITTER, scale=1.0, include_kl=True)
    b = engine.kron_elbo(p, X[2203:], Y[2203:], jitter=K.JITTER, scale=1.0, include_kl=False)
    print('%s halves vs whole: value %.1e' % (name, abs((a[0] + b[0]) - ed) / abs(ed)))
    assert abs((a[0] + b[0]) - ed) <= 1e-11 * abs(ed) and a[1] == kl and b[1] == 0.0
    for k in VEC_KEYS:
        s_ = np.asarray(a[2][k]) + np.asarray(b[2][k])
        assert np.max(np.abs(s_ - np.asarray(g[k]))) <= 1e-9 * max(np.max(np.abs(np.asarray(g[k]))), 1e-300), k
    for k in KERN_KEYS:
        for q in range(2):
            s_ = np.asarray(a[2][k][q]) + np.asarray(b[2][k][q])
            ref = np.asarray(g[k][q])
            assert np.max(np.abs(s_ - ref)) <= 1e-8 * max(np.max(np.abs(ref)), 1e-300), (k, q)


def _head_data(name, lik):
    X, Y, p = K.problem(name)
    return X, ((Y > 0) * 1.0 if lik == 'bernoulli' else Y), K.head_params(p)      # classifier.py:43-44


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('name', ['d31', 'd71', 'L32', 'p81'])
def test_head_predict_and_elbo_match_literal_oracle(engine, name, lik):
    """the single-latent heads, tolerances of tests/test_gpu_heads.py"""
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    X, Y, p = _head_data(name, lik)
    f_mu = 0.0 if lik == 'gaussian' else 0.2
    out = engine.kron_head_predict(p, X, lik, jitter=K.JITTER, f_mu=f_mu)
    ref = o.kron_head_predict(X, p, lik, K.JITTER, f_mu)
    if lik == 'gaussian':
        pairs = (('fmean', out[0], ref[0]), ('fvar', out[1], ref[1]), ('ymean', out[2], ref[0]), ('yvar', out[3], ref[1] + p['noise']))
    else:
        pairs = (('pfmean', out[2], ref[0]), ('pfvar', out[3], ref[1]), ('fmean', out[0], ref[2]), ('fvar', out[1], ref[3]))
    for nm, a, b in pairs:
        e = relerr(a, np.asarray(b).reshape(-1))
        print('%s %s predict %s relerr %.2e' % (name, lik, nm, e))
        assert e < 1e-6, (nm, e)
    scale = K.case_scale(name)
    ed, kl, g = engine.kron_head_elbo(p, X, Y, lik, jitter=K.JITTER, scale=scale, f_mu=f_mu)
    e_r, d_r, kl_r, g_r = ot.kron_head_elbo_and_grad(X, Y, p, lik, K.JITTER, scale=scale, f_mu=f_mu)
    print('%s %s elbo %.10e ref %.10e  kl %.8e ref %.8e' % (name, lik, ed - kl, e_r, kl, kl_r))
    assert abs(ed - scale * d_r) <= 1e-7 * abs(scale * d_r)
    assert abs(kl - kl_r) <= 1e-7 * abs(kl_r)
    _check_grads('%s %s' % (name, lik), K.CASES[name]['D'], g, g_r, ('Zf', 'ell_f', 'var_f'),
                 ('u_fm', 'u_fs_sqrt', 'f_mu') + (('noise',) if lik == 'gaussian' else ()))
    if lik == 'bernoulli':
        assert g['noise'] == 0.0


def _nd_pset(name):
    """the ParamSet of onofftf.model.init_params carrying a fit fixture's inducing inputs and lengthscales (its variances 2.0 / 1.5,
    noise 0.05 as test_device_fit_loop_equals_host_adam_loop sets them)"""
    from onofftf.model import init_params
    X, Y, p = K.fit_problem(name)
    grid = K.FIT_CASES[name]['f']
    ps = init_params(X, grid, grid, kmeans_seed=3, rng=np.random.RandomState(9))
    for tag in ('f', 'g'):
        for q in range(2):
            ps.params['%s_ind/z_%d' % (tag, q)].value = p['Z' + tag][q].copy()
            ps.params['%s_kern/lengthscale_%d' % (tag, q)].value = p['ell_' + tag][q].copy()
        ps.params['%s_kern/variance_0' % tag].value = np.array([2.0])
        ps.params['%s_kern/variance_1' % tag].value = np.array([1.5])
    ps.params['likelihood/variance'].value = np.array(0.05)
    return ps


@pytest.mark.parametrize('name', list(K.FIT_CASES))
def test_device_fit_loop_equals_host_adam_loop_nd(engine, name):
    """zigp_kron_fit_steps at (3,1), (7,1) on a 6 x 5 grid and (3,2) on 10 x 50: 30 steps in two calls, one wrap-around host batch,
    against the same iterations stepped from the host with AdamGroups -- protocol and tolerances of
    test_gpu_onofftf.py::test_device_fit_loop_equals_host_adam_loop (1e-12 of each block's magnitude, 1e-10 on the ELBO history)."""
    from onofftf.model import KronDeviceFit, FIT_BLOCK_NAMES
    from test_gpu_onofftf import _host_steps
    X, Y, _ = K.fit_problem(name)
    X, Y = np.array(X), np.array(Y)
    N, batch, n_steps = X.shape[0], 500, 30
    psets = [_nd_pset(name), _nd_pset(name)]
    assert psets[0].params['f_ind/z_0'].value.shape[1] == K.FIT_CASES[name]['D'][0]
    rs = np.random.RandomState(2)
    rows_seq = [int(r) for r in rs.randint(0, N - batch, size=n_steps)]
    rows_seq[n_steps // 2] = -1
    wi = rs.permutation(N)[:batch]
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    jitter, scale = K.JITTER, N / batch
    h_host = _host_steps(engine, psets[0], rows_seq, batch, jitter, scale, X, Y, wraps)
    engine.set_data(X, Y)
    fit = KronDeviceFit(engine, psets[1])
    assert (fit.shape['D0'], fit.shape['D1']) == K.FIT_CASES[name]['D']
    ed, kl = [], []
    for a, b in ((0, 12), (12, n_steps)):
        seq = rows_seq[a:b]
        e_, k_ = fit.steps(seq, batch, jitter, scale, *(wraps if -1 in seq else (None, None)))
        ed += list(e_); kl += list(k_)
    assert fit.t == n_steps
    h_dev = np.stack([ed, kl], 1)
    eh = np.max(np.abs(h_dev - h_host) / np.abs(h_host))
    worst = max(float(np.max(np.abs(psets[1].params[k].value - psets[0].params[k].value)) / np.max(np.abs(psets[0].params[k].value)))
                for k in FIT_BLOCK_NAMES)
    u0 = _nd_pset(name)
    moved = max(float(np.max(np.abs(psets[0].params[k].value - u0.params[k].value))) for k in ('f_ind/value', 'g_ind/value'))
    print('fit %s D %s grid %s: %d device steps vs host AdamGroups: worst parameter block %.2e, ELBO history %.2e (u moved by up to %.3f)'
          % (name, K.FIT_CASES[name]['D'], K.FIT_CASES[name]['f'], n_steps, worst, eh, moved))
    assert worst <= 1e-12 and eh <= 1e-10 and moved > 1e-2, (worst, eh, moved)


def _nd_head_problem(name, lik):
    """head_fit_ref.head_problem at a fit fixture's column split: (X, Y, make_pset)"""
    from onofftf.heads import init_head_params
    X, Y, p = K.fit_problem(name)
    X, Y = np.array(X), np.array((Y > 0) * 1.0 if lik == 'bernoulli' else Y)
    grid = K.FIT_CASES[name]['f']

    def make_pset():
        ps = init_head_params(X, grid, lik, include_f_mu=(lik == 'bernoulli'), kmeans_seed=3, rng=np.random.RandomState(9))
        for q in range(2):
            ps.params['f_ind/z_%d' % q].value = p['Zf'][q].copy()
            ps.params['f_kern/lengthscale_%d' % q].value = p['ell_f'][q].copy()
        ps.params['f_kern/variance_0'].value = np.array([2.0])
        ps.params['f_kern/variance_1'].value = np.array([1.5])
        if lik == 'gaussian':
            ps.params['likelihood/variance'].value = np.array(0.05)
        return ps

    return X, Y, make_pset


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('name', K.HEAD_FIT_CASES)
def test_head_fit_one_step_and_20_steps_nd(engine, name, lik):
    """zigp_kron_head_fit_steps at (3,1) and (7,1): one step against the reference restatement (tests/head_fit_ref.py: the CPU oracle,
    Log1pe chain, NumPy Adam) and 20 steps in two calls against the host loop, with the bounds of tests/test_gpu_head_fit.py: m, x to
    1e-6, v to 2e-6, the history entry to 1e-7; 20 steps within max(8 d, 1e-13), d from the +-1-ulp-nudged host run, 8 d <= 1e-7."""
    import head_fit_ref as R
    from onofftf.heads import HEAD_FIT_BLOCK_NAMES, HeadDeviceFit
    X, Y, mk = _nd_head_problem(name, lik)
    assert X.shape[0] == R.N_ROWS
    engine.set_data(X, Y)
    pset = mk()
    for i, k in enumerate(HEAD_FIT_BLOCK_NAMES):
        if k in pset.params:
            pset.params[k].learning_rate = 0.003 * (1 + i)
    x0, lr, positive, trainable, shape = R.flat_state(pset)
    assert (shape['D0'], shape['D1']) == K.FIT_CASES[name]['D']
    offs = np.concatenate([[0], np.cumsum(R.block_sizes(shape))])
    rs = np.random.RandomState(8)
    t0, m0, v0 = 37, 0.3 * rs.randn(x0.size), 0.2 * rs.rand(x0.size) + 1e-3
    xr, mr, vr = x0.copy(), m0.copy(), v0.copy()
    ed_r, kl_r = R.ref_head_fit_steps(R.oracle_eg(lik), X, Y, shape, xr, mr, vr, lr, positive, trainable, t0, [700], R.BATCH, jitter=R.JITTER, scale=R.SCALE)
    x, m, v = x0.copy(), m0.copy(), v0.copy()
    ed, kl = engine.kron_head_fit_steps(shape, lik, x, m, v, lr, positive, trainable, t0, [700], R.BATCH, jitter=R.JITTER, scale=R.SCALE)
    print('%s %s t0 %d: elbo_data %.10e (ref %.10e) kl %.10e (ref %.10e)' % (name, lik, t0, ed[0], ed_r[0], kl[0], kl_r[0]))
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
    # 20 steps in calls of 8 + 12, one host wrap-around batch, against the host loop
    seq, wi = R.rows_with_a_wrap(20)
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    a, b, dv = mk(), mk(), mk()
    ha = R.host_loop(engine, a, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps)
    hb = R.host_loop(engine, b, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps, nudge_seed=1)
    engine.set_data(X, Y)
    fit = HeadDeviceFit(engine, dv, lik)
    hist = []
    for lo, hi in ((0, 8), (8, 20)):
        part = seq[lo:hi]
        e_, k_ = fit.steps(part, R.BATCH, R.JITTER, R.SCALE, *(wraps if -1 in part else (None, None)))
        hist.append(np.stack([e_, k_], 1))
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    e_par, e_hist = R.block_distance(dv, a), R.hist_distance(np.concatenate(hist), ha)
    print('%s %s, 20 steps: two host runs d_par %.3e d_hist %.3e | device - host: parameters %.3e (bound %.3e) history %.3e (bound %.3e)'
          % (name, lik, d_par, d_hist, e_par, R.bound(d_par), e_hist, R.bound(d_hist)))
    assert 8 * max(d_par, d_hist) <= 1e-7 and fit.t == 20
    assert e_par <= R.bound(d_par) and e_hist <= R.bound(d_hist)


def test_shifted_inputs(engine):
    """case d21-mix with kron_nd.SHIFT added to every column of X and Z (the moment sums of the kernel cotangent are centred on the
    mid-range of Z_p, KH_ZC: this is the input for which that matters).  The shift is the one at which the oracle's own error is
    <= 1e-9 (test_cpu_kron_nd.py::test_oracle_at_shifted_inputs); prediction and gradient to 1e-6."""
    name = K.SHIFT_CASE
    X, Y, p = K.problem(name, shift=K.SHIFT)
    for goff in (0.0, -1.0):
        out = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=goff)
        ref = K.oracle_predict(name, goff, shift=K.SHIFT)
        errs = [relerr(out[i], ref[i]) for i in range(9)]
        print('%s shift %g g_offset %g: %s' % (name, K.SHIFT, goff, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs))))
        assert max(errs) < 1e-6, errs
    scale = K.case_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    e_r, d_r, kl_r, g_r = K.oracle_grad(name, shift=K.SHIFT)
    assert abs(ed - scale * d_r) <= 1e-7 * abs(scale * d_r) and abs(kl - kl_r) <= 1e-7 * abs(kl_r)
    _check_grads('%s shift %g' % (name, K.SHIFT), K.CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS)


def test_argument_edges(engine):
    """a factor with 9 columns is refused by name and runs nothing; f and g with different column splits are refused; after each
    refusal a good call returns the earlier numbers"""
    X, Y, p = K.problem('d21-12')
    good = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0)
    pred = engine.kron_predict(p, X, jitter=K.JITTER)
    for D0, D1 in ((9, 1), (1, 9)):
        Xb, Yb, pb = K.make_kron_problem_nd(100, 6, 5, D0, D1, seed=1)
        for call in (lambda: engine.kron_elbo(pb, Xb, Yb, jitter=K.JITTER), lambda: engine.kron_predict(pb, Xb, jitter=K.JITTER),
                     lambda: engine.kron_head_elbo(K.head_params(pb), Xb, Yb, 'gaussian', jitter=K.JITTER)):
            with pytest.raises(ValueError, match=r'factor dimensions must be in \[1, 8\]'):
                call()
            _bit_identical(engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0), good)
    _, _, p31 = K.make_kron_problem_nd(100, 10, 20, 1, 2, seed=2)      # the same 3 columns split 1 + 2 for g
    mixed = dict(p, Zg=p31['Zg'], ell_g=p31['ell_g'])
    with pytest.raises(ValueError, match='same input columns'):
        engine.kron_elbo(mixed, X, Y, jitter=K.JITTER)
    with pytest.raises(ValueError, match='same input columns'):
        engine.kron_predict(mixed, X, jitter=K.JITTER)
    _bit_identical(engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0), good)
    assert np.array_equal(engine.kron_predict(p, X, jitter=K.JITTER), pred)
