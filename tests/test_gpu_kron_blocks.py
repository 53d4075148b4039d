"""GPU parity of the Kronecker GEMM-panel path (csrc/zigp_kron.hip kron_run_panels) at inducing grids beyond ONE 128-row block per factor.

The operands of that path are padded to 128, so every other Kronecker fixture of this suite (largest factor: 128 points) has
Mq0 = Mq1 = 128 and one block each: the multi-block tile lists, the split-K reduction with S != nk and planes larger than one tile, the
blocked factorisation at Mq = 256 / 384 with identity padding, and every stride or offset that differs only when Mq0 != Mq1 run nowhere
else.  kron_nd.BLOCK_CASES walks the block counts 2 x 1, 1 x 2, both in one step, 3 x 1 (with N > 1024), the 128 / 129 boundary and
2 x 2; tests/test_cpu_kron_blocks.py pins what the reference alone does on each (floor <= 1e-8, cond <= 1e5), and, for the 2 x 2 grid whose
literal form is too large, the factored restatement tests/kronp_ref.py to the literal oracle at 1e-8.

* end to end: the nine predictive rows, the data term, the KL and every gradient block and input dimension against the oracle at the
  path's tolerance (1e-6), on/off model on all cases, both heads on b21 / b12, one run with Matern factors;
* identities that hold bit for bit: value-only call == gradient call (the KL reads the Cholesky factors the backward pass later
  overwrites), rows= == host rows, a rerun on the same context, every call == the same call on a FRESH context after grids of other
  padded sizes went through the same buffers;
* include_kl=False against the reference without the KL; an empty row range; N = 1; two shards against one call.
Every test prints its figures (pytest -s); they are recorded in profiles/kron_panel_stage_parity.log."""
import numpy as np
import pytest

import kron_nd as K
from conftest import relerr
from test_gpu_kron_nd import PRED_NAMES, KERN_KEYS, VEC_KEYS, _flat, _bit_identical, _check_grads

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings(K.READ_ONLY_NOTE)]

TOL = 1e-6
HEAD_KERN, HEAD_VEC = ('Zf', 'ell_f', 'var_f'), ('u_fm', 'u_fs_sqrt', 'f_mu')


@pytest.mark.parametrize('name', list(K.BLOCK_CASES))
def test_predict_matches_oracle(engine, name):
    X, Y, p = K.block_problem(name)
    for goff in (0.0, -1.0):
        out = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=goff)
        ref = K.block_oracle_predict(name, goff)
        errs = [relerr(out[i], ref[i]) for i in range(9)]
        print('%s blocks %s g_offset %g: %s' % (name, K.block_counts(name), goff, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs))))
        assert max(errs) < TOL, (name, goff, errs)


@pytest.mark.parametrize('name', list(K.BLOCK_CASES))
def test_elbo_and_gradient_match_oracle(engine, name):
    """data term, KL, every gradient block and input dimension; the value-only call returns the gradient call's value and KL bit for bit"""
    X, Y, p = K.block_problem(name)
    scale = K.block_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    e_r, d_r, kl_r, g_r = K.block_oracle_grad(name)
    ev, ek = abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r)
    print('%s blocks %s elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e' % (name, K.block_counts(name), ed - kl, e_r, ev, ek))
    worst = _check_grads(name, K.BLOCK_CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
    print('%s worst gradient figure %.2e' % (name, worst))
    assert ev <= TOL and ek <= TOL, (ev, ek)
    v = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale, need_grad=False)
    assert v[2] is None and v[0] == ed and v[1] == kl, (v[:2], ed, kl)
    _bit_identical(engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale), (ed, kl, g))


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
@pytest.mark.parametrize('name', ['b21', 'b12'])
def test_heads_match_literal_oracle(engine, name, lik):
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    X, Y, p = K.block_problem(name)
    Y, p = ((Y > 0) * 1.0 if lik == 'bernoulli' else Y), K.head_params(p)
    f_mu = 0.0 if lik == 'gaussian' else 0.2
    out = engine.kron_head_predict(p, X, lik, jitter=K.JITTER, f_mu=f_mu)
    ref = o.kron_head_predict(X, p, lik, K.JITTER, f_mu)
    if lik == 'gaussian':
        pairs = (('fmean', out[0], ref[0]), ('fvar', out[1], ref[1]), ('ymean', out[2], ref[0]), ('yvar', out[3], ref[1] + p['noise']))
    else:
        pairs = (('pfmean', out[2], ref[0]), ('pfvar', out[3], ref[1]), ('fmean', out[0], ref[2]), ('fvar', out[1], ref[3]))
    errs = [(nm, relerr(a, np.asarray(b).reshape(-1))) for nm, a, b in pairs]
    print('%s %s predict: %s' % (name, lik, ' '.join('%s %.1e' % e for e in errs)))
    assert max(e for _, e in errs) < TOL, errs
    scale = K.block_scale(name)
    ed, kl, g = engine.kron_head_elbo(p, X, Y, lik, jitter=K.JITTER, scale=scale, f_mu=f_mu)
    e_r, d_r, kl_r, g_r = ot.kron_head_elbo_and_grad(X, Y, p, lik, K.JITTER, scale=scale, f_mu=f_mu)
    ev, ek = abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r)
    print('%s %s elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e' % (name, lik, ed - kl, e_r, ev, ek))
    _check_grads('%s %s' % (name, lik), K.BLOCK_CASES[name]['D'], g, g_r, HEAD_KERN, HEAD_VEC + (('noise',) if lik == 'gaussian' else ()), tol=TOL)
    assert ev <= TOL and ek <= TOL, (ev, ek)
    v = engine.kron_head_elbo(p, X, Y, lik, jitter=K.JITTER, scale=scale, f_mu=f_mu, need_grad=False)
    assert v[0] == ed and v[1] == kl


def test_matern_factors_match_literal_restatement(engine):
    """f ('matern32', 'rbf'), g ('matern52', 'matern52') on the 2 x 1 grid against tests/kron_matern_ref.py"""
    X, Y, p = K.block_matern_fixture()
    name = K.BLOCK_MATERN[0]
    pred_r, (e_r, d_r, kl_r, g_r) = K.block_matern_oracle()
    out = engine.kron_predict(p, X, jitter=K.JITTER, g_offset=0.0)
    errs = [relerr(out[i], pred_r[i]) for i in range(9)]
    print('%s Matern predict: %s' % (name, ' '.join('%s %.1e' % (n, e) for n, e in zip(PRED_NAMES, errs))))
    assert max(errs) < TOL, errs
    scale = K.block_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    ev, ek = abs(ed - scale * d_r) / abs(scale * d_r), abs(kl - kl_r) / abs(kl_r)
    print('%s Matern elbo %.10e ref %.10e  data relerr %.1e  kl relerr %.1e' % (name, ed - kl, e_r, ev, ek))
    _check_grads(name + ' Matern', K.BLOCK_CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
    assert ev <= TOL and ek <= TOL, (ev, ek)
    v = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale, need_grad=False)
    assert v[0] == ed and v[1] == kl


@pytest.mark.parametrize('name', ['b21', 'b12', 'b3'])
def test_resident_rows_equal_host_rows(engine, name):
    """rows=(lo, hi) of the resident data set against the same rows passed from the host: the same bits in every returned array"""
    X, Y, p = K.block_problem(name)
    N = X.shape[0]
    engine.set_data(X, Y)
    for lo, hi in ((0, N), (5, N - 3)):
        a = engine.kron_elbo(p, X[lo:hi], Y[lo:hi], jitter=K.JITTER, scale=2.5)
        b = engine.kron_elbo(p, rows=(lo, hi), jitter=K.JITTER, scale=2.5)
        _bit_identical(a, b)


@pytest.mark.parametrize('name', ['b21', 'b12', 'b22'])
def test_without_kl_matches_reference_without_kl(engine, name):
    """include_kl=False: KL exactly 0, the gradient is the reference's data part alone (the restatement on b22)"""
    X, Y, p = K.block_problem(name)
    scale = K.block_scale(name)
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale, include_kl=False)
    e_r, d_r, kl_r, g_r = K.block_oracle_grad(name, False)
    full = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    assert kl == 0.0 and kl_r == 0.0 and ed == full[0]
    worst = _check_grads(name + ' no KL', K.BLOCK_CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
    print('%s include_kl=False worst gradient figure %.2e' % (name, worst))


@pytest.mark.parametrize('name', ['b21', 'b12'])
def test_empty_row_range_keeps_the_kl(engine, name):
    """rows=(k, k) and a host call with zero rows: data term 0, the KL bit for bit, without the KL an exactly zero gradient, with it the KL
    part of the gradient -- against the call on every row at scale 0 (bound 1e-13 of test_gpu_kron.py::_check_empty_rows) and against the
    reference at scale 0"""
    X, Y, p = K.block_problem(name)
    N = X.shape[0]
    engine.set_data(X, Y)
    full = engine.kron_elbo(p, rows=(0, N), jitter=K.JITTER, scale=3.0)
    kl_only = engine.kron_elbo(p, rows=(0, N), jitter=K.JITTER, scale=0.0)
    g_r = K.block_oracle_grad(name, True, 0.0)[3]
    assert kl_only[0] == 0.0 and kl_only[1] == full[1]
    _check_grads(name + ' scale 0', K.BLOCK_CASES[name]['D'], kl_only[2], g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
    worst = 0.0
    for empty in (dict(rows=(0, 0)), dict(rows=(17, 17)), dict(rows=(N, N)), dict(X=X[:0], Y=Y[:0])):
        e = engine.kron_elbo(p, jitter=K.JITTER, scale=3.0, **empty)
        z = engine.kron_elbo(p, jitter=K.JITTER, scale=3.0, include_kl=False, **empty)
        assert e[0] == 0.0 and e[1] == full[1] and z[0] == 0.0 and z[1] == 0.0
        for (k, x), (_, r), (_, v) in zip(_flat(e)[2:], _flat(kl_only)[2:], _flat(z)[2:]):
            assert np.all(v == 0.0), k
            err = np.max(np.abs(x - r)) / max(np.max(np.abs(r)), 1e-300)
            worst = max(worst, err)
            assert err <= 1e-13, (k, err)
    print('%s empty ranges: KL part of the gradient against the scale-0 call %.2e' % (name, worst))


@pytest.mark.parametrize('name', ['b21', 'b12'])
def test_one_row(engine, name):
    """N = 1 against the literal oracle"""
    import zigp_oracle as o
    import zigp_oracle_torch as ot
    X, Y, p = K.block_problem(name)
    n = int(np.flatnonzero(Y[:, 0] > 0)[0])
    X1, Y1 = np.ascontiguousarray(X[n:n + 1]), np.ascontiguousarray(Y[n:n + 1])
    out = engine.kron_predict(p, X1, jitter=K.JITTER, g_offset=-1.0)
    ref = [np.asarray(r).reshape(-1) for r in o.kron_build_predict(X1, p, K.JITTER, -1.0)]
    errs = [relerr(out[i], ref[i]) for i in range(9)]
    ed, kl, g = engine.kron_elbo(p, X1, Y1, jitter=K.JITTER, scale=500.0)
    e_r, d_r, kl_r, g_r = ot.kron_elbo_and_grad(X1, Y1, p, K.JITTER, scale=500.0)
    ev, ek = abs(ed - 500.0 * d_r) / abs(500.0 * d_r), abs(kl - kl_r) / abs(kl_r)
    print('%s N = 1: predict %.1e data %.1e kl %.1e' % (name, max(errs), ev, ek))
    _check_grads(name + ' N = 1', K.BLOCK_CASES[name]['D'], g, g_r, KERN_KEYS, VEC_KEYS, tol=TOL)
    assert max(errs) < TOL and ev <= TOL and ek <= TOL, (errs, ev, ek)


@pytest.mark.parametrize('name,cut', [('b21', 133), ('b3', 517), ('b22', 150)])
def test_two_shards_add_up(engine, name, cut):
    """two uneven shards, the KL counted once, against the whole batch (b3: 517 + 514 rows pad to 1024 each, the whole batch to 2048) --
    bounds of test_gpu_kron_nd.py::test_shard_additivity_many_tiles"""
    X, Y, p = K.block_problem(name)
    assert cut % 16 and (X.shape[0] - cut) % 16
    ed, kl, g = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=1.0)
    a = engine.kron_elbo(p, X[:cut], Y[:cut], jitter=K.JITTER, scale=1.0, include_kl=True)
    b = engine.kron_elbo(p, X[cut:], Y[cut:], jitter=K.JITTER, scale=1.0, include_kl=False)
    ev = abs((a[0] + b[0]) - ed) / abs(ed)
    worst = 0.0
    assert a[1] == kl and b[1] == 0.0
    for k in VEC_KEYS:
        ref = np.asarray(g[k])
        e = np.max(np.abs(np.asarray(a[2][k]) + np.asarray(b[2][k]) - ref)) / max(np.max(np.abs(ref)), 1e-300)
        worst = max(worst, e)
        assert e <= 1e-9, (k, e)
    for k in KERN_KEYS:
        for q in range(2):
            ref = np.asarray(g[k][q])
            e = np.max(np.abs(np.asarray(a[2][k][q]) + np.asarray(b[2][k][q]) - ref)) / max(np.max(np.abs(ref)), 1e-300)
            worst = max(worst, e)
            assert e <= 1e-8, (k, q, e)
    print('%s shards %d + %d vs whole: value %.1e worst gradient block %.1e' % (name, cut, X.shape[0] - cut, ev, worst))
    assert ev <= 1e-11, ev


def test_context_reuse_across_padded_sizes(engine):
    """one context takes grids of different padded sizes one after another (256 x 128, 128 x 256, 128 x 128 forced onto the panels,
    384 x 128, 256 x 128 again): its buffers are reused, grown and left larger than the next call needs.  Every result -- gradient step and
    prediction -- equals the same call on a fresh context bit for bit."""
    import zigp
    seq = [('b21', K.block_problem('b21')), ('b12', K.block_problem('b12')), ('d11b', K.problem('d11b')), ('b3', K.block_problem('b3')),
           ('b21', K.block_problem('b21'))]

    def run(e, name, X, Y, p):
        e.set_kron_panels(name == 'd11b')
        try:
            return e.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0), e.kron_predict(p, X, jitter=K.JITTER, g_offset=-1.0)
        finally:
            e.set_kron_panels(False)

    used = [run(engine, name, *xyp) for name, xyp in seq]
    for (name, xyp), (res, pred) in zip(seq, used):
        fresh = zigp.DenseEngine(0)
        try:
            res_f, pred_f = run(fresh, name, *xyp)
        finally:
            fresh.close()
        _bit_identical(res, res_f)
        assert np.array_equal(pred, pred_f), name
    _bit_identical(used[0][0], used[4][0])
    assert np.array_equal(used[0][1], used[4][1])
    print('context reuse: %s == fresh contexts, bit for bit' % ' -> '.join(n for n, _ in seq))
