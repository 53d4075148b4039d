"""Stage-level parity of the M x M launches of the Kronecker GEMM-panel path (csrc/zigp_kron.hip kron_run_panels) at one to three 128-row
blocks per factor.  DenseEngine.test_kron_panel_step (zigp_test_kron_panel_step, include/zigp_diag.h) runs one ordinary value-and-gradient
step through the production host code and copies the device buffers out right behind the launches that fill them; tests/kronp_ref.py
restates every launch from the tapped inputs of that launch alone (tests/test_cpu_kronp_ref.py shows on the CPU which mistakes that catches).

* exact tier: the small-integer / dyadic construction of kronf_ref.exact_problem (K_p + jitter I = c_p I, c_p a power of 4) with injected
  integer cotangents: every tap equals the float64 restatement with ==, padding included -- identity in the padding of K_p and P_p, exact
  zeros in the padding of every grid image, gu / gs compact at [M0 M1] -- and the sums over the points equal the construction's integers;
* bound tier: the random fixtures of kron_nd.BLOCK_CASES and the grids 1 x 130, 128 x 129, 200 x 3: every launch holds
  err_gpu <= 4 err_np + 16 eps S against the long-double restatement (S = sum |a||b| over that launch's tapped operands); the split-K plane
  sum equals the float64 sum in plane order bit for bit; P_p is held by its residual against 8 times that of SciPy's Cholesky inverse;
* the step is the ordinary step: value, KL and every gradient equal kron_elbo / kron_head_elbo bit for bit with and without taps, and the
  tapped krow, gu, gs compose to those gradients through the host chain rule bit for bit; facts[] carries Mq, nb, Nc and each reduction's S.
Every test prints its figures (pytest -s); they are recorded in profiles/kron_panel_stage_parity.log."""
import numpy as np
import pytest

import kron_nd as K
import kronf_ref as F
import kronp_ref as R
from test_gpu_kron_nd import _bit_identical

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings(K.READ_ONLY_NOTE)]
EPS = np.finfo(np.float64).eps
GRID_TAPS = ('U', 'S2', 'T0', 'Al', 'dAl', 'dS2', 'T1_a', 'dU', 'T1_b')


def _meta(p, tag):
    Z = [p['Z' + tag][0], p['Z' + tag][1]]
    M = (Z[0].shape[0], Z[1].shape[0])
    return M, Z, np.asarray(p['u_%ss_sqrt' % tag], dtype=np.float64).reshape(M)


def _check_facts(out, p, N, tags):
    f = out['facts']
    Nc = max(1024, -(-N // 1024) * 1024)
    assert f['Nc'] == Nc and f['nk'] == Nc // 16
    for h, tag in enumerate(tags):
        M = _meta(p, tag)[0]
        nb = tuple(-(-m // 128) for m in M)
        L = f['lat'][h]
        assert (L['Mq0'], L['Mq1'], L['nb0'], L['nb1']) == (128 * nb[0], 128 * nb[1], nb[0], nb[1])
        assert L['S_dP0'] == R.split_k_slices(f['nk'], nb[0], nb[0]) and L['S_dP1'] == R.split_k_slices(f['nk'], nb[1], nb[1])
        assert L['S_dAl'] == L['S_dS2'] == R.split_k_slices(f['nk'], nb[0], nb[1])


def _check_padding(t, M):
    for q in range(2):
        for k in ('K', 'P'):
            A = t[k][q]
            assert np.array_equal(A[M[q]:, M[q]:], np.eye(A.shape[0] - M[q])) and not A[M[q]:, :M[q]].any() and not A[:M[q], M[q]:].any(), (k, q)
        assert not t['krow_n'][q][M[q]:].any() and not t['krow'][q][M[q]:].any(), q
    for k in GRID_TAPS:
        assert not t[k][M[0]:].any() and not t[k][:, M[1]:].any(), k
    assert t['gu'].shape == M and t['gs'].shape == M


def _compose(out, p, tags, ordinary):
    """the tapped krow, gu, gs through kron_assemble_grads' chain rule (dZ = krow / ell^2, d ell = sum_m krow / ell^3, m ascending; d u = gu,
    d s = gs): the step's gradients, bit for bit"""
    g = ordinary[2]
    for h, tag in enumerate(tags):
        t = out['lat'][h]
        M = _meta(p, tag)[0]
        assert np.array_equal(t['gu'].reshape(-1), np.asarray(g['u_%sm' % tag]).reshape(-1))
        assert np.array_equal(t['gs'].reshape(-1), np.asarray(g['u_%ss_sqrt' % tag]).reshape(-1))
        for q in range(2):
            ell = np.asarray(p['ell_' + tag][q], dtype=np.float64).reshape(-1)
            D, kr = ell.size, t['krow'][q][:M[q]]
            assert np.array_equal(kr[:, 1:1 + D] / (ell * ell), np.asarray(g['Z' + tag][q]).reshape(M[q], D)), (tag, q)
            dl = np.zeros(D)
            for m in range(M[q]):
                dl = dl + kr[m, 1 + D:1 + 2 * D]
            assert np.array_equal(dl / (ell * ell * ell), np.asarray(g['ell_' + tag][q]).reshape(-1)), (tag, q)


@pytest.mark.parametrize('name,planes_of', [('b21', 'dAl'), ('b12', 'dS2'), ('bmix', 'dP1'), ('b3', 'dP0')])
def test_hook_step_is_the_ordinary_step(engine, name, planes_of):
    """value, KL and gradients of the hook equal kron_elbo's bit for bit, with taps and without; facts; the taps compose to the gradients"""
    X, Y, p = K.block_problem(name)
    scale = K.block_scale(name)
    ordinary = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale)
    for taps in (True, False):
        out = engine.test_kron_panel_step(p, X, Y, jitter=K.JITTER, scale=scale, taps=taps, planes_of=planes_of)
        _bit_identical((out['elbo_data'], out['kl'], {k: v for k, v in out['grads'].items() if k != 'f_mu'}), ordinary)
        _check_facts(out, p, X.shape[0], 'fg')
        if taps:
            _compose(out, p, 'fg', ordinary)
    _bit_identical(engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=scale), ordinary)      # and leaves the context as it found it
    if name == 'b3':
        assert [L['S_dP0'] for L in out['facts']['lat']] == [56, 56] and out['facts']['nk'] == 128      # the one reduction with S != nk


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_hook_head_step_is_the_ordinary_step(engine, lik):
    X, Y, p = K.block_problem('b12')
    Y, p = ((Y > 0) * 1.0 if lik == 'bernoulli' else Y), K.head_params(p)
    ordinary = engine.kron_head_elbo(p, X, Y, lik, jitter=K.JITTER, scale=3.0, f_mu=0.2)
    out = engine.test_kron_panel_step(p, X, Y, lik=lik, jitter=K.JITTER, scale=3.0, f_mu=0.2)
    _bit_identical((out['elbo_data'], out['kl'], out['grads']), ordinary)
    _compose(out, p, 'f', ordinary)


def test_hook_refuses_what_it_cannot_run(engine):
    import ctypes as C
    from zigp import _lib
    lib = engine.lib
    assert lib.zigp_test_kron_panel_step(None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_panel_step(engine.ctx, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_panel_step(engine.ctx, C.byref(_lib.zigp_stage_kron_panels())) == _lib.ZIGP_EARG      # no parameters
    X, Y, p = K.problem('d11b')                              # 32 x 32: the fused kernels take it
    with pytest.raises(ValueError, match='runs on the fused Kronecker kernels'):
        engine.test_kron_panel_step(p, X, Y, jitter=K.JITTER)
    engine.set_kron_panels(True)
    try:
        forced = engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0)
        out = engine.test_kron_panel_step(p, X, Y, jitter=K.JITTER, scale=2.0)
    finally:
        engine.set_kron_panels(False)
    _bit_identical((out['elbo_data'], out['kl'], {k: v for k, v in out['grads'].items() if k != 'f_mu'}), forced)
    Xb, Yb, pb = K.block_problem('b21')
    with pytest.raises(ValueError):
        engine.test_kron_panel_step(pb, Xb[:0], Yb[:0])
    with pytest.raises(ValueError):
        engine.test_kron_panel_step(pb, Xb, Yb, jitter=-1.0)
    _bit_identical(engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0), engine.kron_elbo(p, X, Y, jitter=K.JITTER, scale=2.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# exact tier
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid_f,grid_g,planes_of', [((130, 12), (12, 130), 'dAl'), ((257, 5), (129, 3), 'dP0'), ((130, 129), (128, 129), 'dS2')])
@pytest.mark.parametrize('jitter,kl', [(0.25, True), (0.0, False)])
def test_exact_tier(engine, grid_f, grid_g, planes_of, jitter, kl):
    e = F.exact_problem(grid_f, grid_g, (1, 1), 300, jitter=jitter, seed=3)
    p = e['p']
    out = engine.test_kron_panel_step(p, e['X'], e['Y'], jitter=jitter, scale=1.0, include_kl=kl, inject=[L['cot'] for L in e['lat']],
                                      planes_of=planes_of)
    _check_facts(out, p, 300, 'fg')
    for h, tag in enumerate('fg'):
        t, L = out['lat'][h], e['lat'][h]
        M, Z, s = _meta(p, tag)
        assert M == L['M']
        _check_padding(t, M)
        # the factor stage: K_p + jitter I = c I, L = sqrt(c) I, W = I / sqrt(c), P = I / c on the real part, the identity behind it
        for q in range(2):
            c, Mq = L['c'][q], t['K'][q].shape[0]
            d = np.concatenate([np.full(M[q], 1.0), np.ones(Mq - M[q])])
            for k, v in (('K', c), ('L', np.sqrt(c)), ('W', 1 / np.sqrt(c)), ('P', 1 / c)):
                d[:M[q]] = v
                assert np.array_equal(t[k][q], np.diag(d)), (tag, k, q)
        # the sums over the points: the construction's integers, zero padding
        N = e['N']
        assert np.array_equal(t['cot'][:, :N], L['cot']) and np.array_equal(t['part'][:, :N], L['part'])
        for k in ('dAl', 'dS2'):
            assert np.array_equal(t[k][:M[0], :M[1]], L['sums'][k]), (tag, k)
        for q in range(2):
            assert np.array_equal(t['dP_red'][q][:M[q], :M[q]], L['sums']['dP%d' % q]) and not t['dP_red'][q][M[q]:].any() and not t['dP_red'][q][:, M[q]:].any()
            assert np.array_equal(t['krow_n'][q][:M[q], 0], L['sums']['Kr%d' % q][:, 0]) and not t['krow_n'][q][:, 1:].any(), (tag, q)
        # every launch == its float64 restatement from the tapped inputs, whole padded images
        r = R.restate(t, M, Z, s, jitter, kl, planes_of)
        for name, (v, S) in r.items():
            a = R.tap_of(t, name, planes_of)
            if name == 'klv':       # the logarithms are not exact: sum log s^2 and the two logdets under the bound, the two dyadic sums with ==
                assert np.array_equal(a[[0, 2]], v[[0, 2]]) and np.all(np.abs(a - v) <= 16 * EPS * S), (tag, a, v)
            elif name == 'gs' and kl:       # -1 / s is dyadic for s in {1, 2} only
                mask = F.exact_gs_mask(L)
                assert np.array_equal(a[mask], v[mask]) and np.all(np.abs(a - v) <= 16 * EPS * S), tag
            else:
                assert np.array_equal(a, v), (tag, name)
        # and the finish stage of the fused path's reference on the same construction (an independent statement of the same algebra)
        fin = F.exact_finish(L, e['D'], jitter, kl)
        for q in range(2):
            assert np.array_equal(t['G'][q][:M[q], :M[q]], fin['G%d' % q][0]) and np.array_equal(t['PdPP'][q][:M[q], :M[q]], fin['PXP%d' % q][0]), (tag, q)
            assert np.array_equal(t['krow'][q][:M[q]], fin['krow%d' % q][0]), (tag, q)
        assert np.array_equal(t['gu'], fin['gu'][0])
        mask = F.exact_gs_mask(L) if kl else np.ones(M, dtype=bool)
        assert np.array_equal(t['gs'][mask], fin['gs'][0][mask])
    print('exact tier f %s g %s jitter %g kl %s planes of %s (S %s): every tap == the float64 restatement' %
          (grid_f, grid_g, jitter, kl, planes_of, [L['S_' + planes_of] for L in out['facts']['lat']]))


# ---------------------------------------------------------------------------------------------------------------------------------
# bound tier
# ---------------------------------------------------------------------------------------------------------------------------------
def _p_residual(case, q, Kq, Pq):
    """P_p = K_p^-1 by its residual against 8 times that of SciPy's Cholesky inverse of the same tapped K_p (the bar of test_gpu_kronf_stages.py)"""
    import scipy.linalg as sl
    n = Kq.shape[0]
    c = sl.cho_factor(Kq, lower=True)
    r_ref = float(np.max(np.abs(sl.cho_solve(c, np.eye(n)) @ Kq - np.eye(n))))
    r_gpu = float(np.max(np.abs(Pq @ Kq - np.eye(n))))
    print('  %s P_%d residual max|P K - I| = %.3e   (SciPy Cholesky inverse: %.3e, ratio %.2f, cond %.2e)' % (case, q, r_gpu, r_ref, r_gpu / r_ref, np.linalg.cond(Kq)))
    assert r_ref > 0 and r_gpu <= 8 * r_ref, (case, q, r_gpu, r_ref)


def _bound_tier(engine, case, X, Y, p, scale, kl, planes_of):
    out = engine.test_kron_panel_step(p, X, Y, jitter=K.JITTER, scale=scale, include_kl=kl, planes_of=planes_of)
    _check_facts(out, p, X.shape[0], 'fg')
    worst = {}
    for h, tag in enumerate('fg'):
        t = out['lat'][h]
        M, Z, s = _meta(p, tag)
        _check_padding(t, M)
        for q in range(2):
            _p_residual('%s %s' % (case, tag), q, t['K'][q][:M[q], :M[q]], t['P'][q][:M[q], :M[q]])
            assert not np.triu(t['W'][q], 1).any()      # P = W^T W reads whole diagonal blocks of W
        r64 = R.restate(t, M, Z, s, K.JITTER, kl, planes_of)
        rld = R.restate(t, M, Z, s, K.JITTER, kl, planes_of, dtype=np.longdouble, with_S=False)
        for name, (v, S) in r64.items():
            a = np.asarray(R.tap_of(t, name, planes_of), dtype=np.longdouble)
            if name == 'red':       # sequential float64 adds in plane order: the kernel's own arithmetic
                assert t['planes'].shape[0] == out['facts']['lat'][h]['S_' + planes_of]
                assert np.array_equal(R.tap_of(t, name, planes_of), v), (case, tag, 'plane sum')
                continue
            vl = rld[name][0]
            err_gpu, err_np, S = np.abs(a - vl), np.abs(np.asarray(v, dtype=np.longdouble) - vl), np.asarray(S, dtype=np.longdouble)
            bad = err_gpu > 4 * err_np + 16 * EPS * S
            # the printed figure leaves out elements whose eps S is below the normal range (products of far-off entries of W that
            # underflow); the bound above does not
            big = S > 2.0 ** -960
            ratio = float(np.max(np.where(big, err_gpu / (EPS * np.where(big, S, 1)), 0.0)))
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert not bad.any(), (case, tag, name, ratio, int(bad.sum()))
    print('  %s err_gpu / (eps S) per launch: %s' % (case, '  '.join('%s %.2f' % kv for kv in worst.items())))


@pytest.mark.parametrize('name,planes_of', [('b21', 'dAl'), ('b12', 'dAl'), ('bmix', 'dS2'), ('b3', 'dP0'), ('bedge', 'dP0'), ('b22', 'dAl')])
def test_bound_tier_block_cases(engine, name, planes_of):
    X, Y, p = K.block_problem(name)
    _bound_tier(engine, name, X, Y, p, K.block_scale(name), True, planes_of)


@pytest.mark.parametrize('grid', K.BLOCK_EDGE_GRIDS)
@pytest.mark.parametrize('kl', [True, False])
def test_bound_tier_edge_grids(engine, grid, kl):
    """1 x 130 (one point in a factor), 128 x 129 (a full block beside one row past it), 200 x 3; with and without the KL"""
    X, Y, p = K.block_edge_problem(grid)
    _bound_tier(engine, '%dx%d kl %s' % (grid + (kl,)), X, Y, p, 3.0, kl, 'dP1')
