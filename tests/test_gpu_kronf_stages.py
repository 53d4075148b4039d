"""Stage-level parity of the register-resident fused Kronecker path (csrc/zigp_kronf.hip, zigp_kronl.h): the per-point tile kernels
k_kf_forward / k_kf_backward (+ k_kf_reduce) and k_kfl_forward / k_kfl_backward / k_kfl_accum, plus what the two forward M x M kernels
(k_kf_factor, k_kf_latent / k_kfl_latent) leave behind.  DenseEngine.test_kron_fused_step (zigp_test_kron_fused_step, include/zigp_diag.h)
runs one REAL value-and-gradient step through kronf_run and snapshots its device buffers after the launch that produces each of them; the
references are the NumPy restatements of tests/kronf_ref.py (pinned on the CPU by tests/test_cpu_kronf_ref.py).

* exact tier: inputs with which every K tile is an exact selector and every sum a sum of integers (kronf_ref.exact_problem) and injected
  integer cotangents -- every tap is compared bit for bit, padding and capacity blocks included, at the shapes that reach every
  instantiation, both tiles-per-wave regimes and every number of row ranges (asserted from the hook's `facts`).
* bound tier: ordinary fixtures of tests/kron_nd.py and the ill-conditioned pptr 32 x 32 init, nothing injected; the truth is the long
  double restatement on the stage's own inputs as tapped, the rule the project's own: per element err_gpu <= 4 err_np + 16 eps S.
  P_p = K_p^-1 is held by its residual max |P K - I| against 8 times that of SciPy's float64 Cholesky inverse of the same tapped K.
* hook hygiene: the tapped step returns the bits of an ordinary call, repeats its taps, leaves later calls unchanged, and refuses what
  does not run on the fused kernels.

* finish stage: the KL scalars of the latent kernels and everything the reverse M x M kernels (k_kf_finish, k_kfl_finish<1..3>) leave --
  krow0, krow1, gu, gs; larger grids: the G rows of stage 3, and krow recomputed from those tapped rows -- against kronf_ref.finish /
  kl_scalars in long double on the stage's own tapped inputs, with include_kl on and off: every bound-tier fixture, the heads, the pptr
  init, the edge grids at N = 33 (one-point factors, every kf_lds_mm shape, the row-block bounds of k_kfl_finish, 15 moment columns), two
  latents with different grids; bit for bit on the exact tier; and the gradients a step returns against the host chain rule
  (kron_assemble_grads) of the tapped results.  tests/test_cpu_kronf_finish_ref.py pins that restatement to autograd and shows that the rule
  catches each of eight deliberate mistakes on these fixtures.  The Matern additions of the stage (k_kf_kd_prepare, the second k_kf_finish,
  k_kf_krow_merge, k_kfl_krow_kinds) are held in tests/test_gpu_kron_matern_fused.py.

Every test prints STAGE-LOG lines (profiles/kronf_stage_parity.log and profiles/kronf_finish_parity.log keep a run's).  k_fit_update has no
stage test: it stays covered only through the fit-loop tests (tests/test_gpu_kron_nd.py, test_gpu_head_fit.py, test_gpu_kron_matern_fused.py),
which compare device steps with host-stepped ones."""
import ctypes as C

import numpy as np
import pytest

import kron_nd
import kronf_ref as kr

pytestmark = pytest.mark.gpu
EPS = kr.EPS
NS = (1, 15, 16, 17, 1000, 1025)
N_BWD_TPW2 = 8211          # 576 tiles over 512 waves (two latents): two tiles per wave in the backward launch
N_FWD_TPW2 = 33000         # 2112 tiles over 2048 waves: two tiles per wave in the small-grid forward launch


def _log(kernel, case, text):
    print('STAGE-LOG %-14s %-40s %s' % ('kronf/' + kernel, case, text))


def _rup(n, m):
    return -(-n // m) * m


def _cap(grids):
    return (2, 2) if all(g[0] <= 32 and g[1] <= 32 for g in grids) else (1, 7)


def _pad(a, shape):
    out = np.zeros(shape)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _check_facts(facts, grids, N, nlat):
    """the plan of the step as the hook reports it, against the rules of kf_plan / kronf_run restated here"""
    cap = _cap(grids)
    large = cap == (1, 7)
    nb = [(_rup(g[0], 16) // 16, _rup(g[1], 16) // 16) for g in grids]
    Npad = max(1024, _rup(N, 1024))
    ntiles = Npad // 16
    assert facts['large'] == int(large) and (facts['nb0c'], facts['nb1c']) == cap
    assert (facts['nb0_f'], facts['nb1_f']) == nb[0] and (facts['nb0_g'], facts['nb1_g']) == nb[-1]
    assert facts['large_exact'] == int(large and all(b == cap for b in nb))
    assert facts['Npad'] == Npad and facts['ntiles'] == ntiles
    waves_f = min(ntiles, 1024 // nlat if large else 2048)
    assert facts['tpw_fwd'] == -(-ntiles // waves_f)
    assert facts['one_launch'] == int(large or nlat == 1 or nb[0] == nb[1])
    if not large:
        tpw = -(-ntiles // min(ntiles, 1024 // nlat))
        assert facts['tpw_bwd'] == tpw and facts['nranges'] == 1 and facts['tps'] == 0
        assert facts['nparts'] == _rup(-(-ntiles // tpw), 4)
    else:
        tps = max(4, min(64, ntiles // 16))
        assert facts['tps'] == tps and facts['nparts'] == -(-ntiles // tps)
        assert facts['range_tiles'] % tps == 0 and facts['nranges'] == -(-ntiles // facts['range_tiles'])
    return cap, nb


# =====================================================================================================================================
# exact tier
# =====================================================================================================================================
# id -> (f grid, g grid or None: a second latent on f's grid); the instantiation each reaches is asserted from the facts
SHAPES = {
    's11': ((6, 5), None),           # k_kf_*<1,1>
    's12': ((9, 20), None),          # <1,2>
    's21': ((20, 9), None),          # <2,1>
    's22p': ((17, 31), None),        # <2,2>, one row past a block / one short of two
    's22': ((32, 32), None),         # <2,2>, no padding
    'mix': ((20, 9), (9, 20)),       # block counts differ: one launch per latent
    'under': ((6, 5), (20, 20)),     # a latent under the capacity AND under the other latent
    'Lx': ((10, 100), None),         # k_kfl_*<1,7,true,true>: compile-time bounds
    'Lx2': ((16, 112), None),        # the same instantiation with no padding row at all
    'Lr': ((9, 50), None),           # <1,7,true,false>: runtime bounds
    'Lrmix': ((16, 112), (9, 50)),   # runtime bounds because the latents differ
}
DS = [(2, 1), (1, 1), (3, 2), (7, 7)]
INSTANCE = {'s11': (0, 0, (1, 1)), 's12': (0, 0, (1, 2)), 's21': (0, 0, (2, 1)), 's22p': (0, 0, (2, 2)), 's22': (0, 0, (2, 2)), 'mix': (0, 0, (2, 1)),
            'under': (0, 0, (1, 1)), 'Lx': (1, 1, (1, 7)), 'Lx2': (1, 1, (1, 7)), 'Lr': (1, 0, (1, 4)), 'Lrmix': (1, 0, (1, 7))}


def _assert_exact_taps(tag, t, L, D, N, cap):
    """every tap of one latent of an exact-tier step against kronf_ref.exact_problem, bit for bit"""
    M = L['M']
    Mq = (_rup(M[0], 16), _rup(M[1], 16))
    for q in range(2):
        c, R = L['c'][q], _rup(M[q], 32)
        K = t['K'][q][:R, :R]
        want = np.eye(R)
        want[:M[q], :M[q]] *= c
        assert np.array_equal(K, want), '%s: K_%d + jitter I is not %g I (identity padded)' % (tag, q, c)
        P = _pad(np.eye(M[q]) / c, (Mq[q], Mq[q]))
        assert np.array_equal(t['P'][q], P), '%s: P_%d' % (tag, q)
        assert np.array_equal(t['PF'][q], kr.frag_image(t['P'][q], False)), '%s: fragment image of P_%d' % (tag, q)
        assert np.array_equal(t['dvec'][q][:Mq[q]], np.diag(t['P'][q])), '%s: dvec_%d' % (tag, q)
        assert abs(t['dvec'][q][Mq[q]] - M[q] * np.log(c)) <= 8 * EPS * M[q] * abs(np.log(c)), '%s: logdet K_%d' % (tag, q)
        assert np.array_equal(t['zc'][q], 0.5 * (L['Z'][q].min(0) + L['Z'][q].max(0))), '%s: zc_%d is not the mid-range' % (tag, q)
        assert np.array_equal(t['Zs'][q], _pad(L['Z'][q] * (1.0 / L['ell'][q]), (Mq[q], D[q]))), '%s: Zs_%d' % (tag, q)
    U = _pad(L['U'], Mq)
    for k, want in (('U', U), ('S2', _pad(L['S2'], Mq)), ('T0', U / L['c'][1]), ('T1', U / L['c'][0]), ('Al', U / (L['c'][0] * L['c'][1]))):
        assert np.array_equal(t[k], want), '%s: %s' % (tag, k)
    for k, src, tr in (('AlF', 'Al', False), ('S2F', 'S2', False), ('AlTF', 'Al', True), ('S2TF', 'S2', True)):
        assert np.array_equal(t[k], kr.frag_image(t[src], tr)), '%s: fragment image %s' % (tag, k)
    assert np.array_equal(t['part'][:, :N], L['part']), '%s: part' % tag
    assert not np.any(t['part'][:, N:]), '%s: part rows N .. Npad are not exact zeros' % tag
    assert not np.any(t['cot'][:, N:]), '%s: the point-wise kernel left a cotangent on a padding point' % tag
    want = kr.work_image({k: (v, None) for k, v in L['sums'].items()}, M, D, cap)
    bad = np.flatnonzero(t['work'] != want)
    assert bad.size == 0, '%s: %d elements of the work block differ, first at %d: %r instead of %r' % (tag, bad.size, bad[0], t['work'][bad[0]], want[bad[0]])
    # ---- the finish stage.  The steps of this tier count the KL; tests/test_cpu_kronf_finish_ref.py::test_exact_tier_finish_is_exact shows that
    # on these inputs krow, gu and -- where s is 1 or 2 (-1 / s dyadic) -- gs are exact WITH the KL terms, so the comparison is `==`; gs at s = 3
    # is rounded and stays out.
    jitter = L['c'][0] - L['var'][0]
    f = kr.exact_finish(L, D, jitter, True)
    keep = kr.exact_gs_mask(L)
    for q in range(2):
        assert np.array_equal(t['krow'][q], f['krow%d' % q][0]), '%s: krow%d' % (tag, q)
    assert np.array_equal(t['gu'], f['gu'][0]), '%s: gu' % tag
    assert keep.any() and np.array_equal(t['gs'][keep], f['gs'][0][keep]), '%s: gs where 1 / s is exact' % tag
    if 'G' in t:
        assert np.array_equal(t['G'][0][:M[0], :M[0]], f['G0'][0]) and np.array_equal(t['G'][1][:M[1], :M[1]], f['PXP1'][0]), '%s: G rows of stage 3' % tag
    assert_unwritten(tag, t, M, D)


def _exact_step(engine, shape, D, N, lik, jitter=0.0):
    gf, gg = SHAPES[shape]
    two = lik == 'onoff'
    grids = [gf, gg or gf] if two else [gf]
    e = kr.exact_problem(grids[0], grids[1] if two else None, D, N, jitter, seed=17 + N % 97)
    p = e['p'] if two else kron_nd.head_params(e['p'])
    out = engine.test_kron_fused_step(p, e['X'], e['Y'], lik=lik, jitter=jitter, scale=1.0, inject=[L['cot'] for L in e['lat']])
    return grids, e, out


@pytest.mark.parametrize('D', DS, ids=lambda d: 'D%d%d' % d)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_exact_tier_every_tap_bit_for_bit(engine, shape, D):
    gf, gg = SHAPES[shape]
    large = _cap([gf, gg or gf]) == (1, 7)
    liks = ['onoff'] + (['gaussian'] if gg is None else [])
    ns = list(NS)
    if D == (2, 1):
        ns += [N_BWD_TPW2] + ([] if large else [N_FWD_TPW2])
    reached = set()
    try:
        for lik in liks:
            for N in ns:
                settings = [1024]
                if large and N in (1025, N_BWD_TPW2):
                    settings = [1024, 80, 24] if N == 1025 else [1024, 400, 120]       # 1, 2 and many row ranges, the last one partial
                ranges = []
                for tiles in settings:
                    engine.set_kron_range_tiles(tiles)
                    grids, e, out = _exact_step(engine, shape, D, N, lik)
                    f = out['facts']
                    cap, nb = _check_facts(f, grids, N, len(grids))
                    assert (f['large'], f['large_exact'], (f['nb0_f'], f['nb1_f'])) == INSTANCE[shape]
                    for h, L in enumerate(e['lat']):
                        _assert_exact_taps('%s D%s %s N=%d latent %d (range tiles %d)' % (shape, D, lik, N, h, tiles), out['lat'][h], L, D, N, cap)
                    ranges.append(f['nranges'])
                    reached.add((f['tpw_fwd'] > 1, f['tpw_bwd'] > 1))
                    if large:
                        last = f['ntiles'] - (f['nranges'] - 1) * f['range_tiles']
                        if tiles != 1024:
                            assert 0 < last < f['range_tiles'], 'the last row range is not a partial one'
                if len(settings) == 3:
                    assert ranges[0] == 1 and ranges[1] == 2 and ranges[2] >= 6, ranges
    finally:
        engine.set_kron_range_tiles(1024)
    if D == (2, 1):
        assert (False, True) in reached or (True, True) in reached, 'no step with more than one tile per wave in the backward launch'
        assert large or (True, True) in reached, 'no small-grid step with more than one tile per wave in the forward launch'
    _log('exact', '%s D%s' % (shape, D), 'bit-equal: %d liks x N %s, tpw>1 (fwd, bwd) regimes reached %s' % (len(liks), ns, sorted(reached)))


@pytest.mark.parametrize('shape', ['mix', 'Lr'])
def test_exact_tier_with_a_dyadic_jitter(engine, shape):
    """var_p + jitter a power of 4 with jitter = 1/4: the constants of `part` are no longer the variances themselves
    (part = var0^2 / c0, var1^2 / c1, u r0 r1, s^2 r0^2 r1^2 with r_p = var_p / c_p = 15/16, 3/4, 63/64)."""
    D = (2, 1)
    for N in (17, 1000):
        grids, e, out = _exact_step(engine, shape, D, N, 'onoff', jitter=0.25)
        cap, nb = _check_facts(out['facts'], grids, N, 2)
        for h, L in enumerate(e['lat']):
            hit = L['part'][0] != 0
            assert np.all(L['part'][0][hit] == L['var'][0] ** 2 / L['c'][0]) and L['var'][0] ** 2 / L['c'][0] != L['var'][0]
            _assert_exact_taps('%s jitter 1/4 N=%d latent %d' % (shape, N, h), out['lat'][h], L, D, N, cap)
    _log('exact', '%s jitter 1/4' % shape, 'bit-equal')


# =====================================================================================================================================
# bound tier
# =====================================================================================================================================
TINY = float(np.finfo(np.float64).tiny)      # 2^-1022: below it float64 has no relative accuracy (gradual underflow)


def _rule(kernel, case, name, gpu, ref64, truth, S):
    """per element err_gpu <= 4 err_np + 16 eps S; returns the largest err_gpu / (eps S).
    Where eps S itself is below the normal range (products of two K entries that underflow: the time factor of the pptr init has
    lengthscale 0.005 at an inducing spacing of 0.035) the rounding model behind the rule does not hold -- the absolute error of a
    subnormal result is a multiple of 2^-1074 whatever S is -- so those elements get 2^-1022 of absolute allowance and stay out of
    the printed ratio (their number is printed)."""
    truth = np.asarray(truth, dtype=np.longdouble)
    S = np.asarray(S, dtype=np.float64)
    err_gpu = np.asarray(np.abs(np.asarray(gpu, dtype=np.longdouble) - truth), dtype=np.float64)
    err_np = np.asarray(np.abs(np.asarray(ref64, dtype=np.longdouble) - truth), dtype=np.float64)
    live = S > 0
    assert not np.any(np.asarray(gpu)[~live]), '%s %s %s: a value where the sum has no term' % (kernel, case, name)
    normal = EPS * S >= TINY
    r_gpu = float(np.max(err_gpu[normal] / S[normal] / EPS)) if normal.any() else 0.0
    r_np = float(np.max(err_np[normal] / S[normal] / EPS)) if normal.any() else 0.0
    under = int(np.sum(live & ~normal))
    _log(kernel, case, '%-4s max err_gpu / (eps S) = %7.3f   (numpy float64: %7.3f)%s' % (name, r_gpu, r_np, '   [%d elements in the underflow range]' % under if under else ''))
    bad = err_gpu > 4 * err_np + 16 * EPS * S + np.where(normal, 0.0, TINY)
    assert not bad.any(), '%s %s %s: %d elements beyond 4 err_np + 16 eps S, worst err_gpu / (eps S) = %.2f' % (kernel, case, name, bad.sum(), r_gpu)
    return r_gpu


def _p_residual(kernel, case, q, K, P):
    """max |P K - I| in long double for the kernel's P and for SciPy's float64 Cholesky inverse of the same K"""
    import scipy.linalg as sl
    Kl = np.asarray(K, dtype=np.longdouble)
    eye = np.eye(K.shape[0], dtype=np.longdouble)
    res = lambda Pm: float(np.max(np.abs(np.asarray(Pm, dtype=np.longdouble) @ Kl - eye)))
    Pref = sl.cho_solve(sl.cho_factor(K, lower=True), np.eye(K.shape[0]))
    r_gpu, r_ref = res(P), res(Pref)
    _log(kernel, case, 'P_%d residual max|P K - I| = %.3e   (SciPy Cholesky inverse: %.3e, cond %.2e)' % (q, r_gpu, r_ref, np.linalg.cond(K)))
    assert r_ref > 0 and r_gpu <= 8 * r_ref, '%s P_%d: residual %.3e against 8 x %.3e' % (case, q, r_gpu, r_ref)


def _bound_latent(case, large, t, Z, ell, var, M, D, X, N, cap):
    """one latent of a tapped step: latent, forward and backward stages against the long double restatement on the tapped inputs"""
    Mq = (_rup(M[0], 16), _rup(M[1], 16))
    sfx = 'l' if large else ''
    for q in range(2):
        _p_residual('factor', case, q, t['K'][q][:M[q], :M[q]], t['P'][q][:M[q], :M[q]])
        assert not np.any(t['P'][q][M[q]:]) and not np.any(t['P'][q][:, M[q]:])
        assert np.array_equal(t['PF'][q], kr.frag_image(t['P'][q], False))
    P = [t['P'][q][:M[q], :M[q]] for q in range(2)]
    U, Al, S2 = t['U'][:M[0], :M[1]], t['Al'][:M[0], :M[1]], t['S2'][:M[0], :M[1]]
    for k, src, tr in (('AlF', 'Al', False), ('S2F', 'S2', False), ('AlTF', 'Al', True), ('S2TF', 'S2', True)):
        assert np.array_equal(t[k], kr.frag_image(t[src], tr)), '%s: fragment image %s' % (case, k)
    # ---- k_kf_latent / k_kfl_latent
    l64, lld = kr.latent(P[0], P[1], U), kr.latent(P[0], P[1], U, dtype=np.longdouble)
    for k in ('T0', 'T1', 'Al'):
        assert not np.any(t[k][M[0]:]) and not np.any(t[k][:, M[1]:]), '%s: %s padding' % (case, k)
        _rule('latent' + sfx, case, k, t[k][:M[0], :M[1]], l64[k][0], lld[k][0], l64[k][1])
    # ---- forward
    args = (P[0], P[1], Al, S2, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N)
    f64, S = kr.forward(*args)
    fld, _ = kr.forward(*args, dtype=np.longdouble)
    assert not np.any(t['part'][:, N:]), '%s: part rows N .. Npad' % case
    for r, k in enumerate(('q0', 'q1', 'mean', 'st')):
        _rule('forward' + sfx, case, k, t['part'][r, :N], f64[r], fld[r], S[r])
    # ---- backward (+ accumulate) + reduce
    assert not np.any(t['cot'][:, N:]), '%s: cotangents of padding points' % case
    bargs = args + (t['part'][:, :N],) + tuple(t['cot'][r, :N] for r in range(4)) + (t['zc'][0], t['zc'][1])
    b64, bld = kr.backward(*bargs), kr.backward(*bargs, dtype=np.longdouble)
    w = kr.work_split(t['work'], cap)
    for k in ('dAl', 'dS2', 'dP0', 'dP1', 'Kr0', 'Kr1'):
        r, c = b64[k][0].shape
        assert not np.any(w[k][r:]) and not np.any(w[k][:, c:]), '%s: %s is not zero beyond the latent\'s own grid' % (case, k)
        _rule('backward' + sfx, case, k, w[k][:r, :c], b64[k][0], bld[k][0], b64[k][1])


def _unpack(p, tag):
    return p['Z' + tag], [np.asarray(e, dtype=np.float64).reshape(-1) for e in p['ell_' + tag]], [float(np.squeeze(v)) for v in p['var_' + tag]]


BOUND_CASES = ['d21-12', 'd21-21', 'd11', 'd31', 'd21-mix2', 'd77', 'L32', 'L51', 'L77']


@pytest.mark.parametrize('name', BOUND_CASES)
def test_bound_tier_on_the_fixtures_of_kron_nd(engine, name):
    X, Y, p = kron_nd.problem(name)
    k = kron_nd.CASES[name]
    N, D = X.shape[0], k['D']
    grids = [k['f'], k['g'] or k['f']]
    out = engine.test_kron_fused_step(p, X, Y, jitter=kron_nd.JITTER, scale=kron_nd.case_scale(name))
    cap, nb = _check_facts(out['facts'], grids, N, 2)
    for h, tag in enumerate('fg'):
        Z, ell, var = _unpack(p, tag)
        _bound_latent('%s/%s' % (name, tag), cap == (1, 7), out['lat'][h], Z, ell, var, grids[h], D, X, N, cap)


@pytest.mark.parametrize('name,lik', [('d31', 'gaussian'), ('d21-21', 'bernoulli'), ('L32', 'bernoulli')])
def test_bound_tier_heads(engine, name, lik):
    X, Y, p = kron_nd.problem(name)
    k = kron_nd.CASES[name]
    y = Y if lik == 'gaussian' else (Y > 0).astype(np.float64)
    out = engine.test_kron_fused_step(kron_nd.head_params(p), X, y, lik=lik, jitter=kron_nd.JITTER, scale=kron_nd.case_scale(name), f_mu=0.3)
    cap, nb = _check_facts(out['facts'], [k['f']], X.shape[0], 1)
    Z, ell, var = _unpack(p, 'f')
    _bound_latent('%s/%s' % (name, lik), cap == (1, 7), out['lat'][0], Z, ell, var, k['f'], k['D'], X, X.shape[0], cap)


def test_bound_tier_at_the_illconditioned_pptr_init(engine):
    """the 32 x 32 grid at the precipitation init (cond(K_s) ~ 5e7, tests/test_gpu_pptr_params.py): a 1000-row minibatch"""
    from test_gpu_pptr_params import _pptr_params
    Xtr, Ytr, xb, yb, p = _pptr_params((32, 32))
    jit = 1e-5
    out = engine.test_kron_fused_step(p, xb, yb, jitter=jit, scale=Xtr.shape[0] / 1000.0)
    cap, nb = _check_facts(out['facts'], [(32, 32), (32, 32)], 1000, 2)
    for h, tag in enumerate('fg'):
        Z, ell, var = _unpack(p, tag)
        D = (Z[0].shape[1], Z[1].shape[1])
        ell = [np.full(D[q], ell[q][0]) if ell[q].size == 1 else ell[q] for q in range(2)]
        _bound_latent('pptr32/%s' % tag, False, out['lat'][h], Z, ell, var, (32, 32), D, xb, 1000, cap)


@pytest.mark.parametrize('name,N,settings', [('L51', 1025, (1024, 80, 24)), ('L32', 2100, (1024, 110, 40))])
def test_row_ranges_do_not_change_a_bit(engine, name, N, settings):
    """larger grids: the backward + accumulate launches go through the rows in ranges; 1, 2 and many ranges (a partial last one) give the
    same work block, ELBO and gradients bit for bit on ordinary (inexact) data"""
    X, Y, p = kron_nd.problem(name, N=N)
    ref, seen = None, []
    try:
        for tiles in settings:
            engine.set_kron_range_tiles(tiles)
            out = engine.test_kron_fused_step(p, X, Y, jitter=kron_nd.JITTER, scale=3.0)
            f = out['facts']
            seen.append(f['nranges'])
            assert tiles == 1024 or 0 < f['ntiles'] - (f['nranges'] - 1) * f['range_tiles'] < f['range_tiles']
            cur = [out['elbo_data'], out['kl']] + [out['lat'][h]['work'] for h in range(2)] + _flat(out['grads'])
            if ref is None:
                ref = cur
            for a, b in zip(ref, cur):
                assert np.array_equal(a, b), 'range tiles %d: a result differs from the single-range step' % tiles
    finally:
        engine.set_kron_range_tiles(1024)
    assert seen[0] == 1 and seen[1] == 2 and seen[2] >= 6, seen
    _log('ranges', '%s N=%d' % (name, N), 'bit-equal over %s ranges' % seen)


# =====================================================================================================================================
# the finish stage: k_kf_latent's KL scalars, k_kf_finish / k_kfl_finish<1..3> (Matern additions: tests/test_gpu_kron_matern_fused.py)
# =====================================================================================================================================
def finish_inputs(t, Z, s, M, cap, jitter):
    """the arguments of kronf_ref.finish from the taps of one latent (the stage's own inputs: work, K, P, U, S2, T0, T1, Al, zc) and the
    parameters Z, s"""
    w = kr.work_split(t['work'], cap)
    w = dict(dAl=w['dAl'][:M[0], :M[1]], dS2=w['dS2'][:M[0], :M[1]], dP0=w['dP0'][:M[0], :M[0]], dP1=w['dP1'][:M[1], :M[1]], Kr0=w['Kr0'][:M[0]], Kr1=w['Kr1'][:M[1]])
    K = [t['K'][q][:M[q], :M[q]] for q in range(2)]
    P = [t['P'][q][:M[q], :M[q]] for q in range(2)]
    m = lambda k: t[k][:M[0], :M[1]]
    return (w, K[0], K[1], P[0], P[1], m('U'), m('S2'), m('T0'), m('T1'), m('Al'), np.asarray(s, dtype=np.float64).reshape(M), Z[0], Z[1], t['zc'][0], t['zc'][1], jitter)


def assert_unwritten(case, t, M, D):
    """every finish-stage region at its capacity size: whatever lies outside the part the kernels write (include/zigp_diag.h) must come back
    as the stage sentinel the hook put there -- a kernel that wrote with a wrong row stride, or past its compact part, would show"""
    from zigp import _lib
    SENT = _lib.STAGE_SENTINEL
    Mq = (_rup(M[0], 16), _rup(M[1], 16))

    def rest(name, a, written):
        a = np.asarray(a)
        mask = np.ones(a.shape, dtype=bool)
        for sl in written:
            mask[sl] = False
        bad = a[mask] != SENT
        assert not bad.any(), '%s: %d elements of %s outside what the kernels write were written' % (case, int(bad.sum()), name)
        for sl in written:
            assert not np.any(a[sl] == SENT), '%s: an element of %s the kernels write still holds the sentinel' % (case, name)

    rest('klv', t['klv_cap'], [slice(0, 5)])
    for k in ('gu', 'gs'):
        rest(k, t[k + '_cap'], [slice(0, M[0] * M[1])])
    for k in ('krow', 'krow_first', 'krow2'):
        if k + '_cap' in t:
            for q in range(2):
                rest('%s[%d]' % (k, q), t[k + '_cap'][q], [slice(0, M[q] * (2 + 2 * D[q]))])
    if 'G_cap' in t:
        rest('G[0]', t['G_cap'][0], [(slice(0, Mq[0]), slice(0, Mq[0])), (slice(16, 16 + Mq[0]), slice(0, Mq[0]))])
        rest('G[1]', t['G_cap'][1], [(slice(0, Mq[1]), slice(0, Mq[1]))])


def check_G_and_krow_from_G(kernel, case, t, args, kl, f64, fld, M, krow_of=None):
    """larger grids: the G rows k_kfl_finish<3> leaves (factor 0: G itself, factor 1: P Q2 = P X P) under the rule, their padding rows and
    columns exact zeros, and krow recomputed from the TAPPED rows, so that stage 3's last lines are judged apart from the sandwich.
    krow_of(q, G, aG, dtype) -> (value, S) overrides the RBF form of those lines (Matern factors)."""
    w, K, P, Z, zc, jitter = args[0], args[1:3], args[3:5], args[11:13], args[13:15], args[15]
    Mq = (_rup(M[0], 16), _rup(M[1], 16))
    LD = np.longdouble
    worst = {}
    for q in range(2):
        Gt = t['G'][q][:Mq[q]]
        assert not np.any(Gt[M[q]:]) and not np.any(Gt[:, M[q]:]), '%s: rows / columns M .. Mq of the G region of factor %d' % (case, q)
        key = 'G0' if q == 0 else 'PXP1'
        worst[key] = _rule(kernel, case, key, Gt[:M[q], :M[q]], f64[key][0], fld[key][0], f64[key][1])
        coef = (0.5 * M[1 - q]) if kl else 0.0
        res = []
        for dt in (np.float64, LD):
            g = np.asarray(Gt[:M[q], :M[q]], dtype=dt)
            if q == 1:
                g = -g - dt(coef) * np.asarray(P[1], dtype=dt)
            ag = np.abs(g) if q == 0 else np.abs(np.asarray(Gt[:M[q], :M[q]], dtype=dt)) + dt(coef) * np.abs(np.asarray(P[1], dtype=dt))
            res.append(krow_of(q, g, ag, dt) if krow_of else kr.krow_from_G(g, ag, K[q], w['Kr%d' % q], Z[q], zc[q], jitter, dt))
        worst['krow%d|G' % q] = _rule(kernel, case, 'krow%d|G' % q, t['krow'][q], res[0][0], res[1][0], res[0][1])
    return worst


def check_finish(case, large, t, Z, s, M, D, cap, jitter, kl):
    """klv, krow0, krow1, gu, gs (larger grids: and G) of one latent of a tapped RBF step against kronf_ref in long double on the tapped inputs"""
    sfx = 'l' if large else ''
    Mq = (_rup(M[0], 16), _rup(M[1], 16))
    args = finish_inputs(t, Z, s, M, cap, jitter)
    d = [t['dvec'][q][:M[q]] for q in range(2)]
    k64, kld = kr.kl_scalars(args[5], args[9], args[10], d[0], d[1]), kr.kl_scalars(args[5], args[9], args[10], d[0], d[1], dtype=np.longdouble)
    worst = {}
    for i, k in enumerate(('uAl', 'logs2', 'ds2')):
        worst['klv%d' % i] = _rule('latent' + sfx, case, 'klv%d' % i, t['klv'][i:i + 1], np.reshape(k64[k][0], 1), np.reshape(kld[k][0], 1), np.reshape(k64[k][1], 1))
    assert t['klv'][3] == t['dvec'][0][Mq[0]] and t['klv'][4] == t['dvec'][1][Mq[1]], '%s: klv[3], klv[4] are not the factor kernel\'s logdets' % case
    f64, fld = kr.finish(*args, kl), kr.finish(*args, kl, dtype=np.longdouble)
    for k in ('krow0', 'krow1', 'gu', 'gs'):
        worst[k] = _rule('finish' + sfx, case, k, t[k[:4]][int(k[4])] if k.startswith('krow') else t[k], f64[k][0], fld[k][0], f64[k][1])
    for q in range(2):
        assert t['krow'][q].shape == (M[q], 2 + 2 * D[q]) and not np.any(t['krow'][q][:, 1 + 2 * D[q]]), '%s: krow column 1 + 2 D of factor %d is not exact 0' % (case, q)
    if large:
        worst.update(check_G_and_krow_from_G('finish' + sfx, case, t, args, kl, f64, fld, M))
    else:
        assert 'G' not in t
    assert_unwritten(case, t, M, D)
    return worst


def _finish_case(engine, tag, p, X, Y, grids, D, lik='onoff', jitter=kron_nd.JITTER, scale=1.0, f_mu=0.0):
    two = lik == 'onoff'
    for kl in (True, False):
        out = engine.test_kron_fused_step(p, X, Y, lik=lik, jitter=jitter, scale=scale, f_mu=f_mu, include_kl=kl)
        cap, nb = _check_facts(out['facts'], grids, X.shape[0], len(grids))
        assert out['kl'] == 0.0 or kl
        for h, lt in enumerate('fg' if two else 'f'):
            Z = p['Z' + lt]
            check_finish('%s/%s kl=%d' % (tag, lt if two else lik, kl), cap == (1, 7), out['lat'][h], Z, p['u_%ss_sqrt' % lt], grids[h], D, cap, jitter, kl)


@pytest.mark.parametrize('name', BOUND_CASES)
def test_finish_bound_tier_on_the_fixtures_of_kron_nd(engine, name):
    X, Y, p = kron_nd.problem(name)
    k = kron_nd.CASES[name]
    _finish_case(engine, name, p, X, Y, [k['f'], k['g'] or k['f']], k['D'], scale=kron_nd.case_scale(name))


@pytest.mark.parametrize('name,lik', [('d31', 'gaussian'), ('d21-21', 'bernoulli'), ('L32', 'bernoulli')])
def test_finish_bound_tier_heads(engine, name, lik):
    X, Y, p = kron_nd.problem(name)
    k = kron_nd.CASES[name]
    y = Y if lik == 'gaussian' else (Y > 0).astype(np.float64)
    _finish_case(engine, name, kron_nd.head_params(p), X, y, [k['f']], k['D'], lik=lik, scale=kron_nd.case_scale(name), f_mu=0.3)


def test_finish_bound_tier_at_the_illconditioned_pptr_init(engine):
    from test_gpu_pptr_params import _pptr_params
    Xtr, Ytr, xb, yb, p = _pptr_params((32, 32))
    D = (p['Zf'][0].shape[1], p['Zf'][1].shape[1])
    _finish_case(engine, 'pptr32', p, xb, yb, [(32, 32), (32, 32)], D, jitter=1e-5, scale=Xtr.shape[0] / 1000.0)


# ---- edges: N = 33; the smallest grid the entry point accepts is ONE point per factor (validate_kron refuses M <= 0 only), so (1, 1) and
# (1, 112) stand where a refusal would have asked for 2.  The problems are kron_nd.edge_problem (lengthscale
# constant kron_nd.EDGE_C); tests/test_cpu_kronf_finish_ref.py shows that every mutation of the stage is caught on these very problems.
def _edge_cases():
    return [(g, D) for g in kron_nd.EDGE_GRIDS for D in kron_nd.EDGE_DS]


@pytest.mark.parametrize('grid,D', _edge_cases(), ids=lambda v: 'x'.join(map(str, v)))
def test_finish_edges(engine, grid, D):
    X, Y, p = kron_nd.edge_problem(grid, D)
    _finish_case(engine, 'edge%dx%d D%d%d' % (grid + D), p, X, Y, [grid, grid], D, scale=7.0)


@pytest.mark.parametrize('shape', ['mix', 'under', 'Lrmix'])
def test_finish_edges_two_latents_with_different_grids_and_a_head(engine, shape):
    gf, gg = SHAPES[shape]
    for D in ((1, 1), (7, 7)):
        X, Y, p = kron_nd.edge_problem(gf, D, gg)
        _finish_case(engine, 'edge-%s D%d%d' % ((shape,) + D), p, X, Y, [gf, gg], D, scale=7.0)
    _finish_case(engine, 'edge-%s head' % shape, kron_nd.head_params(p), X, Y, [gf], D, lik='gaussian', scale=7.0, f_mu=0.1)


def test_a_grid_without_points_is_refused(engine):
    X, Y, p = kron_nd.problem('d21-12')
    q = dict(p)
    q['Zf'] = [p['Zf'][0][:0], p['Zf'][1]]
    q['u_fm'], q['u_fs_sqrt'] = p['u_fm'][:0], p['u_fs_sqrt'][:0]
    with pytest.raises(ValueError):
        engine.test_kron_fused_step(q, X, Y)


@pytest.mark.parametrize('name', ['d31', 'd77', 'L32'])
def test_returned_gradients_are_the_host_chain_rule_of_the_tapped_results(engine, name):
    """kron_assemble_grads: the gradients a tapped step returns against kronf_ref.assemble of the tapped krow, gu, gs -- host double arithmetic,
    a few operations per element: 16 eps S."""
    X, Y, p = kron_nd.problem(name)
    out = engine.test_kron_fused_step(p, X, Y, jitter=kron_nd.JITTER, scale=kron_nd.case_scale(name))
    check_assemble(name, out, p, 'fg')


def check_assemble(case, out, p, tags):
    g = out['grads']
    for h, tag in enumerate(tags):
        t = out['lat'][h]
        Z, ell, var = _unpack(p, tag)
        s_gv = np.sum(np.asarray(t['cot'][1], dtype=np.longdouble))
        a64 = kr.assemble(t['krow'], t['gu'], t['gs'], ell, var, float(s_gv))
        ald = kr.assemble(t['krow'], t['gu'], t['gs'], ell, var, s_gv, dtype=np.longdouble)
        pairs = [('u', g['u_%sm' % tag].reshape(t['gu'].shape), 0.0), ('s', g['u_%ss_sqrt' % tag].reshape(t['gs'].shape), 0.0)]
        for q in range(2):
            # the variance cotangents are summed over the points on the device in another order than here: their sum enters with the sum of
            # their absolute values
            sv = float(np.sum(np.abs(t['cot'][1]))) * var[1 - q]
            pairs += [('Z%d' % q, g['Z' + tag][q], 0.0), ('ell%d' % q, g['ell_' + tag][q].reshape(-1), 0.0), ('var%d' % q, np.reshape(g['var_' + tag][q], 1), sv)]
        worst = 0.0
        for k, got, extra in pairs:
            want, S = (ald[k[:-1]][int(k[-1])] if k[-1] in '01' else ald[k])
            S64 = np.asarray(a64[k[:-1]][int(k[-1])][1] if k[-1] in '01' else a64[k][1], dtype=np.float64)
            S64 = np.reshape(S64, np.shape(got)) + extra
            err = np.asarray(np.abs(np.asarray(got, dtype=np.longdouble) - np.reshape(want, np.shape(got))), dtype=np.float64)
            live = S64 > 0
            r = float(np.max(err[live] / S64[live] / EPS)) if live.any() else 0.0
            worst = max(worst, r)
            assert np.all(err <= 16 * EPS * S64), '%s/%s: d %s is not the chain rule of the tapped results: err / (eps S) = %.2f' % (case, tag, k, r)
        _log('assemble', '%s/%s' % (case, tag), 'max err / (eps S) = %.3f' % worst)


# =====================================================================================================================================
# hook hygiene
# =====================================================================================================================================
def _flat(g):
    out = []
    for k in sorted(g):
        v = g[k]
        out += [np.asarray(a) for a in v] if isinstance(v, list) else [np.asarray(v)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name,lik', [('d21-mix', 'onoff'), ('L51', 'onoff'), ('d31', 'gaussian')])
def test_hook_returns_the_bits_of_an_ordinary_call(engine, name, lik):
    X, Y, p = kron_nd.problem(name)
    kw = dict(jitter=kron_nd.JITTER, scale=kron_nd.case_scale(name))
    if lik == 'onoff':
        plain = lambda: engine.kron_elbo(p, X, Y, f_mu=0.2, g_offset=0.1, **kw)
        tapped = lambda **o: engine.test_kron_fused_step(p, X, Y, f_mu=0.2, g_offset=0.1, **kw, **o)
    else:
        ph = kron_nd.head_params(p)
        plain = lambda: engine.kron_head_elbo(ph, X, Y, lik=lik, f_mu=0.2, **kw)
        tapped = lambda **o: engine.test_kron_fused_step(ph, X, Y, lik=lik, f_mu=0.2, **kw, **o)
    ed0, kl0, g0 = plain()
    t1 = tapped()
    assert (t1['elbo_data'], t1['kl']) == (ed0, kl0) and _same(_flat(t1['grads']), _flat(g0)), 'the tapped step is not the ordinary step'
    t2 = tapped()
    for h, lat in enumerate(t1['lat']):
        for k, v in lat.items():
            vs, ws = (v, t2['lat'][h][k]) if isinstance(v, list) else ([v], [t2['lat'][h][k]])
            if k == 'K':                       # beyond the leading R x R part, R = M_p rounded up to 32, the buffer is never written
                Rs = [_rup(P.shape[0], 32) for P in lat['P']]
                vs, ws = [a[:R, :R] for a, R in zip(vs, Rs)], [a[:R, :R] for a, R in zip(ws, Rs)]
            assert _same(vs, ws), 'tap %s of latent %d differs between two tapped calls' % (k, h)
    assert t1['facts'] == t2['facts']
    t3 = tapped(taps=False)
    assert (t3['elbo_data'], t3['kl']) == (ed0, kl0) and _same(_flat(t3['grads']), _flat(g0))
    ed1, kl1, g1 = plain()
    assert (ed1, kl1) == (ed0, kl0) and _same(_flat(g1), _flat(g0)), 'an ordinary call after the tapped ones changed'
    if lik == 'onoff':
        engine.set_kron_panels(True)
        try:
            pa = engine.kron_elbo(p, X, Y, **kw)
            with pytest.raises(ValueError):
                tapped()                       # a fused-eligible grid forced onto the panels: ZIGP_EARG
            pb = engine.kron_elbo(p, X, Y, **kw)
        finally:
            engine.set_kron_panels(False)
        assert pa[:2] == pb[:2] and _same(_flat(pa[2]), _flat(pb[2])), 'the panel path changed after a refused tapped call'
        ed2, kl2, g2 = plain()
        assert (ed2, kl2) == (ed0, kl0) and _same(_flat(g2), _flat(g0))
    _log('hook', '%s %s' % (name, lik), 'tapped == ordinary, taps repeat, later calls unchanged')


def test_hook_argument_errors_leave_the_context_usable(engine):
    from zigp import _lib
    lib = engine.lib
    assert lib.zigp_test_kron_fused_step(None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_kron_fused_step(engine.ctx, None) == _lib.ZIGP_EARG
    s = _lib.zigp_stage_kron_fused()
    assert lib.zigp_test_kron_fused_step(engine.ctx, C.byref(s)) == _lib.ZIGP_EARG          # no parameters
    X, Y, p = kron_nd.problem('d21-12')
    with pytest.raises(ValueError):
        engine.test_kron_fused_step(p, X[:0], Y[:0])                                         # N = 0
    with pytest.raises(ValueError):
        engine.test_kron_fused_step(p, X, Y, jitter=-1.0)
    for beyond in ('p43', 'p81'):                                                            # panels because of size / of D
        Xp, Yp, pp = kron_nd.problem(beyond)
        with pytest.raises(ValueError):
            engine.test_kron_fused_step(pp, Xp, Yp)
    a = engine.kron_elbo(p, X, Y, jitter=kron_nd.JITTER)
    out = engine.test_kron_fused_step(p, X, Y, jitter=kron_nd.JITTER)
    assert (out['elbo_data'], out['kl']) == a[:2]
