"""Stage-level parity of the blocked Cholesky and its inverse (potrf_trtri_jobs, csrc/zigp_host.h): every launch of the chain that opens a
dense call -- and the Kronecker panel path and the sample-path weight stages -- through zigp_test_potrf_stages, which runs ONE job through
potrf_trtri_jobs itself and copies the images right behind each launch.  tests/potrf_ref.py states the chain, the families, the bars and
the derivation of C; tests/test_cpu_potrf_ref.py proves on the CPU that the reference alone is inside every bar and that every deliberate
mistake is >= 1e3 outside one.

EXACT TIER: the exact family must come back bit for bit -- L0, W0, identity padding, exact +0 above the diagonal -- at every size that takes
another path: npan 1 .. 4, nb 2, 3 (the ragged doubling level), 5, 9, 12 and 16, where the split-K trailing updates run at S = 4, 4, 5, 6, 7
(asserted from the hook's facts against the restated plan).  Up to n = 640 every snapshot equals the integer restatement.
BOUND TIER: (a) RBF Kuu at cond ~ 1e4 and 1e7 .. 1e9, (b) B B^T + I, (c) (a) scaled by D = 2^-14 .. 2^14, every snapshot per launch under
err_gpu <= 4 err_np + 16 EPS S (products) and the component-wise bars of the diagonal kernel's levels; one end-to-end run at n = 1024.
STAGE-LOG lines carry the largest err / bar per launch kind beside the same figure of the float64 NumPy emulation of the block algorithm."""
import numpy as np
import pytest

import potrf_ref as R

pytestmark = pytest.mark.gpu

EXACT_SIZES = (1, 16, 17, 31, 32, 33, 96, 97, 128, 129, 200, 300, 640, 1100, 1500, 2048, 1930)
PIVOTS = (1, 16, 17, 32, 33, 96, 97, 128, 129, 273, 300)


def _images_ok(run, n):
    """identity padding, exact +0 above the diagonal of L and W"""
    Mp = run['Mp']
    for X in (run['L'], run['W']):
        up = np.triu(X, 1)
        assert np.array_equal(up, np.zeros((Mp, Mp))) and not np.any(np.signbit(up))
        assert np.array_equal(X[n:, n:], np.eye(Mp - n)) and not X[n:, :n].any()


def _T_mask(run):
    """elements of T some tri1 launch wrote"""
    m = np.zeros((run['Mp'], run['Mp']), dtype=bool)
    for l in run['launches']:
        if l['kind'] == 'tri1':
            for bi, bj, _, _ in R.tiles_of('tri1', l['idx'], run['nb']):
                m[bi * 128:(bi + 1) * 128, bj * 128:(bj + 1) * 128] = True
    return m


@pytest.mark.parametrize('n', EXACT_SIZES)
def test_exact_family_bit_for_bit(engine, n):
    seeds = (0, 1) if n <= 640 else (EXACT_SIZES.index(n) % 2,)
    for seed in seeds:
        A, L0, W0 = R.exact_family(n, seed)
        for sk in (False, True):
            snaps = n <= 640
            run = engine.test_potrf_stages(A, split_k=sk, snapshots=snaps)
            assert run['info'] == 0 and run['Mp'] == -(-n // 128) * 128
            assert R.facts_of(run) == R.plan(n, sk), (n, sk)
            assert np.array_equal(run['L'][:n, :n], L0), (n, seed, sk, 'L')
            assert np.array_equal(run['W'][:n, :n], W0), (n, seed, sk, 'W')
            _images_ok(run, n)
            assert np.all(run['T'][~_T_mask(run)] == R.SENTINEL) and not np.any(run['T'][_T_mask(run)] == R.SENTINEL)
            if snaps:
                assert R.check_final(run)
                for name, (v, S, mask) in R.restate(run, A).items():
                    assert np.array_equal(v, R.tap_of(run, name)), (n, seed, sk, name)
                for l in run['launches']:
                    if l['kind'] == 'diag':
                        j = l['idx']
                        s = slice(j * 128, min(n, (j + 1) * 128))
                        assert np.array_equal(l['snap'][0][s, s], L0[s, s]) and np.array_equal(l['snap'][1][s, s], W0[s, s]), (n, seed, sk, j)
                assert max(R.worst(R.check_diags(run, A)).values()) == 0.0      # (a ragged panel is identity-padded: still exact)


def test_planned_slice_counts_are_the_restated_ones(engine):
    """nb = 16 is the only size of the tier where S != 8: the trailing updates of j = 0 .. 4 run at 4, 4, 5, 6, 7 (uneven slices of 8 k-steps)"""
    seen = set()
    for n in (2048, 1930):
        run = engine.test_potrf_stages(R.exact_family(n, 0)[0], split_k=True, snapshots=False)
        assert [l['S'] for l in run['launches'] if l['kind'] == 'trail'][:6] == [4, 4, 5, 6, 7, 8]
        seen |= {l['S'] for l in run['launches'] if l['kind'] != 'diag'}
    assert seen == {4, 5, 6, 7, 8}
    for n in (129, 640, 1100, 1408):
        run = engine.test_potrf_stages(R.exact_family(n, 0)[0], split_k=True, snapshots=False)
        assert {l['S'] for l in run['launches'] if l['kind'] != 'diag'} == {8}, n
    run = engine.test_potrf_stages(R.exact_family(1500, 0)[0], split_k=True, snapshots=False)
    assert [l['S'] for l in run['launches'] if l['kind'] == 'trail'][:2] == [7, 8]
    assert all(l['S'] == 0 for l in engine.test_potrf_stages(R.exact_family(300, 0)[0], split_k=False, snapshots=False)['launches'])


def _log(tag, w_gpu, w_np):
    for k in sorted(w_gpu):
        print('STAGE-LOG %-12s %-40s max error / bound = %.4g   (NumPy emulation: %s)'
              % ('potrf', '%s %s' % (tag, k), w_gpu[k], '%.4g' % w_np[k] if k in w_np else 'the bar\'s own err_np'))


def _panel_cost(run, A):
    """Not gated.  The panel step multiplies by W_jj^T where a triangular solve X L_jj^T = A[bi][j] would do, and a solve's result satisfies
    |X^ L_jj^T - A[bi][j]| <= 128 EPS |X^| |L_jj^T|.  Returns the largest |L^[bi][j] L^_jj^T - A[bi][j]| / (128 EPS |L^[bi][j]| |L^_jj^T|) over the
    run's panel launches: the product's result in units of the backward-error bar of the solve it replaces."""
    st = R.states(run, A)
    worst = 0.0
    for k, l in enumerate(run['launches']):
        if l['kind'] != 'panel':
            continue
        s = slice(l['idx'] * 128, (l['idx'] + 1) * 128)
        Lb, La = st[k][0], l['snap'][0]
        Ljj = np.tril(Lb[s, s])
        for bi in range(l['idx'] + 1, run['nb']):
            r = slice(bi * 128, (bi + 1) * 128)
            res = np.abs(La[r, s].astype(R.LD) @ Ljj.T.astype(R.LD) - Lb[r, s].astype(R.LD))
            worst = max(worst, R.ratio(res, 128 * R.EPS * (np.abs(La[r, s]) @ np.abs(Ljj).T)))
    return worst


@pytest.mark.parametrize('n', [200, 300, 520])
@pytest.mark.parametrize('fam', R.FAMILIES)
def test_every_launch_within_its_bar(engine, fam, n):
    A = R.family(fam, n)
    for sk in (False, True):
        run = engine.test_potrf_stages(A, split_k=sk)
        assert run['info'] == 0 and R.facts_of(run) == R.plan(n, sk)
        _images_ok(run, n)
        assert R.check_final(run)
        w = R.worst(R.check_diags(run, A), R.check_products(run, A))
        emu = R.emulate(A, split_k=sk)
        w_np = R.worst(R.check_diags(emu, A))
        _log('%s n=%d sk=%d' % (fam, n, sk), w, w_np)
        if n > 128:
            print('STAGE-LOG %-12s %-40s panel result / bar of the solve it replaces = %.4g'
                  % ('potrf', '%s n=%d sk=%d' % (fam, n, sk), _panel_cost(run, A)))
        assert max(w_np.values()) <= 1.0
        assert max(w.values()) <= 1.0, (fam, n, sk, w)


def test_end_to_end_1024_production_regime(engine):
    """family (a) at cond >= 1e7, the split-K chain of a dense call at nb = 8: the levels of all eight diagonal launches and the final
    doubling level (b = 4: 16 tiles of 1 .. 4 blocks of k) per element; the whole result against the long-double inverse residual"""
    n = 1024
    A = R.family('a_high', n)
    run = engine.test_potrf_stages(A, split_k=True)
    assert run['info'] == 0 and R.facts_of(run) == R.plan(n, True)
    _images_ok(run, n)
    assert R.check_final(run)
    only = {'tri1:4', 'tri2:4'}
    w = R.worst(R.check_diags(run, A), R.check_products(run, A, only=only))
    emu = R.emulate(A, split_k=True)
    w_np = R.worst(R.check_diags(emu, A))
    _log('a_high n=1024 sk=1', w, w_np)
    print('STAGE-LOG %-12s %-40s panel result / bar of the solve it replaces = %.4g' % ('potrf', 'a_high n=1024 sk=1', _panel_cost(run, A)))
    assert set(w) == {'diag.pad', 'diag.factor', 'diag.inv16', 'diag.couple', 'diag.dist', 'tri1', 'tri2'}
    assert max(w_np.values()) <= 1.0
    assert max(w.values()) <= 1.0, w


def test_two_jobs_at_once_equal_the_single_job(engine):
    """the dense M x M forward runs both latents' chains alternating on two streams, on `prepared` buffers, with split-K: L and W of each
    latent must be the bits of the hook's single split-K job on the Kuu that call built"""
    from conftest import make_problem
    _, _, p = make_problem(8, 200, 3, seed=11, Mg=520, ell=0.1)
    outs = engine.test_latents_forward(p, 1e-4, False)
    for h, M in enumerate((200, 520)):
        o = outs[h]
        run = engine.test_potrf_stages(o['Kuu'], split_k=True, snapshots=False)
        assert np.array_equal(run['L'][:M, :M], o['L']), h
        assert np.array_equal(run['W'][:M, :M], o['W']), h


# ---- failure reporting: ordinary refused inputs (a pivot that is not > 0), as tests/test_gpu_blocks.py::test_potrf_not_pd exercises ----
@pytest.fixture(scope='module')
def good300():
    """the good call on a FRESH engine: what the session's engine must return after every refused one"""
    import zigp
    A = R.exact_family(300, 1)[0]
    e = zigp.DenseEngine(0)
    try:
        out = {sk: e.test_potrf_stages(A, split_k=sk, snapshots=False) for sk in (False, True)}
    finally:
        e.close()
    return A, out


def _refused(engine, A, sk, p, good300):
    import zigp
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        engine.test_potrf_stages(A, split_k=sk, snapshots=False)
    assert int(engine.lib.zigp_last_info(engine.ctx)) == p, (p, sk)
    assert ei.value.stages['info'] == p and R.facts_of(ei.value.stages) == R.plan(A.shape[0], sk)
    Ag, ref = good300
    again = engine.test_potrf_stages(Ag, split_k=sk, snapshots=False)
    for k in ('L', 'W', 'T'):
        assert np.array_equal(again[k], ref[sk][k]), (p, sk, k)


@pytest.mark.parametrize('value', [0.0, -1.0])
def test_failure_index_at_every_boundary(engine, good300, value):
    for p in PIVOTS:
        A = R.exact_with_pivot(300, p, value)
        for sk in (False, True):
            _refused(engine, A, sk, p, good300)


def test_failure_index_first_of_two_nan_and_tiny_pivot(engine, good300):
    for p, q in ((5, 20), (20, 40), (100, 273)):       # the same 32-panel in different halves; different panels; different 128-blocks
        A = R.exact_with_pivot(300, p, -1.0)
        A[q - 1, q - 1] = -1.0
        for sk in (False, True):
            _refused(engine, A, sk, p, good300)
    for p in (97, 129):
        A = R.exact_family(300, 0)[0].copy()
        A[p - 1, p - 1] = np.nan
        for sk in (False, True):
            _refused(engine, A, sk, p, good300)
    A = R.exact_with_pivot(300, 300, 2.0 ** -40)
    _, L0, _ = R.exact_family(300, 0)
    for sk in (False, True):
        run = engine.test_potrf_stages(A, split_k=sk, snapshots=False)
        assert run['info'] == 0 and run['L'][299, 299] == 2.0 ** -20
        assert np.array_equal(run['L'][:299, :299], L0[:299, :299]) and np.array_equal(run['L'][299, :299], L0[299, :299])


def test_failed_call_still_returns_its_snapshots(engine):
    import zigp
    A = R.exact_with_pivot(300, 129, 0.0)
    with pytest.raises(zigp.NotPositiveDefiniteError) as ei:
        engine.test_potrf_stages(A, split_k=True)
    run = ei.value.stages
    assert run['info'] == 129 and len(run['launches']) == len(R.plan(300, True)) and all(len(l['snap']) for l in run['launches'])
    _, L0, W0 = R.exact_family(300, 0)
    first = run['launches'][0]['snap']
    assert np.array_equal(first[0][:128, :128], L0[:128, :128]) and np.array_equal(first[1][:128, :128], W0[:128, :128])
    # the failing diagonal kernel writes nothing: its block is what the trailing update left
    k = [i for i, l in enumerate(run['launches']) if l['kind'] == 'diag' and l['idx'] == 1][0]
    before = run['launches'][k - 1]['snap'][0]
    assert np.array_equal(run['launches'][k]['snap'][0], before)


# ---- hook manners ----
def test_argument_errors_leave_the_context_usable(engine):
    import ctypes as C
    from zigp import _lib
    A = R.exact_family(130, 0)[0]
    good = engine.test_potrf_stages(A, split_k=True, snapshots=False)
    with pytest.raises(ValueError):
        engine.test_potrf_stages(np.zeros((0, 0)))
    with pytest.raises(ValueError):
        engine.test_potrf_stages(np.zeros((3, 4)))
    facts = np.zeros(_lib.PSF_REC + _lib.PSF_PER * 6, dtype=np.int64)
    snap = np.zeros((8, 256, 256))
    Ac = np.ascontiguousarray(A)
    base = dict(n=130, split_k=1, A=_lib.ptr(Ac), facts=facts.ctypes.data_as(C.POINTER(C.c_int64)), facts_cap=facts.size, snap=_lib.ptr(snap), snap_cap=8)
    for bad in (dict(A=None), dict(n=0), dict(n=-5), dict(n=4097), dict(facts_cap=facts.size - 1), dict(snap_cap=7)):
        a = _lib.zigp_stage_potrf(**dict(base, **bad))
        assert engine.lib.zigp_test_potrf_stages(engine.ctx, C.byref(a)) == _lib.ZIGP_EARG, bad
    a = _lib.zigp_stage_potrf(**base)
    assert engine.lib.zigp_test_potrf_stages(engine.ctx, C.byref(a)) == 0 and facts[2] == 6 and facts[3] == 8
    again = engine.test_potrf_stages(A, split_k=True, snapshots=False)
    for k in ('L', 'W', 'T'):
        assert np.array_equal(good[k], again[k])


def test_gradient_call_has_identical_bits_around_a_tapped_call(engine):
    from conftest import make_problem
    X, Y, p = make_problem(2000, 96, 3, seed=7)
    engine.set_data(X, Y)
    first = engine.elbo(p, jitter=1e-6)
    engine.test_potrf_stages(R.family('b', 300), split_k=True)
    engine.test_potrf_stages(R.exact_family(200, 0)[0], split_k=False)
    second = engine.elbo(p, jitter=1e-6)
    assert first[0] == second[0] and first[1] == second[1]
    for k in first[2]:
        assert np.array_equal(np.asarray(first[2][k]), np.asarray(second[2][k])), k
