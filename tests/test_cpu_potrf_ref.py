"""CPU-side proof of tests/potrf_ref.py, the per-launch restatement of the blocked Cholesky and its inverse that
tests/test_gpu_potrf_stages.py holds the GPU against:

  * the families have the properties the GPU tiers rely on (the exact family is exact; the cond ranges of the bound families are pinned);
  * THE REFERENCE ALONE stays within every bar: LAPACK's factor and inverse, and the float64 NumPy emulation of the block algorithm, go
    through the checkers the GPU's images go through.  A bar or a family that fails here is wrong here;
  * every deliberate mistake (potrf_ref.MUTATIONS, the _mut idiom of tests/test_cpu_kronp_ref.py) leaves at least one bar by >= 1e3;
  * the restated slice rule, and the failure index against LAPACK's info."""
import numpy as np
import pytest
from scipy.linalg import lapack

import potrf_ref as R

SIZES_EXACT = (33, 300, 1100, 2048)
PIVOTS = (1, 16, 17, 32, 33, 96, 97, 128, 129, 273, 300)


@pytest.mark.parametrize('seed', [0, 1])
def test_exact_family_is_exact(seed):
    for n in SIZES_EXACT:
        A, L0, W0 = R.exact_family(n, seed)
        assert np.abs(A).max() <= 10937 and np.abs(W0).max() <= 1024
        for X in (A, L0, W0):          # small dyadic numbers: multiples of 1/4 (1/2 for W0: N and N^2 are integer, 1 / d in {1/2, 1, 2})
            assert np.array_equal(X * 4, np.round(X * 4))
        assert set(np.unique(np.diag(L0))) == {0.5, 1.0, 2.0}
        assert np.array_equal(W0 @ L0, np.eye(n)) and np.array_equal(L0 @ W0, np.eye(n))
        assert np.array_equal(np.linalg.cholesky(A), L0)
        # every partial sum of every product of the chain is exact: the sums of absolute terms stay far below 2^53 quarters
        assert n * np.abs(L0).max() * np.abs(W0).max() * 16 < 2.0 ** 53 and n * np.abs(L0).max() ** 2 * 16 < 2.0 ** 53
    a, b = R.exact_family(300, 0)[1], R.exact_family(300, 1)[1]
    assert np.mean((a != 0) != (b != 0)) > 0.02          # the second seed moves the zeros


def test_exact_family_without_period():
    _, L0, _ = R.exact_family(520, 0)
    d = np.diag(L0)
    for p in (1, 2, 3, 4, 8, 16, 32, 64, 128):
        assert not np.array_equal(d[p:], d[:-p])
        assert not np.array_equal(L0[2 * p:, p:-p], L0[p:-p, :-2 * p])


def _cond(A):
    e = np.linalg.eigvalsh(A)
    return e[-1] / e[0]


def test_cond_ranges_are_pinned():
    for n in (200, 300, 520):
        assert R.COND_MID[0] <= _cond(R.family('a_mid', n)) <= R.COND_MID[1]
        assert R.COND_B[0] <= _cond(R.family('b', n)) <= R.COND_B[1]
    for n in (200, 300, 520, 1024):
        assert R.COND_HIGH[0] <= _cond(R.family('a_high', n)) <= R.COND_HIGH[1]
    assert _cond(R.family('a_high', 1024)) >= 1e7
    for n in (200, 520):      # (c): a diagonal scaling over 8 decades of the high member; scaled back it is that member
        D = R.graded_scale(n)
        assert D.min() <= 1e-4 and D.max() >= 1e4 and not np.array_equal(D, np.sort(D))
        assert np.array_equal(R.family('c', n) / D[:, None] / D[None, :], R.family('a_high', n))


@pytest.fixture(scope='module')
def runs():
    """emulated split-K runs of every bound family at n = 300 (nb = 3: a ragged doubling level and a ragged last block), shared"""
    return {f: (R.family(f, 300), R.emulate(R.family(f, 300), split_k=True)) for f in R.FAMILIES}


def test_slice_rule():
    for nb in range(1, 12):
        assert {l['S'] for l in R.plan(nb * 128, True) if l['kind'] != 'diag'} <= {8}
    p16 = R.plan(2048, True)
    assert [l['S'] for l in p16 if l['kind'] == 'trail'][:6] == [4, 4, 5, 6, 7, 8]
    assert {l['S'] for l in p16 if l['kind'] != 'diag'} == {4, 5, 6, 7, 8}
    assert {l['S'] for l in R.plan(1930, True) if l['kind'] != 'diag'} == {4, 5, 6, 7, 8}
    assert all(l['S'] == 0 for l in R.plan(2048, False))
    assert [l['npan'] for l in R.plan(300, True) if l['kind'] == 'diag'] == [4, 4, 2]
    assert [R.plan(n, True)[0]['npan'] for n in (1, 16, 17, 31, 32, 33, 96, 97, 128)] == [1, 1, 1, 1, 1, 2, 3, 4, 4]
    # every launch writes each of its tiles once, in the lower block triangle
    for nb in (2, 3, 5, 9, 16):
        for l in R.plan(nb * 128, True):
            if l['kind'] != 'diag':
                t = [(bi, bj) for bi, bj, _, _ in R.tiles_of(l['kind'], l['idx'], nb)]
                assert len(set(t)) == len(t) == l['tiles'] and all(bi >= bj for bi, bj in t)
    # recursive doubling covers every strictly-lower block exactly once
    for nb in (2, 3, 5, 9, 12, 16):
        t = [(bi, bj) for l in R.plan(nb * 128, True) if l['kind'] == 'tri2' for bi, bj, _, _ in R.tiles_of('tri2', l['idx'], nb)]
        assert sorted(t) == [(bi, bj) for bi in range(nb) for bj in range(bi)]


def test_emulation_is_the_factorisation(runs):
    for f, (A, run) in runs.items():
        n = A.shape[0]
        L, W = run['L'][:n, :n], run['W'][:n, :n]
        assert np.max(np.abs(L @ L.T - A)) <= 1e-13 * np.abs(A).max() * n, f
        assert np.max(np.abs(W.astype(R.LD) @ L.astype(R.LD) - np.eye(n))) <= 1e-9 * max(1.0, _cond(A) * 1e-6) * 1e3, f
        assert np.array_equal(run['L'][n:, n:], np.eye(run['Mp'] - n)) and np.array_equal(run['W'][n:, n:], np.eye(run['Mp'] - n))
        assert not run['L'][n:, :n].any() and not run['W'][n:, :n].any()
        assert R.check_final(run) and R.facts_of(run) == R.plan(n, True)
    A, L0, W0 = R.exact_family(300, 0)
    for sk in (False, True):
        run = R.emulate(A, split_k=sk)
        assert np.array_equal(run['L'][:300, :300], L0) and np.array_equal(run['W'][:300, :300], W0) and R.check_final(run)
        for name, (v, S, mask) in R.restate(run, A).items():
            assert np.array_equal(v, R.tap_of(run, name)), name


def test_reference_alone_is_within_every_bar(runs):
    """the float64 emulation through every checker; restated with ANOTHER slice count than it ran with (one product per tile), so that the
    product bars are asked to hold across summation orders, as they are on the GPU"""
    for f, (A, run) in runs.items():
        d = R.check_diags(run, A)
        other = dict(run, launches=[dict(l, S=0) for l in run['launches']])
        p = R.check_products(other, A)
        w = R.worst(d, p)
        print('REF-LOG emulation %-7s %s' % (f, '  '.join('%s %.3g' % kv for kv in sorted(w.items()))))
        assert set(w) == {'diag.pad', 'diag.factor', 'diag.inv16', 'diag.couple', 'diag.dist', 'panel', 'trail', 'tri1', 'tri2'}
        assert max(w.values()) <= 1.0, (f, w)


def test_lapack_alone_is_within_the_diagonal_bars():
    """LAPACK's dpotrf / dtrtri on 128 x 128 blocks (and ragged ones) of every family through the checks of the diagonal kernel that are
    backward-error bounds of ANY factorisation / substitution: the factor residual, the 16 x 16 left residual (diagonal blocks of a triangular
    inverse are the inverses of the diagonal blocks) and the padding.  The coupling and distance bars restate THIS algorithm's products --
    dtrtri does not form W21 as -W22 (L21 W11) -- so they are printed for LAPACK and asserted for the emulation only."""
    for f in R.FAMILIES:
        A = R.family(f, 300)
        for lo, npan in ((0, 4), (128, 4), (256, 2)):
            blk = R.padded(A)[lo:lo + 128, lo:lo + 128]
            if lo:      # a Schur complement, as the chain hands it to the kernel
                L0 = np.linalg.cholesky(A)[:, :lo]
                S = R.padded(A)
                S[:300, :300] -= L0 @ L0.T
                blk = S[lo:lo + 128, lo:lo + 128]
            L = np.linalg.cholesky(blk)
            W, info = lapack.dtrtri(L, lower=1)
            assert info == 0
            r = R.diag_checks(blk, L, np.tril(W), npan)
            print('REF-LOG lapack    %-7s block %d %s' % (f, lo // 128, '  '.join('%s %.3g' % kv for kv in sorted(r.items()))))
            assert max(r[k] for k in ('factor', 'inv16', 'pad')) <= 1.0, (f, lo, r)


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_every_mistake_leaves_a_bar(mut, runs):
    """on the well-conditioned dense-sign family (b) and on the production-regime one (a_high): the mistake is a factor >= 1e3 outside"""
    for f in ('b', 'a_high'):
        A, run = runs[f]
        if mut in ('Woff', ):
            bad = R.mutate_run(run, mut)
            w = R.worst(R.check_diags(bad, A), R.check_products(bad, A))
        elif mut == 'nocouple':
            bad = R.emulate(A, split_k=True, _mut=(mut,))
            w = R.worst(R.check_diags(bad, A))
        elif mut == 'upper':
            w = R.worst(R.check_products(run, A, _mut=(mut,)))
            assert max(R.worst(R.check_products(R.mutate_run(run, mut), A)).values()) >= 1e3
        else:
            w = R.worst(R.check_products(run, A, _mut=(mut,)))
        assert max(w.values()) >= 1e3, (mut, f, w)
        clean = R.worst(R.check_diags(run, A), R.check_products(run, A))
        assert max(clean.values()) <= 1.0


def _lapack_info(A):
    _, info = lapack.dpotrf(A, lower=1)
    return info


def test_failure_index_equals_lapack():
    for value in (0.0, -1.0):
        for p in PIVOTS:
            A = R.exact_with_pivot(300, p, value)
            assert _lapack_info(A) == p, (value, p)
            for sk in (False, True):
                assert R.emulate(A, split_k=sk)['info'] == p, (value, p, sk)
    for p, q in ((5, 20), (20, 40), (100, 273)):       # two bad pivots: same panel / other half, other panel, other block -> the first
        A = R.exact_with_pivot(300, p, -1.0)
        A[q - 1, q - 1] = -1.0
        assert _lapack_info(A) == p and R.emulate(A)['info'] == p
    A = R.exact_family(300, 0)[0].copy()
    A[96, 96] = np.nan
    assert R.emulate(A)['info'] == 97
    # a last pivot of exactly 2^-40 passes, with L[n-1][n-1] = 2^-20 exactly
    A = R.exact_with_pivot(300, 300, 2.0 ** -40)
    assert _lapack_info(A) == 0 and np.linalg.cholesky(A)[299, 299] == 2.0 ** -20 and R.emulate(A)['L'][299, 299] == 2.0 ** -20
