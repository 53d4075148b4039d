"""CPU-side proof that the per-launch restatement of the panel path's M x M stage (tests/kronp_ref.py restate()) catches deliberate mistakes,
with the _mut idiom of tests/test_cpu_kronf_finish_ref.py.

kronp_ref.simulate() computes the taps of one latent of a panel step on the CPU (float64) from a fixture of kron_nd.BLOCK_CASES and
data-like cotangents; restate() on those taps reproduces every launch's output bit for bit (it is the same arithmetic).  With a mistake
switched on, restate() stands for a kernel that has it: the test asks that at least one launch's output then leaves the bound the GPU test
applies (16 eps S of that launch; here err_np = 0) -- by a factor of at least 1e3, so that the GPU test's own rounding cannot hide it.
Every mistake is caught on b21 (Mq 256 x 128) and on b12 (128 x 256), where the two padded sizes differ.  'S forced to nk' changes
nothing on those grids (nk = 64 <= 512 / (nba nbb) for every reduction): it is held by the rule itself, pinned here for every reduction of
every block case, and by the hook's facts and the plane count of b3's dP0 reduction on the GPU."""
import numpy as np
import pytest

import kron_nd as K
import kronp_ref as R

pytestmark = pytest.mark.filterwarnings(K.READ_ONLY_NOTE)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module', params=['b21', 'b12'])
def taps(request):
    name = request.param
    X, Y, p = K.block_problem(name)
    rs = np.random.RandomState(7)
    N = X.shape[0]
    gv = -0.5 * (0.5 + rs.rand(N))                 # the variance cotangent of a data term is negative
    cot = np.stack([rs.randn(N), gv, 0.3 * rs.randn(N), 0.3 * rs.randn(N)]) * 50.0
    out = {}
    for tag in 'fg':
        t, M, s = R.simulate(X, p, tag, cot, K.JITTER, True)
        out[tag] = (t, M, [p['Z' + tag][0], p['Z' + tag][1]], s)
    return name, out


def _worst_ratio(t, r):
    """largest |restated - tapped| / (16 eps S) over the launches, and the launch it belongs to"""
    worst, where = 0.0, None
    for name, (v, S) in r.items():
        a = np.asarray(R.tap_of(t, name), dtype=np.float64)
        v, S = np.asarray(v, dtype=np.float64), np.asarray(S, dtype=np.float64)
        assert a.shape == v.shape, (name, a.shape, v.shape)
        ratio = float(np.max(np.abs(v - a) / (16 * EPS * np.maximum(S, 1e-300))))
        if ratio > worst:
            worst, where = ratio, name
    return worst, where


def test_restatement_reproduces_the_simulated_taps(taps):
    name, lat = taps
    for tag, (t, M, Z, s) in lat.items():
        r = R.restate(t, M, Z, s, K.JITTER, True)
        assert set(r) >= {'P0', 'P1', 'T0', 'Al', 'vec', 'klv', 'red', 'T1_a', 'dU', 'T1_b', 'dP_acc0', 'dP_acc1', 'Q0', 'Q1', 'dP_comb0', 'dP_comb1',
                          'PdPP0', 'PdPP1', 'G0', 'G1', 'krow0', 'krow1', 'gu', 'gs'}
        for k, (v, S) in r.items():
            assert np.array_equal(np.asarray(v), np.asarray(R.tap_of(t, k))), (name, tag, k)
            assert np.all(np.asarray(S) >= np.abs(np.asarray(v)) * (1 - 1e-12)), (name, tag, k)       # S bounds its value
        # identity in the padding of K and P, zeros in the padding of every grid image, gu / gs compact
        for q in range(2):
            for k in ('K', 'P'):
                A = t[k][q]
                assert np.array_equal(A[M[q]:, M[q]:], np.eye(A.shape[0] - M[q])) and not A[M[q]:, :M[q]].any() and not A[:M[q], M[q]:].any(), (k, q)
        for k in ('U', 'S2', 'T0', 'Al', 'dAl', 'dS2', 'dU'):
            assert not t[k][M[0]:].any() and not t[k][:, M[1]:].any(), k
        assert t['gu'].shape == M and t['gs'].shape == M


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_every_mistake_is_caught(taps, mut):
    name, lat = taps
    ratios = {}
    for tag, (t, M, Z, s) in lat.items():
        ratios[tag] = _worst_ratio(t, R.restate(t, M, Z, s, K.JITTER, True, _mut=(mut,)))
    print('%s %-11s f: %.2e x the bound at %s   g: %.2e x at %s' % ((name, mut) + ratios['f'] + ratios['g']))
    for tag in 'fg':
        assert ratios[tag][0] >= 1e3, (name, mut, tag, ratios[tag])


def test_split_k_rule_at_every_block_case():
    """S = min(nk, 512 / (nba nbb)): equal to nk on every reduction of every block case but dP0 of b3 (3 x 3 tiles: 56 of nk = 128), the one
    place where 'S forced to nk' would show -- tests/test_gpu_kron_panel_stages.py reads that S from the hook's facts and sums its 56 planes"""
    below = []
    for name, k in K.BLOCK_CASES.items():
        nk = max(1024, -(-k['N'] // 1024) * 1024) // 16
        for tag, (nb0, nb1) in zip('fg', K.block_counts(name)):
            for red, (a, b) in (('dP0', (nb0, nb0)), ('dP1', (nb1, nb1)), ('dAl', (nb0, nb1)), ('dS2', (nb0, nb1))):
                S = R.split_k_slices(nk, a, b)
                assert 1 <= S <= nk
                if S != nk:
                    below.append((name, tag, red, S, nk))
    assert below == [('b3', 'f', 'dP0', 56, 128), ('b3', 'g', 'dP0', 56, 128)], below
