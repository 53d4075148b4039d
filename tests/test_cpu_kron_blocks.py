"""CPU-side pin of the fixtures of tests/test_gpu_kron_blocks.py (kron_nd.BLOCK_CASES: inducing grids beyond one 128-row block of the
GEMM-panel path), before any GPU result is looked at.

* every case whose literal (dense) oracle can be evaluated holds the project's fixture conditions on the reference alone: op-order floor
  <= 1e-8, max cond(K_p + jitter) <= 1e5, 40 % to 80 % exact zeros in Y, N no multiple of 16, every gradient block of the oracle live in
  every input dimension; the block counts are what the table says they are, and one case has N > 1024;
* b22 (130 x 129: literal form 16 770 x 16 770) holds cond <= 1e5; its truth is the factored restatement tests/kronp_ref.py;
* that restatement equals the literal oracle in value, KL, the nine predictive rows and every autograd gradient, per block and per input
  dimension, to 1e-8 relative (the fixture floor) on b21, b12 and bmix -- the grids with 2 x 1, 1 x 2 and both block shapes;
* the Matern run of the block cases holds the same floor and conditioning against tests/kron_matern_ref.py.
Every test prints its figures (pytest -s); they are recorded in profiles/kron_panel_stage_parity.log."""
import numpy as np
import pytest

import kron_nd as K

pytestmark = pytest.mark.filterwarnings(K.READ_ONLY_NOTE)

EXPECTED_BLOCKS = {'b21': ((2, 1), (2, 1)), 'b12': ((1, 2), (1, 2)), 'bmix': ((2, 1), (1, 2)), 'b3': ((3, 1), (3, 1)),
                   'bedge': ((2, 1), (1, 1)), 'b22': ((2, 2), (2, 2))}
KERN_KEYS = ('Zf', 'Zg', 'ell_f', 'ell_g', 'var_f', 'var_g')
VEC_KEYS = ('u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'noise')


def test_table():
    assert set(K.BLOCK_CASES) == set(EXPECTED_BLOCKS)
    for name, k in K.BLOCK_CASES.items():
        assert K.block_counts(name) == EXPECTED_BLOCKS[name], name
        assert k['N'] % 16 and k['N'] <= 1031 and max(k['f'] + (k['g'] or ())) <= 384, name
    assert any(k['N'] > 1024 for k in K.BLOCK_CASES.values())                  # Nc = 2048: nk and the split-K S change
    k = K.BLOCK_CASES['bedge']
    assert k['f'][0] == 129 and k['g'][0] == 128                               # the 128 / 129 boundary in one step
    for name in K.BLOCK_LITERAL:                                               # the literal oracle up to ~3 100 inducing points in total (bmix)
        k = K.BLOCK_CASES[name]
        g = k['g'] or k['f']
        assert k['f'][0] * k['f'][1] + g[0] * g[1] <= 3200, name


@pytest.mark.parametrize('name', K.BLOCK_LITERAL)
def test_fixture_floor_conditioning_zeros_and_live_gradients(name):
    X, Y, p = K.block_problem(name)
    k = K.BLOCK_CASES[name]
    g_grid = k['g'] or k['f']
    assert X.shape == (k['N'], sum(k['D']))
    assert [Z.shape for Z in p['Zf']] == [(k['f'][0], k['D'][0]), (k['f'][1], k['D'][1])]
    assert [Z.shape for Z in p['Zg']] == [(g_grid[0], k['D'][0]), (g_grid[1], k['D'][1])]
    floor, cond = K.fixture_floor_and_cond(X, p, ref=K.block_oracle_predict(name, 0.0))
    zeros = float(np.mean(Y == 0.0))
    print('%-6s D %s f %s g %s N %d c %s: op-order floor %.2e, max cond(K_p + jitter) %.2e, zeros %.2f'
          % (name, k['D'], k['f'], k['g'] or 'same', X.shape[0], k['c'], floor, cond, zeros))
    assert floor <= 1e-8, floor
    assert cond <= 1e5, cond
    assert 0.4 <= zeros <= 0.8, zeros
    g = K.block_oracle_grad(name)[3]
    for key in ('Zf', 'Zg', 'ell_f', 'ell_g'):
        for q in range(2):
            a = np.abs(np.asarray(g[key][q])).reshape(-1, k['D'][q])
            assert np.all(a.max(0) > 0.0), (key, q, a.max(0))
    for key in ('var_f', 'var_g'):
        for q in range(2):
            assert abs(float(np.squeeze(g[key][q]))) > 0.0, (key, q)
    for key in VEC_KEYS:
        assert np.max(np.abs(np.asarray(g[key]))) > 0.0, key


def test_b22_conditioning():
    """the 2 x 2-block grid: cond alone (its literal form is not evaluated), zeros, and a finite restatement with live gradients"""
    X, Y, p = K.block_problem('b22')
    cond, zeros = K.fixture_cond(p), float(np.mean(Y == 0.0))
    print('b22    D %s f %s N %d c %s: max cond(K_p + jitter) %.2e, zeros %.2f' % (K.BLOCK_CASES['b22']['D'], K.BLOCK_CASES['b22']['f'], X.shape[0],
                                                                                  K.BLOCK_CASES['b22']['c'], cond, zeros))
    assert cond <= 1e5 and 0.4 <= zeros <= 0.8, (cond, zeros)
    e, d, kl, g = K.block_oracle_grad('b22')
    assert np.isfinite([e, d, kl]).all()
    for key in KERN_KEYS:
        for q in range(2):
            a = np.asarray(g[key][q], dtype=np.float64)
            assert np.isfinite(a).all() and np.all(np.abs(a).reshape(-1, a.shape[-1] if a.ndim > 1 else 1).max(0) > 0.0), (key, q)
    for key in VEC_KEYS:
        assert np.isfinite(np.asarray(g[key])).all() and np.max(np.abs(np.asarray(g[key]))) > 0.0, key


@pytest.mark.parametrize('name', ['b21', 'b12', 'bmix'])
def test_factored_restatement_equals_literal_oracle(name):
    """kronp_ref.factored_* against the literal oracle: value, KL, predictive rows, every gradient block and input dimension to 1e-8"""
    import kronp_ref as R
    X, Y, p = K.block_problem(name)
    dims, scale = K.BLOCK_CASES[name]['D'], K.block_scale(name)
    worst = 0.0
    for goff in (0.0, -1.0):
        a, b = R.factored_predict(X, p, K.JITTER, goff), K.block_oracle_predict(name, goff)
        worst = max([worst] + [K._relerr(a[i], b[i]) for i in range(9)])
    print('%s restatement vs literal: predictive rows %.2e' % (name, worst))
    for include_kl in (True, False):
        e, d, kl, g = R.factored_elbo_and_grad(X, Y, p, K.JITTER, scale=scale, include_kl=include_kl)
        e_r, d_r, kl_r, g_r = K.block_oracle_grad(name, include_kl)
        ev, ek = abs(d - d_r) / abs(d_r), (abs(kl - kl_r) / abs(kl_r) if include_kl else abs(kl) + abs(kl_r))
        eg = 0.0
        for key in KERN_KEYS:
            for q in range(2):
                u, v = np.asarray(g[key][q], dtype=np.float64).reshape(-1), np.asarray(g_r[key][q], dtype=np.float64).reshape(-1)
                eg = max(eg, K._relerr(u, v))
                if not key.startswith('var'):
                    u2, v2 = u.reshape(-1, dims[q]), v.reshape(-1, dims[q])
                    eg = max(eg, float(np.max(np.max(np.abs(u2 - v2), 0) / np.max(np.abs(v2), 0))))
        for key in VEC_KEYS:
            eg = max(eg, K._relerr(g[key], g_r[key]))
        print('%s restatement vs literal, include_kl %s: data %.2e kl %.2e worst gradient block / dimension %.2e' % (name, include_kl, ev, ek, eg))
        worst = max(worst, ev, ek, eg)
    assert worst <= 1e-8, worst


def test_matern_fixture_floor_and_conditioning():
    import kron_matern_ref as kmr
    X, Y, p = K.block_matern_fixture()
    assert kmr.kinds_of(p) == (('matern32', 'rbf'), ('matern52', 'matern52'))
    floor, cond = kmr.fixture_floor_and_cond(X, p, K.JITTER)
    print('%s f %s g %s: op-order floor %.2e, cond %s' % (K.BLOCK_MATERN + (floor, ' '.join('%s %.2e' % kv for kv in sorted(cond.items())))))
    assert floor <= 1e-8 and max(cond.values()) <= 1e5, (floor, cond)


@pytest.mark.parametrize('grid', K.BLOCK_EDGE_GRIDS)
def test_edge_grid_conditioning(grid):
    """the further grids of the stage tests: floor and conditioning as for the block cases"""
    X, Y, p = K.block_edge_problem(grid)
    floor, cond = K.fixture_floor_and_cond(X, p)
    print('%d x %d (N = %d, c %s): op-order floor %.2e, max cond(K_p + jitter) %.2e' % (grid + (X.shape[0], K.BLOCK_EDGE_C, floor, cond)))
    assert floor <= 1e-8 and cond <= 1e5, (floor, cond)
