"""Gradient steps take the latent variance from the J' product's epilogue (var = var0 + sum_m K J', no A2 product): ELBO and every
gradient block against the torch oracle over ragged M with Mf != Mg, D = 1 .. 8, several chunks with a partial last one, the merged
(paired) and the per-latent launch orders, and a case with cond(Kuu) ~ 1e8.  Tolerances are those of test_gpu_dense.py."""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

CASES = [
    # N, Mf, Mg, D, ell, chunk
    (1500, 70, 45, 1, 2.0, 1024),
    (2500, 200, 136, 2, 0.25, 1024),      # ragged, Mf != Mg, 3 chunks, the last one partial
    (2048, 128, 128, 3, 0.3, 1024),       # cond(Kuu_g) ~ 2e8
    (1700, 96, 140, 4, 0.5, 1024),
    (1400, 150, 90, 5, 0.6, 1024),
    (1100, 130, 64, 6, 0.7, 1024),
    (1000, 64, 300, 7, 0.8, 1024),
    (1300, 150, 100, 8, 0.9, 1024),
    (24000, 1000, 900, 3, 0.12, 8192),    # 8 row blocks per latent, 64 column panels: the merged (paired) launches; last chunk partial
]


def _conds(p, jitter):
    import zigp_oracle as o
    out = []
    for h in ('f', 'g'):
        Z = p['Z' + h]
        out.append(np.linalg.cond(o.rbf_K(Z, None, p['ell_' + h], p['var_' + h]) + jitter * np.eye(Z.shape[0])))
    return out


@pytest.mark.parametrize('N,Mf,Mg,D,ell,chunk', CASES)
def test_gradient_step_matches_oracle(engine, N, Mf, Mg, D, ell, chunk):
    import zigp_oracle_torch as ot
    X, Y, p = make_problem(N, Mf, D, seed=N + Mf + D, Mg=Mg, ell=ell, u_scale=0.5)
    if D == 1:
        X = X * 10.0
        p['Zf'] *= 10.0
        p['Zg'] *= 10.0
    engine.set_chunk(chunk)
    try:
        engine.set_data(X, Y)
        scale = 1.3
        ed, kl, g = engine.elbo(p, jitter=1e-6, scale=scale)
        ed_v, kl_v, _ = engine.elbo(p, jitter=1e-6, scale=scale, need_grad=False)    # value-only: variance through the A2 product
        elbo_r, data_r, kl_r, g_r = ot.elbo_and_grad(X, Y, p, 1e-6, scale=scale, chunk=2000)
    finally:
        engine.set_chunk(16384)
    c = max(_conds(p, 1e-6))
    print('N=%d Mf=%d Mg=%d D=%d cond %.1e: elbo rel %.1e, gradient step vs value-only elbo_data %.1e'
          % (N, Mf, Mg, D, c, abs((ed - kl) - elbo_r) / abs(elbo_r), abs(ed - ed_v) / abs(ed_v)))
    assert kl == kl_v
    assert abs(ed - scale * data_r) <= 1e-7 * abs(scale * data_r)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    assert abs(ed - ed_v) <= max(1e-9, 1e-16 * c) * abs(ed_v)
    for k in ot.PARAM_KEYS:
        a, b = np.asarray(g[k]).reshape(-1), np.asarray(g_r[k]).reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        print('  grad %-10s relerr %.2e' % (k, e))
        assert e < max(1e-6, 1e-13 * c), (k, e)


def test_gradient_step_bit_stable_with_and_without_overlap(engine):
    """The K-weighted column sums of the J' epilogue run in a fixed order: two calls, and the call with the stream overlap off, agree bit for bit."""
    X, Y, p = make_problem(5000, 200, 3, seed=3, Mg=136, ell=0.3)
    engine.set_chunk(2048)
    try:
        engine.set_data(X, Y)
        r0 = engine.elbo(p, jitter=1e-6)
        r1 = engine.elbo(p, jitter=1e-6)
        engine.set_overlap(False)
        try:
            r2 = engine.elbo(p, jitter=1e-6)
        finally:
            engine.set_overlap(True)
    finally:
        engine.set_chunk(16384)
    for r in (r1, r2):
        assert r[0] == r0[0] and r[1] == r0[1]
        for k in r0[2]:
            assert np.array_equal(np.asarray(r[2][k]), np.asarray(r0[2][k])), k
