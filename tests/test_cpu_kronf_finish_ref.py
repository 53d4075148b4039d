"""Pins the restatement of the fused Kronecker path's finish stage (kronf_ref.finish / kl_scalars / assemble, kronf_matern_ref.finish) before
tests/test_gpu_kronf_stages.py and tests/test_gpu_kron_matern_fused.py hold k_kf_finish, k_kfl_finish<1..3>, k_kf_kd_prepare, k_kf_krow_merge and
k_kfl_krow_kinds to it.

* independent truth: the stage is the reverse pass of a scalar function of (U, s, Z_p, ell_p, var_p); torch autograd of that function, with
  fixed random linear functionals as the cotangents the earlier stages would deliver, must equal assemble(finish(.)).
* the rule can see the errors that matter: on CPU-made inputs of every fixture class of the GPU tests, each of eight deliberate mistakes
  FAILS err <= 4 err_np + 16 eps S against the long double result.
* exact tier: on kronf_ref.exact_problem inputs float64 and long double agree bit for bit, so the expectations the GPU test compares with
  `==` are exact.
"""
import numpy as np
import pytest

import kron_nd
import kronf_matern_ref as km
import kronf_ref as kr

EPS = kr.EPS
LD = np.longdouble


def _unpack(p, tag):
    return p['Z' + tag], [np.asarray(e, dtype=np.float64).reshape(-1) for e in p['ell_' + tag]], [float(np.squeeze(v)) for v in p['var_' + tag]]


kr16 = kr.moment_block16


def stage_inputs(X, p, tag, kinds, jitter, seed):
    """The finish stage's inputs of one latent, made on the CPU in float64 the way a step makes them: K_p + jitter I, its inverse, the latent
    stage (kronf_ref.latent) and the sums over points (kronf_matern_ref.backward) of random point cotangents -- the stage is linear in them.
    Returns (args, kw) of km.finish(kinds, *args, **kw)."""
    Z, ell, var = _unpack(p, tag)
    M = (Z[0].shape[0], Z[1].shape[0])
    N = X.shape[0]
    rs = np.random.RandomState(seed)
    K = [np.asarray(km.factor_K(kinds[q], Z[q], ell[q], var[q], jitter), dtype=np.float64) for q in range(2)]
    P = [np.linalg.inv(K[q]) for q in range(2)]
    P = [(a + a.T) / 2 for a in P]
    U, s = p['u_%sm' % tag].reshape(M), p['u_%ss_sqrt' % tag].reshape(M)
    lat = kr.latent(P[0], P[1], U)
    T0, T1, Al = (np.asarray(lat[k][0], dtype=np.float64) for k in ('T0', 'T1', 'Al'))
    zc = [0.5 * (Z[q].min(0) + Z[q].max(0)) for q in range(2)]
    gm, gv, dq0, dq1 = rs.randn(4, N) * np.array([[1.0], [0.3], [0.3], [0.3]])
    b = km.backward(kinds, P[0], P[1], Al, s * s, Z[0], Z[1], ell[0], ell[1], var[0], var[1], X, N, None, gm, gv, dq0, dq1, zc[0], zc[1])
    w = {k: np.asarray(b[k][0], dtype=np.float64) for k in ('dAl', 'dS2', 'dP0', 'dP1')}
    for q in range(2):
        w['Kr%d' % q] = kr16(np.asarray(b['Kr%d' % q][0], dtype=np.float64), None if b['Kd%d' % q] is None else np.asarray(b['Kd%d' % q][0], dtype=np.float64))
    return (w, K[0], K[1], P[0], P[1], U, s * s, T0, T1, Al, s, Z[0], Z[1], zc[0], zc[1], jitter), dict(ell=ell, var=var)


# =====================================================================================================================================
# independent truth: torch autograd
# =====================================================================================================================================
def _torch_K(torch, kind, Z, X, ell, var):
    d = (Z[:, None, :] - X[None, :, :]) / ell
    r2 = (d * d).sum(2)
    if kind == 'rbf':
        return var * torch.exp(-r2 / 2)
    r = torch.sqrt(r2 + km.FLOOR)
    if kind == 'matern32':
        t = 3 ** 0.5 * r
        return var * (1 + t) * torch.exp(-t)
    t = 5 ** 0.5 * r
    return var * (1 + t + 5.0 / 3.0 * r * r) * torch.exp(-t)


@pytest.mark.parametrize('kl', [True, False], ids=['kl', 'nokl'])
@pytest.mark.parametrize('kinds', [('rbf', 'rbf'), ('matern32', 'rbf'), ('rbf', 'matern52'), ('matern52', 'matern32')], ids=lambda k: '-'.join(k))
@pytest.mark.parametrize('grid,D', [((7, 9), (2, 1)), ((14, 50), (1, 3))], ids=['small', 'larger'])
def test_finish_and_assemble_are_the_autograd_gradient(grid, D, kinds, kl):
    """L = <dAl, Alpha(U, P)> + <dS2, s^2> + sum_p <dPc_p, P_p> + sum_p <dKx_p, K_p(Z_p, X_p)> - kl KL, P_p = (K_p(Z_p, Z_p) + jitter I)^-1,
    KL = GaussKLkron.  Its gradient with respect to U, s, Z_p, ell_p, var_p is assemble(finish(.)) when the work block holds dAl, dS2, the
    (unsymmetrised) dPc_p and the moments of t_p = dKx_p . K_p (Matern: of t'_p = dKx_p . K'_p in the columns 1 .. 2 D, sum t' in column 15).
    Per block, relative to the block's largest entry, at the 1e-8 floor of a reference's own error (tests/test_cpu_kron_nd.py)."""
    import torch
    rs = np.random.RandomState(5 + grid[0])
    M, N, jitter = grid, 37, 1e-5
    Xp = [rs.rand(N, D[0]) * 10, rs.rand(N, D[1])]
    Z = [rs.rand(M[0], D[0]) * 10, rs.rand(M[1], D[1])]
    if D[0] == 1:
        Z[0] = np.sort(Z[0], 0)
    ell = [0.5 * 10 * M[0] ** (-1.0 / D[0]) * (1 + 0.2 * rs.rand(D[0])), 0.5 * M[1] ** (-1.0 / D[1]) * (1 + 0.2 * rs.rand(D[1]))]
    var = [1.7, 0.8]
    U, s = 0.3 * rs.randn(*M), 0.5 + rs.rand(*M)
    dAl, dS2 = rs.randn(*M), rs.randn(*M)
    dPc = [rs.randn(M[q], M[q]) for q in range(2)]
    dKx = [rs.randn(M[q], N) for q in range(2)]
    # ---- autograd
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    tc = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    tU, ts, tZ, tl, tv = tt(U), tt(s), [tt(z) for z in Z], [tt(e) for e in ell], [tt(v) for v in var]
    Kt = [_torch_K(torch, kinds[q], tZ[q], tZ[q], tl[q], tv[q]) + jitter * torch.eye(M[q], dtype=torch.float64) for q in range(2)]
    Pt = [torch.linalg.inv(k) for k in Kt]
    Alt = Pt[0] @ tU @ Pt[1]
    L = (tc(dAl) * Alt).sum() + (tc(dS2) * ts * ts).sum()
    for q in range(2):
        L = L + (tc(dPc[q]) * Pt[q]).sum() + (tc(dKx[q]) * _torch_K(torch, kinds[q], tZ[q], tc(Xp[q]), tl[q], tv[q])).sum()
    if kl:
        d0, d1 = torch.diagonal(Pt[0]), torch.diagonal(Pt[1])
        KL = 0.5 * ((tU * Alt).sum() - M[0] * M[1] - torch.log(ts * ts).sum() + (d0[:, None] * d1[None, :] * ts * ts).sum()
                    + M[1] * torch.logdet(Kt[0]) + M[0] * torch.logdet(Kt[1]))
        L = L - KL
    L.backward()
    want = dict(u=tU.grad.numpy(), s=ts.grad.numpy(), Z=[z.grad.numpy() for z in tZ], ell=[e.grad.numpy() for e in tl], var=[float(v.grad) for v in tv])
    # ---- finish + assemble on the same numbers
    K = [Kt[q].detach().numpy() for q in range(2)]
    P = [Pt[q].detach().numpy() for q in range(2)]
    lat = kr.latent(P[0], P[1], U)
    zc = [0.5 * (Z[q].min(0) + Z[q].max(0)) for q in range(2)]
    w = dict(dAl=dAl, dS2=dS2, dP0=dPc[0], dP1=dPc[1])
    for q in range(2):
        Kx, _, Kdx, _ = km.ktile(kinds[q], Z[q], ell[q], var[q], Xp[q], grad=True)
        ps = kr.psi(Xp[q], zc[q])
        t, td = dKx[q] * Kx, dKx[q] * Kdx
        w['Kr%d' % q] = kr16(np.concatenate([t @ ps[:, :1], td @ ps[:, 1:]], 1), None if kinds[q] == 'rbf' else td.sum(1))
    f = km.finish(kinds, w, K[0], K[1], P[0], P[1], U, s * s, lat['T0'][0], lat['T1'][0], lat['Al'][0], s, Z[0], Z[1], zc[0], zc[1], jitter, kl, ell, var)
    got = kr.assemble([f['krow0'][0], f['krow1'][0]], f['gu'][0], f['gs'][0], ell, var, 0.0)
    worst = 0.0
    for k in ('u', 's'):
        worst = max(worst, kron_nd._relerr(got[k][0], want[k]))
    for q in range(2):
        for k in ('Z', 'ell', 'var'):
            e = kron_nd._relerr(got[k][q][0], want[k][q])
            assert e <= 1e-8, 'd %s_%d: %.3e' % (k, q, e)
            worst = max(worst, e)
        assert not np.any(f['krow%d' % q][0][:, -1]) and not np.any(f['krow%d' % q][1][:, -1])
    assert worst <= 1e-8, worst


def test_kinds_form_with_every_kind_rbf_is_the_rbf_form_bit_for_bit():
    X, Y, p = kron_nd.problem('d21-12')
    args, kw = stage_inputs(X, p, 'f', ('rbf', 'rbf'), kron_nd.JITTER, 3)
    for kl in (True, False):
        for dt in (np.float64, LD):
            a, b = km.finish(('rbf', 'rbf'), *args, kl, dtype=dt, **kw), kr.finish(*args, kl, dtype=dt)
            assert sorted(a) == sorted(b)
            for k in a:
                assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), k
    w = args[0]
    g, ag = kr.finish(*args, True)['G0']
    a = kr.krow_from_G(g, ag, args[1], w['Kr0'], args[11], args[13], kron_nd.JITTER)
    assert np.array_equal(a[0], kr.finish(*args, True)['krow0'][0])


def test_assemble_restates_the_host_chain_rule():
    rs = np.random.RandomState(0)
    krow = [rs.randn(5, 6), rs.randn(7, 4)]
    ell, var = [np.array([0.5, 2.0]), np.array([0.25])], [2.0, 0.5]
    a = kr.assemble(krow, rs.randn(5, 7), rs.randn(5, 7), ell, var, 3.0)
    assert np.allclose(a['Z'][0][0], krow[0][:, 1:3] / ell[0] ** 2) and np.allclose(a['ell'][1][0], krow[1][:, 2:3].sum(0) / ell[1] ** 3)
    assert np.isclose(a['var'][0][0], krow[0][:, 0].sum() / 2.0 + 3.0 * 0.5) and np.isclose(a['var'][1][0], krow[1][:, 0].sum() / 0.5 + 3.0 * 2.0)


def test_kl_scalars_against_the_literal_sums():
    rs = np.random.RandomState(1)
    U, Al, s, d0, d1 = rs.randn(6, 9), rs.randn(6, 9), 0.5 + rs.rand(6, 9), rs.rand(6), rs.rand(9)
    a, b = kr.kl_scalars(U, Al, s, d0, d1), kr.kl_scalars(U, Al, s, d0, d1, dtype=LD)
    want = (float(np.sum(U * Al)), float(np.sum(np.log(s ** 2))), float(np.einsum('i,j,ij->', d0, d1, s ** 2)))
    for k, v in zip(('uAl', 'logs2', 'ds2'), want):
        assert abs(a[k][0] - v) <= 16 * EPS * a[k][1] and abs(float(b[k][0]) - v) <= 16 * EPS * a[k][1] and a[k][1] >= abs(v)


# =====================================================================================================================================
# the rule can see the errors that matter
# =====================================================================================================================================
# fixture class -> (problem, latent, kinds).  c, the lengthscale constant of each problem, is the one recorded next to the case: kron_nd.CASES
# for the named fixtures (tuned there to floor <= 1e-8, cond <= 1e5 on the reference alone), EDGE_C below for the N = 33 edge grids.
EDGE_C, EDGE_GRIDS, EDGE_DS, edge_problem = kron_nd.EDGE_C, kron_nd.EDGE_GRIDS, kron_nd.EDGE_DS, kron_nd.edge_problem


def _fixture_classes():
    out = []
    for name in ['d21-12', 'd21-21', 'd11', 'd31', 'd21-mix2', 'd77', 'L32', 'L51', 'L77']:           # the bound tier (RBF)
        out.append(('bound/' + name, ('named', name), 'fg'[len(out) % 2], ('rbf', 'rbf')))
    for tag in 'fg':                                                                                  # the ill-conditioned pptr 32 x 32 init
        out.append(('bound/pptr32/' + tag, ('pptr',), tag, ('rbf', 'rbf')))
    for grid in EDGE_GRIDS:
        for D in EDGE_DS:
            out.append(('edge/%dx%d/D%d%d' % (grid + D), ('edge', grid, D), 'f', ('rbf', 'rbf')))
    kinds = km.fixture_kinds()
    for name in ['d11', 'd21-21', 'd31', 'd17', 'd77', 'd21-mix2', 'L32', 'L51', 'L77']:             # the Matern fixtures
        kf, kg = kinds[name] if name in kinds else L77_KINDS
        for tag, k in (('f', kf), ('g', kg)):
            if tuple(k) != ('rbf', 'rbf'):
                out.append(('matern/%s/%s' % (name, tag), ('named', name), tag, tuple(k)))
    return out


L77_KINDS = km.L77_KINDS
CLASSES = _fixture_classes()


def _fails(mut64, f64, fld, keys):
    """True when the mutated float64 result breaks err <= 4 err_np + 16 eps S on some element of some output in `keys`"""
    for k in keys:
        truth = np.asarray(fld[k][0], dtype=LD)
        S = np.asarray(f64[k][1], dtype=np.float64)
        err = np.asarray(np.abs(np.asarray(mut64[k][0], dtype=LD) - truth), dtype=np.float64)
        err_np = np.asarray(np.abs(np.asarray(f64[k][0], dtype=LD) - truth), dtype=np.float64)
        if np.any(err > 4 * err_np + 16 * EPS * S):
            return True
    return False


@pytest.mark.parametrize('case', CLASSES, ids=[c[0] for c in CLASSES])
def test_rule_catches_each_mutation(case):
    label, src, tag, kinds = case
    if src[0] == 'pptr':
        X, p = kron_nd.pptr_problem((32, 32))[2::2]
    else:
        X, Y, p = kron_nd.problem(src[1]) if src[0] == 'named' else edge_problem(src[1], src[2])
    jitter = kron_nd.JITTER
    args, kw = stage_inputs(X, p, tag, kinds, jitter, 11)
    M = (args[3].shape[0], args[4].shape[0])
    run = lambda kl, dtype=np.float64, a=args, **o: km.finish(kinds, *a, kl, dtype=dtype, **kw, **o)
    base = {kl: (run(kl), run(kl, LD)) for kl in (True, False)}
    for kl in (True, False):        # the unmutated float64 result itself passes
        assert not _fails(base[kl][0], base[kl][0], base[kl][1], ('krow0', 'krow1', 'gu', 'gs', 'G0', 'G1'))
    krows = ('krow0', 'krow1')
    missed = []

    def expect(name, kl, keys=krows, **o):
        """the mistake must break the rule -- unless it IS no mistake on this fixture: a one-point factor has no off-diagonal entry, no
        z_j - z_m and z_m = zc, so some of them leave the long double result bit for bit unchanged there, and nothing could see them"""
        if _fails(run(kl, **o), base[kl][0], base[kl][1], keys):
            return
        mld = run(kl, LD, **o)
        if any(not np.array_equal(mld[k][0], base[kl][1][k][0]) for k in keys):
            missed.append('%s (kl %s)' % (name, kl))
        else:
            identities.append(name)

    identities = []
    nojit = args[:15] + (0.0,)
    for kl in (True, False):
        expect('K_p used without subtracting the jitter', kl, a=nojit)
        expect('dP not symmetrised', kl, _mut=('nosym',))
        expect('factor 2 of the first-moment column dropped', kl, _mut=('no2',))
        expect('re-centring with dz of the wrong sign', kl, _mut=('dzsign',))
    if M[0] != M[1]:
        expect('coef formed with M_p instead of M_o', True, _mut=('coefMp',))
    expect('1/4 (Q + Q^T) dropped', True, _mut=('noQ',))
    for q in range(2):
        if kinds[q] == 'rbf':
            continue
        w, (Z, ell, var) = args[0], _unpack(p, tag)
        col0 = dict(w)
        col0['Kr%d' % q] = w['Kr%d' % q].copy()
        col0['Kr%d' % q][:, 15] = w['Kr%d' % q][:, 0]
        Kplain = km.ktile(kinds[q], Z[q], ell[q], var[q], Z[q], grad=True)[:2]
        for kl in (True, False):
            expect('Matern factor %d re-centred with column 0' % q, kl, krows[q:q + 1], a=(col0,) + args[1:])
            expect('Matern factor %d moment columns with K instead of K\'' % q, kl, krows[q:q + 1], Kd=tuple(Kplain if i == q else None for i in range(2)))
    assert min(M) == 1 or not identities, '%s: no mistake at all on a grid without a one-point factor: %s' % (label, identities)
    assert not missed, '%s: not caught: %s' % (label, '; '.join(missed))


# =====================================================================================================================================
# exact tier
# =====================================================================================================================================
exact_finish, exact_gs_mask = kr.exact_finish, kr.exact_gs_mask


@pytest.mark.parametrize('jitter', [0.0, 0.25])
@pytest.mark.parametrize('grids,D', [(((6, 5), None), (2, 1)), (((20, 9), (9, 20)), (3, 2)), (((17, 31), None), (7, 7)), (((16, 112), (9, 50)), (1, 1)),
                                     (((10, 100), None), (2, 1))])
def test_exact_tier_finish_is_exact(grids, D, jitter):
    """On exact-tier inputs the float64 stage equals the long double one bit for bit -- with kl off AND with kl on, which is how the steps of
    the GPU exact tier run (tests/test_gpu_kronf_stages.py::_assert_exact_taps compares with kronf_ref.exact_finish(..., kl=True) by `==`).
    Why: P_p = I / c_p with c_p a power of 4 makes dAl T^T, P X P and P dAl P scalings by powers of two of small integers (P_p is diagonal: one
    non-zero term per inner sum); kz = K - jitter I is var_p I exactly (4 - 0, 4 - 1/4, ...); the inducing inputs and the centre are small
    multiples of powers of two; the moment sums are sums of such numbers far below 2^53.  The KL terms keep that: Q_p = U U^T / c_o and
    w_p = sum s^2 / c_o are integers over a power of 4, coef P = M_o / (2 c_p), gu subtracts Alpha = U / (c_0 c_1).
    Exact with kl on: krow0, krow1, gu, G of factor 0, P Q2 of factor 1, and gs where s is 1 or 2.  NOT exact with kl on: gs where s = 3,
    since -1 / 3 is rounded (exact_gs_mask leaves those elements out, here and on the GPU).  The KL scalars klv (log s^2) are not exact
    either and are held by the rule in the bound tier, not here."""
    e = kr.exact_problem(grids[0], grids[1], D, 200, jitter, seed=3)
    for L in e['lat']:
        for kl in (False, True):
            a, b = exact_finish(L, D, jitter, kl), exact_finish(L, D, jitter, kl, LD)
            for k in ('krow0', 'krow1', 'gu', 'gs', 'G0', 'PXP1'):
                keep = exact_gs_mask(L) if (k == 'gs' and kl) else np.ones(a[k][0].shape, dtype=bool)
                assert keep.any()
                assert np.array_equal(np.asarray(a[k][0], dtype=LD)[keep], b[k][0][keep]), '%s is not exact on the exact tier (kl %s)' % (k, kl)
                assert np.all(np.isfinite(a[k][0]))
