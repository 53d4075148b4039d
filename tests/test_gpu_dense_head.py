"""GPU parity of the single-latent heads on the dense path (zigp_head_elbo / zigp_head_predict; DenseEngine.head_elbo / head_predict;
onoffgpf.SVGP) against tests/dense_head_ref.py, the CPU restatement (checked by tests/test_cpu_dense_head.py).

Bounds are the dense path's own (tests/test_gpu_dense.py, tests/test_gpu_matern.py): data term 1e-7, KL 1e-8, predict rows
min(max(1e-9, 1e-13 cond), 1e-6), gradients max(1e-6, 1e-13 cond) per block, cond = cond(Kuu + jitter I) of latent f, computed and
asserted on the CPU side first (it cannot exceed Mf var_f / jitter by more than rounding) and printed with every measured error.

A head call runs the two-latent schedule with a one-point placeholder latent; no dense test went below M = 12 before, so the first
test here is the plain OnOff model at Mg = 1 against the oracle."""
import functools

import numpy as np
import pytest

from conftest import make_problem, relerr
import dense_head_ref as hr
import matern_ref as mr
import fullcov_ref as fr

pytestmark = pytest.mark.gpu
JIT = 1e-6
N_ROWS = 1500          # with set_chunk(1024): two chunks, the second ragged (476 rows in a 1024-row pass)
ROWS4 = ('fmean', 'fvar', 'pfmean', 'pfvar')


def _labels(Y, lik):
    return (Y != 0) * 1.0 if lik == 'bernoulli' else Y


def _cond_f(p, jitter=JIT):
    c = mr.kuu_cond(p, jitter)
    M = np.shape(p['Zf'])[0]
    assert np.isfinite(c) and 1.0 <= c <= 1.001 * M * float(p['var_f']) / jitter + 1.0, c      # eigenvalues lie in [jitter, M var + jitter]
    return c


# Mf, D, mode, kind, mean, include_kl, scale -- every value of the issue's list occurs: Mf 37 / 137, D 1 / 3 / 8 / 9, the three
# parametrisations, RBF / Matern52, Zero / Constant / Linear, include_kl 0 / 1, scale != 1
CASES = [
    (37, 3, 'diag', 'rbf', 'zero', 1, 1.7),
    (137, 1, 'diag', 'rbf', 'constant', 1, 1.0),
    (37, 8, 'white', 'matern52', 'linear', 1, 2.5),
    (137, 9, 'white_full', 'rbf', 'constant', 0, 1.7),
    (37, 3, 'white_full', 'matern52', 'zero', 1, 1.0),
    (137, 8, 'diag', 'matern52', 'linear', 0, 0.6),
    (37, 9, 'diag', 'rbf', 'zero', 1, 1.7),
    (37, 1, 'white', 'rbf', 'linear', 1, 1.3),
]
_ID = lambda c: 'M%d_D%d_%s_%s_%s_kl%d' % c[:6]      # noqa: E731


@functools.lru_cache(maxsize=None)
def _problem(Mf, D, mode, kind, mean):
    X, Y, p = mr.problem(N_ROWS, Mf, 5, D)
    if mode == 'white':
        p['whiten'] = True
    if mode == 'white_full':
        p = fr.make_lq(p, seed=3, negative=2)
    p = {k: v for k, v in p.items() if k in hr.HEAD_KEYS + ('whiten', 'q_diag')}
    p['noise'] = 0.05
    if kind != 'rbf':
        p['kern_f'] = kind
    rs = np.random.RandomState(Mf + D)
    if mean in ('constant', 'linear'):
        p['mean_b'] = 0.37
    if mean == 'linear':
        p['mean_a'] = rs.randint(-4, 5, D) / 8.0
    return X, Y, p


@functools.lru_cache(maxsize=None)
def _reference(case, lik):
    """the restatement of one case, computed once and shared (never modified)"""
    Mf, D, mode, kind, mean, include_kl, scale = case
    X, Y, p = _problem(Mf, D, mode, kind, mean)
    Yl = _labels(Y, lik)
    return (hr.elbo_and_grad(X, Yl, p, lik, JIT, scale=scale, include_kl=bool(include_kl)), hr.head_predict(X[:400], p, lik, JIT))


def _grad_keys(p, lik):
    return tuple(k for k in hr.HEAD_KEYS if not (k == 'noise' and lik == 'bernoulli')) + tuple(k for k in ('mean_a', 'mean_b') if k in p)


def _check_grads(tag, g, g_r, c, keys):
    worst = 0.0
    for k in keys:
        a, b = np.asarray(g[k], dtype=float).reshape(-1), np.asarray(g_r[k], dtype=float).reshape(-1)
        e = np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
        worst = max(worst, e)
        print('  %s grad %-10s relerr %.2e (max |ref| %.3e)' % (tag, k, e, np.max(np.abs(b))))
        assert e < max(1e-6, 1e-13 * c), (k, e)
    return worst


# =====================================================================================================================================
# the guard: the OnOff model with a one-point latent g
# =====================================================================================================================================
@pytest.mark.parametrize('which', ['random_point', 'placeholder'])
def test_onoff_with_a_one_point_latent_g_matches_the_oracle(engine, which):
    """zigp_elbo and zigp_predict at Mg = 1 (a 128-row panel holding one inducing point) under the dense bounds: a random point with its own
    u, s, ell, var, and the heads' placeholder itself (origin, u = 0, s = 1, ell = var = 1)."""
    import zigp
    import zigp_oracle_torch as ot
    X, Y, p = make_problem(N_ROWS, 37, 3, seed=11, Mg=1)
    if which == 'placeholder':
        p = dict(p, **{k: v for k, v in zigp.head_placeholder(3).items() if k != 'kern_g'})
    c = _cond_f(p)
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=JIT, scale=1.7)
    ed_v = engine.elbo(p, jitter=JIT, scale=1.7, need_grad=False)[0]
    elbo_r, data_r, kl_r, g_r = ot.elbo_and_grad(X, Y, p, JIT, scale=1.7, chunk=500)
    e_d, e_v, e_k = abs(ed - 1.7 * data_r) / abs(1.7 * data_r), abs(ed_v - 1.7 * data_r) / abs(1.7 * data_r), abs(kl - kl_r) / abs(kl_r)
    print('HEAD-PARITY guard Mg=1 %s: cond(Kuu_f)=%.2e data rel %.2e (value-only %.2e) kl rel %.2e' % (which, c, e_d, e_v, e_k))
    assert e_d <= 1e-7 and e_v <= 1e-7 and e_k <= 1e-8
    _check_grads('guard ' + which, g, g_r, c, ot.PARAM_KEYS)
    out, ref = engine.predict(p, X[:400], jitter=JIT), ot_predict(X[:400], p)
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    for i in range(9):
        assert relerr(out[i], ref[i]) < tol, i
    engine.set_chunk(16384)


def ot_predict(X, p):
    return mr.build_predict(X, p, JIT)


# =====================================================================================================================================
# both heads against the restatement
# =====================================================================================================================================
@pytest.mark.parametrize('lik', hr.LIKS)
@pytest.mark.parametrize('case', CASES, ids=_ID)
def test_heads_match_the_restatement(engine, case, lik):
    Mf, D, mode, kind, mean, include_kl, scale = case
    X, Y, p = _problem(Mf, D, mode, kind, mean)
    c = _cond_f(p)
    (elbo_r, data_r, kl_r, g_r), pred_r = _reference(case, lik)
    engine.set_chunk(1024)
    engine.set_data(X, _labels(Y, lik))
    ed, kl, g = engine.head_elbo(p, lik, jitter=JIT, scale=scale, include_kl=bool(include_kl))
    ed_v, kl_v, none = engine.head_elbo(p, lik, jitter=JIT, scale=scale, include_kl=bool(include_kl), need_grad=False)
    e_d, e_v = abs(ed - scale * data_r) / abs(scale * data_r), abs(ed_v - scale * data_r) / abs(scale * data_r)
    e_k = abs(kl - kl_r) / abs(kl_r) if include_kl else 0.0
    print('HEAD-PARITY %s %s: cond(Kuu)=%.2e data rel %.2e (value-only %.2e) kl rel %.2e' % (lik, _ID(case), c, e_d, e_v, e_k))
    assert none is None and kl_v == kl
    assert e_d <= 1e-7 and e_v <= 1e-7
    assert e_k <= 1e-8 if include_kl else (kl == 0.0 and kl_r == 0.0)
    assert abs((ed - kl) - elbo_r) <= 1e-7 * abs(elbo_r)
    mean_keys = {'mean_a', 'mean_b'} if 'mean_b' in p else set()      # (a Constant mean returns an empty mean_a, as elbo does)
    assert set(g) == set(hr.HEAD_KEYS) | mean_keys
    if lik == 'bernoulli':
        assert g['noise'] == 0.0
    w = _check_grads('%s %s' % (lik, _ID(case)), g, g_r, c, _grad_keys(p, lik))
    out = engine.head_predict(p, X[:400], lik, jitter=JIT)
    tol = min(max(1e-9, 1e-13 * c), 1e-6)
    worst_p = 0.0
    for i, name in enumerate(ROWS4):
        e = relerr(out[i], pred_r[i])
        worst_p = max(worst_p, e)
        assert e < tol, (name, e, c)
    print('HEAD-PARITY %s %s: worst gradient block %.2e, worst predict row %.2e (bound %.1e)' % (lik, _ID(case), w, worst_p, tol))
    engine.set_chunk(16384)


# =====================================================================================================================================
# ties to the calls that exist already
# =====================================================================================================================================
@pytest.mark.parametrize('lik', hr.LIKS)
@pytest.mark.parametrize('case', [CASES[0], CASES[2], CASES[4]], ids=_ID)
def test_predict_rows_are_the_onoff_rows_and_the_density_rows(engine, case, lik):
    """Rows 0 and 1 of head_predict are rows 3 and 4 of predict on the same launches (the placeholder as latent g), bit for bit -- the
    head kernel sums the planes of f as k_pointwise does; rows 2 and 3 are density_rows' ymean and yvar at those rows, bit for bit;
    head_predict_device returns the same block."""
    import torch
    import zigp
    Mf, D, mode, kind, mean, _, _ = case
    X, Y, p = _problem(Mf, D, mode, kind, mean)
    engine.set_chunk(1024)
    out = engine.head_predict(p, X, lik, jitter=JIT)
    full = engine.predict(dict(p, **zigp.head_placeholder(D, q_full=mode == 'white_full')), X, jitter=JIT)
    assert np.array_equal(out[0], full[3]) and np.array_equal(out[1], full[4])
    rows, total = engine.density_rows(lik, out[0], out[1], None, None, _labels(Y, lik).reshape(-1), p['noise'])
    assert np.array_equal(out[2], rows[1]) and np.array_equal(out[3], rows[2])
    assert np.all(np.isfinite(rows[0])) and np.isfinite(total)
    dev = engine.head_predict_device(p, torch.from_numpy(X).to('cuda:0'), lik, jitter=JIT)
    assert np.array_equal(dev.cpu().numpy(), out)
    engine.set_chunk(16384)


def test_kl_is_latent_f_alone_at_a_jitter_that_shows_the_placeholder(engine):
    """At jitter 1e-2 the placeholder's own KL is 0.5 (1 / 1.01 - 1 + log 1.01) = 2.5e-5 (unwhitened): kl is KL_f -- prior_kl's entry for
    latent f (1e-13: the bound tests/test_gpu_matern.py puts on that call) -- and not the pair's sum."""
    import zigp
    X, Y, p = _problem(37, 3, 'diag', 'rbf', 'zero')
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    _, kl, _ = engine.head_elbo(p, 'gaussian', jitter=1e-2)
    kl2 = engine.prior_kl(dict(p, **zigp.head_placeholder(3)), jitter=1e-2)
    assert kl2[1] > 2e-5
    assert abs(kl - kl2[0]) <= 1e-13 * abs(kl2[0]) and abs(kl - kl2.sum()) > 1e-8 * abs(kl)
    kl_r = hr.elbo_and_grad(X[:10], Y[:10], p, 'gaussian', 1e-2, need_grad=False)[2]
    assert abs(kl - kl_r) <= 1e-8 * abs(kl_r)
    engine.set_chunk(16384)


def test_bernoulli_p_equals_the_kronecker_head_on_an_equivalent_grid(engine):
    """Small integers: inducing inputs 100 lengthscales apart (Kuu = I exactly at jitter 0, exp(-5000) = 0), rows on the inducing inputs,
    integer u and dyadic s -- fmean = u_m and fvar = s_m^2 exactly on both paths, so the dense head's p equals the Kronecker
    head's (a 3 x 1 grid: the second factor is one point at 0 with variance 1, the rows carry a zero column) bit for bit: one link, one
    arithmetic."""
    Z0 = np.array([[0.0], [100.0], [200.0]])
    u, s = np.array([-2.0, 0.0, 3.0]), np.array([0.5, 1.0, 1.5])
    idx = np.arange(300) % 3
    X0 = Z0[idx]
    p_dense = dict(Zf=Z0, u_fm=u, u_fs_sqrt=s, ell_f=np.ones(1), var_f=1.0)
    p_kron = dict(Zf=[Z0, np.zeros((1, 1))], ell_f=[np.ones(1), np.ones(1)], var_f=[1.0, 1.0], u_fm=u, u_fs_sqrt=s)
    out = engine.head_predict(p_dense, X0, 'bernoulli', jitter=0.0)
    ref = engine.kron_head_predict(p_kron, np.hstack([X0, np.zeros((300, 1))]), 'bernoulli', jitter=0.0)
    assert np.array_equal(out[0], u[idx]) and np.array_equal(out[1], (s * s)[idx])
    assert np.array_equal(ref[0], u[idx]) and np.array_equal(ref[1], (s * s)[idx])
    assert np.array_equal(out[2], ref[2])
    # p - p^2: the dense head rounds p (1 - p) as zigp_density_rows does, the Kronecker head pr - pr * pr: two roundings of one number
    assert np.all(np.abs(out[3] - ref[3]) <= 2 * np.spacing(ref[3]))
    assert 0.001 <= out[2].min() < 0.05 and out[2].max() > 0.9      # z = -2 / sqrt(1.25) and 3 / sqrt(3.25): both tails of the link


@pytest.mark.parametrize('lik', hr.LIKS)
def test_row_ranges_and_selected_rows(engine, lik):
    """Two row ranges sum to the whole call (1e-12 relative; gradients to the dense path's own 1e-8); rows= on the engine equals the same
    rows set as the data, bit for bit; select_rows with repeats matches the restatement."""
    case = CASES[0]
    X, Y, p = _problem(*case[:5])
    Yl = _labels(Y, lik)
    engine.set_chunk(1024)
    engine.set_data(X, Yl)
    ed, kl, g = engine.head_elbo(p, lik, scale=1.7)
    a, b = engine.head_elbo(p, lik, scale=1.7, rows=(0, 700), include_kl=False), engine.head_elbo(p, lik, scale=1.7, rows=(700, N_ROWS))
    assert abs((a[0] + b[0]) - ed) <= 1e-12 * abs(ed) and a[1] == 0.0 and b[1] == kl
    for k in _grad_keys(p, lik):
        s = np.asarray(a[2][k], dtype=float) + np.asarray(b[2][k], dtype=float)
        assert np.max(np.abs(s - np.asarray(g[k], dtype=float))) <= 1e-8 * max(np.max(np.abs(np.asarray(g[k], dtype=float))), 1e-300), k
    lo, hi = 100, 1450                                     # crosses the chunk boundary: [100, 1124) and [1124, 1450)
    got = engine.head_elbo(p, lik, scale=2.5, rows=(lo, hi))
    engine.set_data(X[lo:hi], Yl[lo:hi])
    host = engine.head_elbo(p, lik, scale=2.5)
    assert got[0] == host[0] and got[1] == host[1]
    for k in host[2]:
        assert np.array_equal(np.asarray(got[2][k]), np.asarray(host[2][k])), k
    engine.set_data(X, Yl)
    idx = np.random.RandomState(4).randint(0, N_ROWS, size=1300)
    idx[10:20] = idx[0]
    engine.select_rows(idx)
    sel = engine.head_elbo(p, lik, scale=1.5)
    engine.select_rows(None)
    e_r, d_r, kl_r, g_r = hr.elbo_and_grad(X[idx], Yl[idx], p, lik, JIT, scale=1.5)
    assert abs(sel[0] - 1.5 * d_r) <= 1e-7 * abs(1.5 * d_r) and abs(sel[1] - kl_r) <= 1e-8 * abs(kl_r)
    _check_grads('select_rows ' + lik, sel[2], g_r, _cond_f(p), _grad_keys(p, lik))
    engine.set_chunk(16384)


def test_a_head_call_leaves_the_onoff_calls_as_they_were(engine):
    """OnOff, head, OnOff on one context (Matern52 on latent g, which the head call neither reads nor changes): the second OnOff call
    returns the bits of the first, elbo and predict."""
    X, Y, p = mr.problem(N_ROWS, 50, 37, 3)
    p = dict(p, kern_g='matern52')
    ph = {k: v for k, v in p.items() if k in hr.HEAD_KEYS}
    engine.set_chunk(1024)
    engine.set_data(X, Y)
    first, pred1 = engine.elbo(p, scale=1.7), engine.predict(p, X[:300])
    for lik in hr.LIKS:
        engine.head_elbo(ph, lik, scale=0.5)
        engine.head_predict(ph, X[:200], lik)
    assert engine.get_kernel(1) == 'matern52'
    second, pred2 = engine.elbo(p, scale=1.7), engine.predict(p, X[:300])
    assert first[0] == second[0] and first[1] == second[1]
    for k in first[2]:
        assert np.array_equal(np.asarray(first[2][k]), np.asarray(second[2][k])), k
    assert np.array_equal(pred1, pred2)
    engine.set_chunk(16384)


def test_refusals_leave_the_outputs_at_their_sentinels(engine):
    """ZIGP_EARG naming the argument, through the C-ABI: elbo_data, kl, every gradient buffer and the predict block keep their sentinels."""
    import ctypes as C
    from zigp import _lib
    from zigp.engine import _Packed, head_placeholder
    X, Y, p = _problem(37, 3, 'diag', 'rbf', 'zero')
    engine.set_whiten(False); engine.set_q_full(False); engine.set_kernel(0, 'rbf'); engine._set_mean_function({}, 3)
    engine.set_data(X, Y)
    lib, ctx = engine.lib, engine.ctx
    SENT = -7.25

    def call_elbo(pk, lik, rows=(0, N_ROWS), jitter=JIT):
        ed, kl = C.c_double(SENT), C.c_double(SENT)
        g = dict(Zf=np.full((37, 3), SENT), u_fm=np.full(37, SENT), u_fs_sqrt=np.full(37, SENT), ell_f=np.full(3, SENT))
        gs = _lib.zigp_grads()
        for k, a in g.items():
            setattr(gs, k, a.ctypes.data)
        gs.var_f = gs.var_g = gs.noise = SENT
        rc = lib.zigp_head_elbo(ctx, C.byref(pk.struct) if pk is not None else None, lik, jitter, 1.0, rows[0], rows[1], 1, C.byref(ed), C.byref(kl),
                                C.byref(gs))
        untouched = ed.value == SENT and kl.value == SENT and all(np.all(a == SENT) for a in g.values()) and gs.var_f == SENT and gs.noise == SENT \
            and gs.var_g == SENT
        return rc, (lib.zigp_last_error(ctx) or b'').decode(), untouched

    def call_predict(pk, lik):
        out = np.full((4, 50), SENT)
        rc = lib.zigp_head_predict(ctx, C.byref(pk.struct), lik, X[:50].ctypes.data, 50, JIT, out.ctypes.data)
        return rc, (lib.zigp_last_error(ctx) or b'').decode(), bool(np.all(out == SENT))

    def packed(**over):
        return _Packed(dict(dict(p, **head_placeholder(3)), **over))

    ok = packed()
    rc, msg, untouched = call_elbo(ok, _lib.LIK_GAUSSIAN)
    assert rc == 0 and not untouched                                           # the harness itself: a good call fills everything
    for lik in (_lib.LIK_ONOFF, 3, -1):
        for rc, msg, untouched in (call_elbo(ok, lik), call_predict(ok, lik)):
            assert rc == _lib.ZIGP_EARG and 'lik' in msg and untouched, (lik, msg)
    bad = [(packed(var_f=0.0), 'var_f'), (packed(noise=-1.0), 'noise'), (packed(ell_f=np.array([0.3, 0.0, 0.3])), 'ell_f'),
           (packed(u_fs_sqrt=np.r_[-1.0, np.ones(36)]), 'u_fs_sqrt')]
    for pk, word in bad:
        for rc, msg, untouched in (call_elbo(pk, _lib.LIK_GAUSSIAN), call_predict(pk, _lib.LIK_GAUSSIAN)):
            assert rc == _lib.ZIGP_EARG and word in msg and untouched, (word, msg)
    rc, msg, untouched = call_elbo(packed(noise=-1.0), _lib.LIK_BERNOULLI)      # the Bernoulli head does not read the noise
    assert rc == 0
    nul = packed()
    nul.struct.Zf = None
    rc, msg, untouched = call_elbo(nul, _lib.LIK_GAUSSIAN)
    assert rc == _lib.ZIGP_EARG and 'Zf' in msg and untouched
    rc, msg, untouched = call_elbo(None, _lib.LIK_GAUSSIAN)
    assert rc == _lib.ZIGP_EARG and 'params' in msg and untouched
    rc, msg, untouched = call_elbo(ok, _lib.LIK_GAUSSIAN, rows=(5, N_ROWS + 1))
    assert rc == _lib.ZIGP_EARG and 'row range' in msg and untouched
    rc, msg, untouched = call_elbo(ok, _lib.LIK_GAUSSIAN, jitter=-1.0)
    assert rc == _lib.ZIGP_EARG and 'jitter' in msg and untouched
    engine.set_q_full(True)                                                     # q_full without whitening, as zigp_elbo refuses it
    rc, msg, untouched = call_elbo(ok, _lib.LIK_GAUSSIAN)
    engine.set_q_full(False)
    assert rc == _lib.ZIGP_EARG and 'zigp_set_q_full' in msg and untouched
    engine.set_kernel(0, 'matern52')                                            # a Matern f at D = 9; latent g's kernel is not read
    X9 = np.random.RandomState(0).rand(64, 9)
    engine.set_data(X9, np.zeros(64))
    p9 = _Packed(dict(Zf=X9[:5], u_fm=np.zeros(5), u_fs_sqrt=np.ones(5), ell_f=np.ones(9), var_f=1.0, noise=0.1, **head_placeholder(9)))
    ed, kl = C.c_double(SENT), C.c_double(SENT)
    rc = lib.zigp_head_elbo(ctx, C.byref(p9.struct), _lib.LIK_GAUSSIAN, JIT, 1.0, 0, 64, 1, C.byref(ed), C.byref(kl), None)
    assert rc == _lib.ZIGP_EARG and 'Matern' in (lib.zigp_last_error(ctx) or b'').decode() and ed.value == SENT and kl.value == SENT
    engine.set_kernel(0, 'rbf'); engine.set_kernel(1, 'matern52')
    rc = lib.zigp_head_elbo(ctx, C.byref(p9.struct), _lib.LIK_GAUSSIAN, JIT, 1.0, 0, 64, 1, C.byref(ed), C.byref(kl), None)
    engine.set_kernel(1, 'rbf')
    assert rc == 0 and np.isfinite(ed.value)
    with pytest.raises(ValueError):
        engine.head_elbo(p, 'onoff')
    # the context is as usable as before
    engine.set_data(X, Y)
    assert np.isfinite(engine.head_elbo(p, 'gaussian')[0])


def test_a_communicator_refuses_the_heads():
    """zigp_comm_init attached: ZIGP_EARG naming the communicator, nothing enqueued; after zigp_comm_destroy the same call runs.  A one-rank
    communicator, in a process of its own (as every test that enters RCCL: tests/test_gpu_bench_launch.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import os, sys\n"
        "sys.path[:0] = [%r, %r, %r]\n"
        "import numpy as np, zigp\n"
        "from conftest import make_problem\n"
        "X, Y, p = make_problem(300, 12, 2, seed=3)\n"
        "e = zigp.DenseEngine(0)\n"
        "assert e.comm_available()\n"
        "e.comm_set_timeout(60.0)\n"
        "e.comm_init(0, 1, e.comm_unique_id())\n"
        "e.set_data(X, Y)\n"
        "for call in (lambda: e.head_elbo(p, 'gaussian'), lambda: e.head_predict(p, X[:10], 'bernoulli')):\n"
        "    try:\n"
        "        call(); print('NO ERROR'); sys.stdout.flush(); os._exit(3)\n"
        "    except ValueError as err:\n"
        "        assert 'communicator' in str(err), str(err)\n"
        "e.comm_destroy()\n"
        "assert np.isfinite(e.head_elbo(p, 'gaussian')[0])\n"
        "print('heads refused under a communicator'); sys.stdout.flush()\n"
        "os._exit(0)\n" % (os.path.join(root, 'zero-inflated-gp_amd'), os.path.join(root, 'tests'), os.path.join(root, 'oracle')))
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0 and 'heads refused under a communicator' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# =====================================================================================================================================
# onoffgpf.SVGP
# =====================================================================================================================================
def _toy(n=400, seed=0):
    """1-D zero-inflated toy data: a sine where a slow square wave is on, exact zeros elsewhere"""
    rs = np.random.RandomState(seed)
    X = np.sort(rs.rand(n, 1) * 10.0, axis=0)
    on = np.sin(0.9 * X[:, 0]) > -0.2
    Y = np.where(on, 1.5 + np.sin(2.0 * X[:, 0]) + 0.1 * rs.randn(n), 0.0)[:, None]
    return X, Y


def test_svgp_fits_the_toy_data_and_the_hurdle_recipe_runs(engine):
    """200 L-BFGS-B iterations raise the bound of both heads, predict_density is finite, and the hurdle recipe of scripts/hurdle.py:49-50
    -- a Bernoulli SVGP on Y != 0, then a Gaussian SVGP on the rows it switches on -- runs end to end."""
    from onoffgpf import SVGP, kernels, likelihoods
    X, Y = _toy()
    Z = np.linspace(0.0, 10.0, 20)[:, None]
    clf = SVGP(X, (Y != 0) * 1.0, kernels.RBF(1, lengthscales=1.0), likelihoods.Bernoulli(), Z.copy())
    b0 = clf.compute_log_likelihood()
    clf.optimize(maxiter=200)
    b1 = clf.compute_log_likelihood()
    print('HEAD-SVGP bernoulli bound %.4f -> %.4f, KL %.4f' % (b0, b1, clf.compute_prior_KL()))
    assert b1 > b0 and clf.compute_prior_KL() > 0
    pm, pv = clf.predict_y(X)
    on = pm[:, 0] > 0.5                                                        # hurdle.py:49-50
    assert 0.3 * len(X) < on.sum() < len(X) and np.mean(on == (Y[:, 0] != 0)) > 0.9
    assert np.all(np.isfinite(clf.predict_density(X, (Y != 0) * 1.0)))
    reg = SVGP(X[on], Y[on], kernels.Matern52(1, lengthscales=1.0), likelihoods.Gaussian(), Z.copy(), q_diag=True, whiten=False)
    r0 = reg.compute_log_likelihood()
    reg.optimize(maxiter=200)
    r1 = reg.compute_log_likelihood()
    print('HEAD-SVGP gaussian bound %.4f -> %.4f, noise %.4g' % (r0, r1, float(reg.likelihood.variance.value[0])))
    assert r1 > r0
    fm, fv = reg.predict_f(X)
    ym, yv = reg.predict_y(X)
    assert np.array_equal(fm, ym) and np.all(yv > fv) and np.all(fv > 0)
    ld = reg.predict_density(X[on], Y[on])
    assert ld.shape == (on.sum(), 1) and np.all(np.isfinite(ld))
    hurdle_mean = np.where(on, ym[:, 0], 0.0)                                  # the hurdle model's prediction of y
    assert np.sqrt(np.mean((hurdle_mean - Y[:, 0]) ** 2)) < 0.5 * np.std(Y)
    reg.optimize(method='adam', maxiter=5, learning_rate=0.01)                 # the host Adam loop, minibatches included
    mb = SVGP(X, Y, kernels.RBF(1), likelihoods.Gaussian(), Z.copy(), minibatch_size=100)
    mb.optimize(method='adam', maxiter=5)
    assert np.isfinite(mb.compute_log_likelihood())
