"""Stage-level parity of the dense M x M reverse stage (latent_mxm_backward, latent_mxm_backward_white) through
engine.test_mxm_backward: the chain of split-K products with its taps, one launch at a time.

  exact tier   integer operands (stage_ref.mxm_int_operands; tests/test_cpu_stage_ref.py pins that the float64 chain on them is exact):
               every tap and every output must be np.array_equal to the numpy chain, at the sizes that reach each slice count of
               run_gemm_sk (nb = 1, 2, 3: S = 8 everywhere; nb = 9: 6 and 8 within one chain; nb = 12: 3 and 6).
  bound tier   normal operands: every launch against the operands ITS kernel read (the taps) within its stage_ref bound; the largest
               error-to-bound ratio per launch is printed as a STAGE-LOG line (profiles/mxm_stage_parity.log keeps a run's).
"""
import numpy as np
import pytest

import stage_ref as sr

pytestmark = pytest.mark.gpu

OUTPUTS = ('a1gm', 'du', 'dsq', 'G', 'dLq', 'krow')


def _call(engine, op, mode, with_data=True, with_kl=True, P=None, pad=0.0, krow=None):
    return engine.test_mxm_backward(op['W'], op['L'], op['Kuu'], op['Z'], op['s'], op['alpha'], C1=op['C1'] if with_data else None, v=op['v'],
                                    u=op['u'], P=P, mode=mode, with_data=with_data, with_kl=with_kl, jitter=op['jitter'],
                                    krow=op['krow'] if krow is None else krow, pad=pad)


def _flat(got):
    """{launch name: what the GPU left}: the taps and the outputs under the names stage_ref.mxm_backward uses."""
    d = dict(got['taps'])
    d.update({k: got[k] for k in OUTPUTS if k in got})
    return d


def _where(name, a, b):
    bad = np.argwhere(a != b)
    k = tuple(int(x) for x in bad[0])
    loc = sr.locate(k[-2], k[-1]) if a.ndim >= 2 and name != 'krow' else str(k)
    return 'launch %s: %d elements differ, first at %s: gpu %r, reference %r' % (name, len(bad), loc, a[k], b[k])


def _assert_exact(tag, got, ref, with_data, mode):
    g = _flat(got)
    for name, (val, _) in ref.items():
        assert name in g, (tag, name)
        assert np.array_equal(g[name], val), '%s %s' % (tag, _where(name, g[name], val))
    M = got['G'].shape[0]
    if not with_data:
        assert not got['a1gm'].any() and not got['du'].any() and not got['dsq'].any() and not set(got['taps']) - {'P', 'PSP'}
    if mode != 'diag':
        assert not got['du'].any(), 'the whitened stage relies on du being zero and must leave it so'
    return M


def _assert_structure(got):
    """R and Q W: zero in every tile above the diagonal, computed in full inside the diagonal tiles; Q = tril(., -1) + diag / 2 (nothing
    above the diagonal); dL zero above the diagonal; G symmetric to the bit."""
    t, M = got['taps'], got['G'].shape[0]
    up = ~sr.lower_tiles(M)
    for name in ('R', 'QW'):
        assert not t[name][up].any(), name
    # R = W^T V is not triangular: the diagonal tiles are stored in full (Q W, a product of two lower-triangular factors, is triangular anyway)
    assert np.triu(t['R'][:min(M, 128), :min(M, 128)], 1).any(), 'R: nothing above the diagonal inside the diagonal tile'
    assert not np.triu(t['Q'], 1).any() and not np.triu(t['dL'], 1).any()
    assert np.array_equal(got['G'], got['G'].T)


_REF = {}


def _ref(M, D, mode, with_data, with_kl, P):
    key = (M, D, mode, with_data, with_kl, P)
    if key not in _REF:
        op = sr.mxm_int_operands(M, D, seed=sr.mxm_int_seed(M, D), mode=mode)
        Pm = op['W'].T @ op['W'] if P else None
        _REF[key] = (op, Pm, sr.mxm_backward(dict(op, P=Pm), mode, with_data, with_kl))
    return _REF[key]


FLAGS = [(1, 1), (1, 0), (0, 1)]
CASES = [(M, mode, f, P) for M in (9, 127, 128, 129, 300) for mode in sr.MXM_MODES for f in FLAGS
         for P in ((False, True) if mode == 'diag' and f[1] else (False,))]
CASES += [(M, mode, (1, 1), P) for M in (1100, 1536) for mode in sr.MXM_MODES for P in ((False, True) if mode == 'diag' else (False,))]


@pytest.mark.parametrize('M,mode,flags,P', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_reverse_stage_exact(engine, M, mode, flags, P):
    """Every tap and output bit-equal to the numpy chain on the integer operands.  nb = 1, 1, 1, 2, 3 run every product at S = 8; M = 1100
    (nb = 9) is the first size whose products disagree on S (6 for "y", "tt", "full", "s"; 8 for "r", "rfull", "t") and is ragged against
    its padding; M = 1536 (nb = 12) brings 3 and 6.  All of them share the plane buffer Latent::sk."""
    with_data, with_kl = bool(flags[0]), bool(flags[1])
    op, Pm, ref = _ref(M, 3, mode, with_data, with_kl, P)
    got = _call(engine, op, mode, with_data, with_kl, P=Pm)
    tag = 'M=%d %s data=%d kl=%d P=%s' % (M, mode, with_data, with_kl, 'given' if P else 'formed')
    _assert_exact(tag, got, ref, with_data, mode)
    if with_data:
        _assert_structure(got)
    nb = sr.round_up(M, 128) // 128
    covered = sorted({(sr.MXM_PRODUCTS[mode][n], sr.sk_slices(sr.MXM_PRODUCTS[mode][n], nb)) for n in got['taps'] if n in sr.MXM_PRODUCTS[mode]})
    print('STAGE-LOG mxm-exact    %-44s bit-equal; nb=%d (product, S): %s' % (tag, nb, covered))


def test_the_sizes_reach_every_slice_count():
    """What the exact tier's sizes cover, from the restated slice rule: S = 8 alone up to nb = 8, {6, 8} at nb = 9, {3, 6} at nb = 12."""
    def counts(M):
        nb = sr.round_up(M, 128) // 128
        return {sr.sk_slices(n, nb) for n in set(sr.MXM_PRODUCTS['diag'].values()) | {'rfull'}}
    assert [counts(M) for M in (9, 127, 128, 129, 300)] == [{8}] * 5 and counts(1100) == {6, 8} and counts(1536) == {3, 6}


@pytest.mark.parametrize('mode', sr.MXM_MODES)
def test_krow_is_added_to_and_the_padding_is_left_alone(engine, mode):
    """krow with non-zero initial values in every slab, row and column: the stage ADDS its sums to slab 0, rows < M, and writes nothing
    else -- the rows M .. Mp of the device buffer come back as they went in.  Then pad hygiene: with the padding of Z, Kuu, s, C1 and of
    K gm (krow's rows >= M) holding numbers instead of zeros, every M x M result and every real row of krow keep their bits."""
    M, D = 300, 3
    op, _, _ = _ref(M, D, mode, True, True, False)
    rs = np.random.RandomState(5)
    krow = rs.randint(-3, 4, op['krow'].shape).astype(np.float64)
    krow[:, :M, 1 + 2 * D] = op['krow'][:, :M, 1 + 2 * D]           # the same K gm
    krow[:, M:] = 0.0
    ref = sr.mxm_backward(dict(op, krow=krow), mode)
    got = _call(engine, op, mode, krow=krow)
    _assert_exact('initial krow', got, ref, True, mode)
    assert not got['krow'][:, M:].any() and np.array_equal(got['krow'][1:], krow[1:])
    junk = krow.copy()
    junk[:, M:] = rs.randint(1, 6, junk[:, M:].shape)
    got2 = _call(engine, op, mode, krow=junk, pad=3.0)
    assert np.array_equal(got2['krow'][:, M:], junk[:, M:]), 'the stage wrote to the padded rows of krow'
    a, b = _flat(got), _flat(got2)
    for name in a:
        x, y = (a[name][:, :M], b[name][:, :M]) if name == 'krow' else (a[name], b[name])
        assert np.array_equal(x, y), 'padding leaked into the result: ' + _where(name, y, x)


@pytest.mark.parametrize('D', [1, 3, 8, 9, 17, 64])
def test_kuu_grad_every_dimension_exact(engine, D):
    """k_kuu_grad (D = 1, 3, 8) and k_kuu_grad_wide (D = 9: one partial window past the first; 17: two full windows plus one; 64: eight full
    windows) on integer G, Kuu, Z: krow bit-equal, with initial values in krow."""
    M = 300
    op, _, _ = _ref(M, D, 'diag', True, True, False)
    krow = op['krow'].copy()
    krow[0, :M, :1 + 2 * D] = np.random.RandomState(D).randint(-2, 3, (M, 1 + 2 * D))
    ref = sr.mxm_backward(dict(op, krow=krow), 'diag')
    got = _call(engine, op, 'diag', krow=krow)
    _assert_exact('D=%d' % D, got, ref, True, 'diag')
    assert np.count_nonzero(got['krow'][0, :M] - krow[0, :M]) > 0.5 * M * (1 + 2 * D)


def _normal_operands(M, D, seed, mode):
    rs = np.random.RandomState(seed)
    W = np.tril(rs.randn(M, M)) / np.sqrt(M) + np.eye(M)
    L = np.tril(rs.randn(M, M)) / np.sqrt(M) + np.eye(M)
    B = rs.randn(M, M)
    Kuu = rs.randn(M, M)
    krow = np.zeros((sr.KG_SPLIT, sr.round_up(M, 128), 2 + 2 * D))
    krow[:, :M] = rs.randn(sr.KG_SPLIT, M, 2 + 2 * D)
    op = dict(W=W, L=L, Kuu=Kuu + Kuu.T, Z=rs.rand(M, D), C1=B + B.T, krow=krow, jitter=1e-6, alpha=rs.randn(M), v=rs.randn(M), u=rs.randn(M))
    op['s'] = np.tril(rs.randn(M, M)) / np.sqrt(M) + np.diag(0.3 + rs.rand(M)) if mode == 'white_full' else 0.3 + rs.rand(M)
    return op


def _assert_bound(engine, stage, got, op, mode, with_data=True, with_kl=True, P=None):
    """Every launch against the operands its kernel read: stage_ref.mxm_backward with given = the GPU's taps and outputs."""
    g = _flat(got)
    if mode == 'white_full' and 'Rt' not in op:      # the factor image the "rfull" launch read: the forward stage's own (same kernels, same bits)
        op['Rt'] = engine.test_q_full_forward(op['W'], op['s'], op['u'])[1]
    ref = sr.mxm_backward(dict(op, P=P), mode, with_data, with_kl, given=g)
    worst = {}
    for name, (val, bnd) in ref.items():
        r, k = sr.worst(np.abs(g[name] - val), bnd)
        worst[name] = r
        what = sr.MXM_PRODUCTS[mode].get(name, 'element-wise / reduction')
        print('STAGE-LOG %-12s %-34s max error / bound = %.4g' % (stage, '%s launch %s (%s)' % (mode, name, what), r))
        assert r <= 1.0, (stage, name, r, k)
    return worst


@pytest.mark.parametrize('D', [1, 3, 8, 9, 17, 64])
def test_kuu_grad_every_dimension_bound(engine, D):
    M = 300
    op = _normal_operands(M, D, 40 + D, 'diag')
    got = _call(engine, op, 'diag')
    _assert_bound(engine, 'mxm-D=%d' % D, got, op, 'diag')


@pytest.mark.parametrize('mode', sr.MXM_MODES)
@pytest.mark.parametrize('M', [136, 300, 1100])
def test_reverse_stage_bound_normal_operands(engine, M, mode):
    """Normal operands at nb = 2, 3 and 9, with and without a supplied P, with and without rows."""
    op = _normal_operands(M, 3, 7 + M, mode)
    got = _call(engine, op, mode)
    _assert_bound(engine, 'mxm-M=%d' % M, got, op, mode)
    _assert_structure(got)
    if M == 300:
        if mode == 'diag':
            P = op['W'].T @ op['W']
            _assert_bound(engine, 'mxm-M=%d-P' % M, _call(engine, op, mode, P=P), op, mode, P=P)
        _assert_bound(engine, 'mxm-M=%d-nodata' % M, _call(engine, op, mode, with_data=False), op, mode, with_data=False)
        _assert_bound(engine, 'mxm-M=%d-nokl' % M, _call(engine, op, mode, with_kl=False), op, mode, with_kl=False)


def test_calls_do_not_depend_on_what_ran_before(engine):
    """An unwhitened call (which writes du), then a whitened one (which relies on du being zero), then the unwhitened one again, on one
    context: each equals, bit for bit, what a fresh context gives for the same call."""
    import zigp
    M = 300
    ops = {mode: _normal_operands(M, 3, 90, mode) for mode in ('diag', 'white')}
    seq = ['diag', 'white', 'diag']
    here = [_flat(_call(engine, ops[m], m)) for m in seq]
    for i, m in enumerate(seq):
        fresh = zigp.DenseEngine(0)
        try:
            alone = _flat(_call(fresh, ops[m], m))
        finally:
            fresh.close()
        for name in alone:
            assert np.array_equal(here[i][name], alone[name]), 'call %d (%s): %s' % (i, m, _where(name, here[i][name], alone[name]))
    assert here[0]['du'].any() and not here[1]['du'].any()


def test_mxm_stage_calls_leave_the_context_usable(engine):
    """Two identical engine.elbo gradient calls with every new diagnostic run between them return identical bits: the reverse stage in
    its three modes; the pack in its three modes, with and without need_grad and with mean_on (it overwrites the latents' sizes,
    variances, small vectors and accumulators and switches the context's mean function for the launch); the forward stage unwhitened and
    whitened (it switches the context's parametrisation) and its refused full-covariance call."""
    import fullcov_ref
    from conftest import make_problem
    X, Y, p = make_problem(2000, 96, 3, seed=7)
    engine.set_data(X, Y)
    first = engine.elbo(p, jitter=1e-6)
    for mode in sr.MXM_MODES:
        op, Pm, _ = _ref(129, 3, mode, True, True, False)
        _call(engine, op, mode)
        _call(engine, op, mode, with_data=False)
        lat = [_pack_operands(M, 3, M, mode) for M in (137, 60)]
        pw = np.random.RandomState(3).randn(40, 13)
        for need_grad in (True, False):
            engine.test_dense_pack(lat[0], lat[1], pw, 3, mode, need_grad=need_grad)
        engine.test_dense_pack(lat[0], lat[1], pw, 3, mode, include_kl=False, mean_on=True)
    op = _normal_operands(200, 9, 3, 'diag')
    _call(engine, op, 'diag', P=op['W'].T @ op['W'])
    _, _, q = make_problem(8, 150, 3, seed=4, Mg=40, ell=0.1)
    for white in (False, True):
        for need_grad in (True, False):
            engine.test_latents_forward(dict(q, whiten=white), 1e-4, need_grad)
    with pytest.raises(ValueError):
        engine.test_latents_forward(fullcov_ref.make_lq(q), 1e-4, True)
    second = engine.elbo(p, jitter=1e-6)
    assert first[0] == second[0] and first[1] == second[1]
    for k in first[2]:
        assert np.array_equal(np.asarray(first[2][k]), np.asarray(second[2][k])), k


def test_mxm_entry_point_validates_its_arguments(engine):
    """NULL context, M <= 0, D outside 1 .. ZIGP_MAX_D, a mode outside 0 .. 2, a missing operand, a zero on the diagonal of s or Lq: each
    is refused with ZIGP_EARG, and the context goes on working."""
    import ctypes
    from zigp import _lib
    lib = engine.lib
    assert lib.zigp_test_mxm_backward(None, None) == _lib.ZIGP_EARG
    assert lib.zigp_test_mxm_backward(engine.ctx, None) == _lib.ZIGP_EARG
    op, _, ref = _ref(9, 3, 'diag', True, True, False)
    a = _lib.zigp_stage_mxm()
    keep = {k: np.ascontiguousarray(op[k]) for k in ('W', 'L', 'Kuu', 'Z', 's', 'alpha', 'v', 'C1', 'krow')}
    for k, x in keep.items():
        setattr(a, k, _lib.ptr(x))
    a.M, a.D, a.mode, a.with_data, a.with_kl, a.jitter = 9, 3, 0, 1, 1, 0.5

    def refused(**kw):
        b = _lib.zigp_stage_mxm()
        ctypes.memmove(ctypes.byref(b), ctypes.byref(a), ctypes.sizeof(a))
        for k, v in kw.items():
            setattr(b, k, v)
        return lib.zigp_test_mxm_backward(engine.ctx, ctypes.byref(b)) == _lib.ZIGP_EARG

    assert refused(M=0) and refused(M=-3) and refused(D=0) and refused(D=_lib.MAX_D + 1) and refused(mode=3) and refused(mode=-1)
    assert refused(W=None) and refused(C1=None) and refused(v=None) and refused(krow=None) and refused(jitter=-1.0)
    s0 = op['s'].copy()
    s0[4] = 0.0
    with pytest.raises(ValueError):
        _call(engine, dict(op, s=s0), 'diag')
    opf, _, _ = _ref(9, 3, 'white_full', True, True, False)
    Lq0 = opf['s'].copy()
    Lq0[7, 7] = 0.0
    with pytest.raises(ValueError):
        _call(engine, dict(opf, s=Lq0), 'white_full')
    _assert_exact('after the refusals', _call(engine, op, 'diag'), ref, True, 'diag')


# =====================================================================================================================================
# the M x M forward stage behind the factorisation (zigp_test_latents_forward)
# =====================================================================================================================================
FWD_SHAPES = [(9, 9), (127, 129), (300, 100), (100, 520), (1100, 136)]


@pytest.mark.parametrize('white', [False, True], ids=['diag', 'white'])
@pytest.mark.parametrize('shape', FWD_SHAPES, ids=lambda s: '%dx%d' % s)
def test_forward_stage_outputs(engine, shape, white):
    """v, alpha, dkinv, the KL scalar, P, Qt, Wp, Rt, Wt (whitened: wh, its KL, alpha = W^T u, D W) against their one-line statements applied
    to the W and L the GPU produced.  "rt" and "s" are k-restricted like the reverse products; the unequal pairs run the two alternating
    streams at different chain lengths (1100 x 136: nb = 9 and 2, S = 6 against 8)."""
    from conftest import make_problem
    Mf, Mg = shape
    _, _, p = make_problem(8, Mf, 3, seed=Mf + Mg, Mg=Mg, ell=0.1)
    p = dict(p, whiten=white)
    jitter = 1e-4
    outs = engine.test_latents_forward(p, jitter, True)
    again = engine.test_latents_forward(p, jitter, True)
    for h, tag in enumerate('fg'):
        o = outs[h]
        M = shape[h]
        for k in o:
            assert (o[k] is None) == (again[h][k] is None) and (o[k] is None or np.array_equal(o[k], again[h][k])), 'forward not bit-stable: ' + k
        u, s = p['u_%sm' % tag].reshape(-1), p['u_%ss_sqrt' % tag].reshape(-1)
        ref = sr.mxm_forward(o['W'], o['L'], u, s, white=white, given=o)
        assert set(ref) == {k for k in o if o[k] is not None} - {'W', 'L', 'Kuu'}, sorted(ref)
        for name, (val, bnd) in ref.items():
            r, k = sr.worst(np.abs(np.asarray(o[name]) - val), bnd)
            print('STAGE-LOG %-12s %-34s max error / bound = %.4g' % ('mxm-fwd', '%s %s M=%d %s' % ('white' if white else 'diag', tag, M, name), r))
            assert r <= 1.0, (tag, name, r, k)
    if not white:          # the value-only forward leaves the same v, alpha, dkinv, KL
        vo = engine.test_latents_forward(p, jitter, False)
        for h in range(2):
            for k in ('W', 'L', 'v', 'alpha', 'dkinv'):
                assert np.array_equal(vo[h][k], outs[h][k]), k
            assert vo[h]['kl'] == outs[h]['kl'] and vo[h]['Rt'] is None and vo[h]['P'] is None


def test_forward_stage_refuses_a_full_covariance_call_and_keeps_the_context(engine):
    from conftest import make_problem
    import fullcov_ref
    _, _, p = make_problem(8, 20, 2, seed=1, Mg=12)
    with pytest.raises(ValueError):
        engine.test_latents_forward(fullcov_ref.make_lq(p), 1e-6, True)
    assert engine.test_latents_forward(p, 1e-6, True)[0]['P'] is not None


# =====================================================================================================================================
# k_dense_pack (zigp_test_dense_pack)
# =====================================================================================================================================
def _pack_operands(M, D, seed, mode):
    rs = np.random.RandomState(seed)
    q = dict(krow=rs.randn(sr.KG_SPLIT, M, 2 + 2 * D), du=rs.randn(M), kl_vec1=rs.randn(M), kl_vec2=rs.rand(M) + 0.1, ell=0.2 + rs.rand(D),
             var=0.5 + rs.rand(), kl=rs.rand())
    if mode == 'white_full':
        q['dLq'] = np.tril(rs.randn(M, M))
    else:
        q.update(dsq=rs.randn(M), s=(0.3 + rs.rand(M)) * rs.choice([-1.0, 1.0], M) if mode == 'diag' else 0.3 + rs.rand(M))
    return q


def _assert_pack(stage, pk, ref):
    for name, (val, bnd) in ref.items():
        got = pk[name[0]][name[1:]] if name[0] in 'fg' and name[1:] in ('dZ', 'du', 'ds', 'dell') else pk[name]
        r, k = sr.worst(np.abs(np.asarray(got) - val), bnd)
        print('STAGE-LOG %-12s %-34s max error / bound = %.4g' % (stage, name, r))
        assert r <= 1.0, (stage, name, r, k)


@pytest.mark.parametrize('include_kl', [1, 0], ids=['kl', 'nokl'])
@pytest.mark.parametrize('mode', sr.MXM_MODES)
@pytest.mark.parametrize('D', [2, 8, 17])
def test_dense_pack_blocks(engine, D, mode, include_kl):
    """dZ, du, ds (or the dLq block), dell, d var and the header from random accumulators, Mf != Mg, more point-wise blocks than threads."""
    lat = [_pack_operands(M, D, 10 * D + M, mode) for M in (137, 300)]
    pw = np.random.RandomState(D).randn(300, 13)
    pk = engine.test_dense_pack(lat[0], lat[1], pw, D, mode, include_kl=bool(include_kl))
    _assert_pack('pack-D=%d-%s-kl%d' % (D, mode, include_kl), pk, sr.dense_pack_ref(lat[0], lat[1], pw, D, mode, bool(include_kl)))
    assert not pk['mean_a'].any() and pk['mean_b'] == 0.0 and not pk['packed'][14:16].any()
    vo = engine.test_dense_pack(lat[0], lat[1], pw, D, mode, need_grad=False, include_kl=bool(include_kl))
    assert vo['packed'].shape == (16,) and vo['data'] == pk['data'] and vo['kl'] == pk['kl'] and vo['var_f'] == 0.0 and vo['var_g'] == 0.0
    if D <= 8:
        mo = engine.test_dense_pack(lat[0], lat[1], pw, D, mode, include_kl=bool(include_kl), mean_on=True)
        assert np.allclose(mo['mean_b'], pw[:, 4].sum(), rtol=1e-12, atol=1e-12) and np.allclose(mo['mean_a'][:D], pw[:, 5:5 + D].sum(0), rtol=1e-12, atol=1e-12)
        assert not mo['mean_a'][D:].any() and np.array_equal(mo['packed'][16:], pk['packed'][16:])


def test_dense_pack_validates_its_arguments(engine):
    from zigp import _lib
    assert engine.lib.zigp_test_dense_pack(None, None) == _lib.ZIGP_EARG
    assert engine.lib.zigp_test_dense_pack(engine.ctx, None) == _lib.ZIGP_EARG
    lat = [_pack_operands(M, 2, M, 'diag') for M in (5, 9)]
    pw = np.zeros((4, 13))
    with pytest.raises(ValueError):
        engine.test_dense_pack(lat[0], lat[1], pw, _lib.MAX_D + 1)
    with pytest.raises(ValueError):
        engine.test_dense_pack(dict(lat[0], s=np.zeros(5)), lat[1], pw, 2)
    with pytest.raises(ValueError):
        engine.test_dense_pack(dict(lat[0], krow=None), lat[1], pw, 2)
    with pytest.raises(ValueError):
        engine.test_dense_pack(lat[0], lat[1], pw, 9, mean_on=True)
    assert engine.test_dense_pack(lat[0], lat[1], pw, 2)['f']['dZ'].shape == (5, 2)


# =====================================================================================================================================
# the stages composed: chunk stages -> reverse stage (with taps) -> pack, against the real step
# =====================================================================================================================================
COMPOSED = [dict(N=2900, Mf=100, Mg=136, Nc=3072, ell=0.3, jitter=1e-6, seed=21), dict(N=1000, Mf=300, Mg=1100, Nc=1024, ell=0.08, jitter=1e-4, seed=5)]


@pytest.mark.parametrize('c', COMPOSED, ids=lambda c: '%dx%d' % (c['Mf'], c['Mg']))
def test_composed_gradient_is_the_real_step(engine, c):
    """The real C1 and krow of the chunk stages (test_gpu_stages._compose) through the reverse stage with taps, every launch within its
    bound against the operands it read, and its results through the pack diagnostic: the SAME kernels on the SAME doubles as engine.elbo,
    with only the diagnostics' host round trips between them -- so the data term, the KL and every gradient block are asserted bit-equal
    to the real step."""
    from conftest import make_problem
    from test_gpu_stages import _compose
    X, Y, p = make_problem(c['N'], c['Mf'], 3, seed=c['seed'], Mg=c['Mg'], ell=c['ell'])
    D, jitter = X.shape[1], c['jitter']
    engine.set_data(X, Y)
    ed, kl, g = engine.elbo(p, jitter=jitter)
    a = _compose(engine, X, Y, p, c['Nc'], True, jitter)
    fwd = engine.test_latents_forward(p, jitter, True)
    lat = []
    for h, tag in enumerate('fg'):
        f = fwd[h]
        M = f['W'].shape[0]
        s = p['u_%ss_sqrt' % tag].reshape(-1)
        krow = np.zeros((sr.KG_SPLIT, sr.round_up(M, 128), 2 + 2 * D))
        krow[:, :M] = a['krow_' + tag]
        op = dict(W=f['W'], L=f['L'], Kuu=f['Kuu'], Z=p['Z' + tag], s=s, alpha=f['alpha'], v=f['v'], u=p['u_%sm' % tag].reshape(-1),
                  C1=a['C1_' + tag], krow=krow, jitter=jitter)
        got = _call(engine, op, 'diag', P=f['P'])
        _assert_bound(engine, 'compose-%s%d' % (tag, M), got, op, 'diag', P=f['P'])
        _assert_structure(got)
        lat.append(dict(krow=got['krow'][:, :M], du=got['du'], dsq=got['dsq'], s=s, kl_vec1=f['alpha'], kl_vec2=f['dkinv'], ell=p['ell_' + tag],
                        var=p['var_' + tag], kl=f['kl']))
    pk = engine.test_dense_pack(lat[0], lat[1], a['acc'], D, 'diag')
    pairs = [('data', pk['data'], ed), ('kl', pk['kl'], kl), ('var_f', pk['var_f'], g['var_f']), ('var_g', pk['var_g'], g['var_g']), ('noise', pk['noise'], g['noise'])]
    for tag in 'fg':
        pairs += [('Z' + tag, pk[tag]['dZ'], g['Z' + tag]), ('u_%sm' % tag, pk[tag]['du'], g['u_%sm' % tag]),
                  ('u_%ss_sqrt' % tag, pk[tag]['ds'], g['u_%ss_sqrt' % tag]), ('ell_' + tag, pk[tag]['dell'], g['ell_' + tag])]
    same = {}
    for name, mine, real in pairs:
        mine, real = np.asarray(mine, dtype=np.float64).reshape(-1), np.asarray(real, dtype=np.float64).reshape(-1)
        same[name] = bool(np.array_equal(mine, real))
        rel = float(np.max(np.abs(mine - real)) / max(np.max(np.abs(real)), 1e-300))
        print('STAGE-LOG %-12s %-34s bit-equal to engine.elbo: %s (rel diff %.3g)' % ('composition', '%dx%d %s' % (c['Mf'], c['Mg'], name), same[name], rel))
    assert all(same.values()), sorted(k for k, v in same.items() if not v)
