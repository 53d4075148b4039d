"""Stage-level parity of the update kernels of the device fit loops: k_fit_update<false> / k_fit_update<true> (csrc/zigp_kronf.hip; the
loops of zigp_kron_fit_steps / zigp_kron_head_fit_steps) and k_dense_fit_image, k_dense_fit_image_tri, k_dense_fit_update
(csrc/zigp_kernels.h; zigp_fit_steps[_mode]).  DenseEngine.test_kron_fit_update / test_dense_fit_update (include/zigp_diag.h) run the host
loops themselves -- descriptor, grid, launches, lr factors, download, failure decoding -- with every gradient step replaced by a
caller-supplied result, and snapshot the state and the parameter image behind every launch.  The reference is tests/fit_update_ref.py
(pinned on the CPU, with its mutation tier, by tests/test_cpu_fit_update_ref.py); the acceptance rule is fit_update_ref.kron_accept /
dense_accept, the same function the mutation tier runs:

* exact tier (positive = 0 on every block: no libm function is evaluated): every output of every step equals the float64 reference bit for
  bit -- x, m, v, the whole image (so nothing outside the compact blocks is written), the history;
* bound tier (the transforms the models set): per element err_gpu <= 4 err_np + 16 eps S against the long double reference on the
  device's own inputs; the IEEE relations among the device's own values (KH_INV == 1 / KH_ELL, Zs == Z (KUF_C (1 / ell)), the pivot
  tolerance, the block a step read left intact, untrainable blocks, zero slots and padding) bit for bit in either tier.

Every unwritten double of a result block holds the stage sentinel, so an update that read outside the compact parts would show as 1e306.
A factor dimension of 8 does not reach k_fit_update: the fused path stops at 7 (17 moment columns), the fit loops and the hook refuse.
STAGE-LOG lines carry the largest err / (eps S) per output class (profiles/fit_update_parity.log keeps a run's)."""
import numpy as np
import pytest

import fit_update_ref as R
from zigp import _lib

pytestmark = pytest.mark.gpu


def _log(kernel, case, text):
    print('STAGE-LOG %-22s %-34s %s' % ('fit_update/' + kernel, case, text))


def _fmt(ratios):
    return ' '.join('%s %.2f' % (k.replace(' ', '_'), v) for k, v in sorted(ratios.items()))


def _kron_run(engine, case):
    L = case['L']
    x, m, v = case['x'].copy(), case['m'].copy(), case['v'].copy()
    out = engine.test_kron_fit_update(L.shape, L.lik, x, m, v, case['lr'], case['positive'], case['trainable'], case['t0'], case['blocks'])
    out['final'] = (x, m, v)
    return out


def _kron_final(case, out):
    """the call's in / out arrays hold the last snapshot"""
    for k, a in zip('xmv', out['final']):
        assert R.same_bits(a, out['snap_' + k][-1]), k


@pytest.mark.parametrize('tier', ('exact', 'bound'))
@pytest.mark.parametrize('name', sorted(R.KRON_CASES))
def test_kron_update(engine, name, tier):
    k = R.KRON_CASES[name]
    facts = engine.test_kron_fit_update_facts(k['shape'], k['lik'])
    mine = R.KronLayout(k['shape'], k['lik']).facts
    assert {q: facts[q] for q in mine} == mine                      # kf_prepare / kf_fit_describe as restated
    assert facts['big_off'][8] == k['big'] and facts['grid'] == -(-k['big'] // 256) + 1
    case = R.kron_fixture(name, tier, facts=facts)
    L = case['L']
    seen = [q for q in L.element_map() if q is not None]            # the thread -> element map covers every element exactly once
    assert sorted(seen) == [(b, i) for b in range(L.nblocks) for i in range(L.sizes[b])]
    out = _kron_run(engine, case)
    fails, ratios = R.kron_accept(case, out)
    _log('k_fit_update<%s>' % ('true' if L.head else 'false'), '%s %s' % (name, tier), 'grid %d big %d  %s' % (facts['grid'], k['big'], _fmt(ratios) or 'bits'))
    assert not fails, fails[:6]
    assert out['rc'] == 0 and out['steps_applied'] == 3
    _kron_final(case, out)
    if k['trainable'] is not None:                                  # untrainable blocks: unchanged over all steps, yet in every new block
        f = L.facts
        for b, tr in enumerate(k['trainable']):
            if not tr:
                for a in 'xmv':
                    assert R.same_bits(out['snap_' + a][-1][L.sl(b)], case[a][L.sl(b)])
        for i in range(1, 4):
            Hw = f['off_hyp2'] if i & 1 else f['off_hyp']
            img = out['snap_img'][i]
            assert img[Hw + f['KH_NOISE']] == out['snap_img'][0][f['off_hyp'] + f['KH_NOISE']] or k['trainable'][8]
            assert img[Hw + f['KH_FMU']] == out['snap_img'][0][f['off_hyp'] + f['KH_FMU']] or k['trainable'][9]
            for q in range(2):
                if not k['trainable'][4 + q]:
                    D = L.D[q]
                    assert R.same_bits(img[Hw + L.rec(0, q) + f['KH_ELL']:Hw + L.rec(0, q) + f['KH_ELL'] + D],
                                       out['snap_img'][0][f['off_hyp'] + L.rec(0, q) + f['KH_ELL']:f['off_hyp'] + L.rec(0, q) + f['KH_ELL'] + D])


@pytest.mark.parametrize('t0', (0, 37, 10 ** 6))
@pytest.mark.parametrize('lik', ('onoff', 'gaussian', 'bernoulli'))
def test_kron_transform_edges(engine, lik, t0):
    """x in +-{0, 5e-324, 1e-8, 1, 36, 37.5, 40, 709, 745.2, 1e3} x |g| in {0, 1e-320, 1e-12, 1e-8, 1, 1e6, 1e9} x four (m, v) in a Log1pe block:
    the s block of a head, and of latent g of the on/off model (behind latent f's blocks in the element map)"""
    facts = engine.test_kron_fit_update_facts(R.EDGE_SHAPES['onoff' if lik == 'onoff' else 'head'], lik)
    case = R.kron_edge_case(lik, t0, facts=facts)
    L = case['L']
    out = _kron_run(engine, case)
    fails, ratios = R.kron_accept(case, out)
    _log('k_fit_update<%s>' % ('true' if L.head else 'false'), 'edges %s t0 %d' % (lik, t0),
         _fmt({k: v for k, v in ratios.items() if k.endswith(' s') or k.startswith('image')}))
    assert not fails, fails[:6]
    sl = L.sl(case['edge_block'])
    x0, x1 = out['snap_x'][0][sl], out['snap_x'][1][sl]
    m0, m1, v0, v1 = out['snap_m'][0][sl], out['snap_m'][1][sl], out['snap_v'][0][sl], out['snap_v'][1][sl]
    n_still = n_sat = 0
    for j, (xe, g, (me, ve)) in enumerate(case['edge']):
        if g == 0.0 and me == 0.0 and ve == 0.0:                    # no gradient, no momentum: x keeps its bits (the signed zero too)
            assert x1[j:j + 1].view(np.int64)[0] == x0[j:j + 1].view(np.int64)[0], (j, xe)
            n_still += 1
        if 0.5 * (1.0 + np.tanh(0.5 * xe)) == 0.0:                  # a saturated sigmoid: the moments only decay, and without momentum x stays
            assert m1[j] == 0.9 * m0[j] and v1[j] == 0.999 * v0[j], (j, xe, g)
            if me == 0.0:
                assert x1[j:j + 1].view(np.int64)[0] == x0[j:j + 1].view(np.int64)[0], (j, xe, g)
            n_sat += 1
    assert n_still == 20 and n_sat >= 2 * 7 * 4


@pytest.mark.parametrize('name', ('gauss-15x17-d21', 'berno-9x50-d17', 'onoff-32x32-10x12-d21', 'onoff-16x112-9x50-d51'))
def test_kron_failure_latch(engine, name):
    """an injected Cholesky status (no Cholesky runs): the state freezes at the step before, the lower job index wins, the history from
    the failing step on comes back NaN, ZIGP_ENOTPD with steps_applied; a failure in step 0 leaves the inputs; the context works afterwards"""
    k = R.KRON_CASES[name]
    facts = engine.test_kron_fit_update_facts(k['shape'], k['lik'])
    njobs = 2 if k['lik'] != 'onoff' else 4
    for step, info, want in ((1, [0] * (njobs - 1) + [7], (njobs - 1, 7)), (1, [0, 5] + [9] * (njobs - 2), (1, 5)), (0, [3] + [4] * (njobs - 1), (0, 3)),
                             (2, [0, -2], (1, -2))):
        case = R.kron_fixture(name, 'exact', facts=facts, info={step: info})
        out = _kron_run(engine, case)
        fails, _ = R.kron_accept(case, out)
        assert not fails, fails[:6]
        assert out['rc'] == _lib.ZIGP_ENOTPD and out['steps_applied'] == step and tuple(out['fail'][:3]) == (1 + step,) + want
        assert 'pivot %d' % want[1] in out['error'] and 'step %d' % step in out['error']
        assert np.all(np.isfinite(out['elbo_data'][:step])) and np.all(np.isnan(out['elbo_data'][step:])) and np.all(np.isnan(out['kl'][step:]))
        _kron_final(case, out)
        if step == 0:
            for a, b in zip('xmv', out['final']):
                assert R.same_bits(b, case[a])
    case = R.kron_fixture(name, 'exact', facts=facts)                # a clean call on the same context afterwards
    out = _kron_run(engine, case)
    assert out['rc'] == 0 and not R.kron_accept(case, out)[0]
    _log('k_fit_update', 'failure latch ' + name, 'ok')


@pytest.mark.parametrize('lik', ('onoff', 'gaussian', 'bernoulli'))
def test_kron_kl_history(engine, lik):
    """pws[7] in {0, 1, 2} on grids with M0 != M1 (on/off: both latents different): the history against kron_kl's formula, bit for bit"""
    shape = R.KL_SHAPES['onoff' if lik == 'onoff' else 'head']
    facts = engine.test_kron_fit_update_facts(shape, lik)
    for ranks in (0.0, 1.0, 2.0):
        case = R.kron_case(shape, lik, 'exact', ranks=ranks, facts=facts)
        out = _kron_run(engine, case)
        L, f = case['L'], facts
        for i, blk in enumerate(case['blocks']):
            kl = 0.0
            if ranks > 0:
                for h, (M0, M1) in enumerate(L.M):
                    vk = blk[h * f['RES_SIZE']:h * f['RES_SIZE'] + 5]
                    kl += 0.5 * (vk[0] - ranks * float(M0) * M1 - vk[1] + vk[2] + float(M1) * vk[3] + float(M0) * vk[4])
            assert out['kl'][i] == kl and out['elbo_data'][i] == blk[f['RES_PWS']], (ranks, i)
        assert (ranks == 0.0) == bool(np.all(out['kl'] == 0.0))
        assert not R.kron_accept(case, out)[0]


def test_kron_refusals(engine):
    """what the fit loops refuse, the hook refuses: a factor dimension of 8, a grid beyond the fused kernels, the panel switch"""
    for shape in (dict(M0f=4, M1f=4, D0=8, D1=1), dict(M0f=4, M1f=4, D0=1, D1=8), dict(M0f=33, M1f=33, D0=1, D1=1), dict(M0f=17, M1f=100, D0=1, D1=1)):
        with pytest.raises(ValueError, match='beyond the fused Kronecker kernels'):
            engine.test_kron_fit_update_facts(shape, 'gaussian')
    engine.set_kron_panels(True)
    try:
        with pytest.raises(ValueError, match='beyond the fused Kronecker kernels'):
            engine.test_kron_fit_update_facts(dict(M0f=4, M1f=4, D0=1, D1=1), 'gaussian')
    finally:
        engine.set_kron_panels(False)
    assert engine.test_kron_fit_update_facts(dict(M0f=4, M1f=4, D0=7, D1=7), 'gaussian')['grid'] == 2


# ---- dense
@pytest.fixture(scope='module')
def dense_engine():
    """an engine of its own: the dense hook needs a resident data set of the case's D (the loop plans its step), and no other test's"""
    import zigp
    e = zigp.DenseEngine(0)
    yield e
    e.close()


_DATA = {}


def _dense_run(eng, case, D):
    if _DATA.get('D') != D:
        rs = np.random.RandomState(5)
        eng.set_data(rs.rand(64, D), rs.rand(64, 1))
        _DATA['D'] = D
    L = case['L']
    x, m, v = case['x'].copy(), case['m'].copy(), case['v'].copy()
    shape = dict(Mf=L.M[0], Mg=L.M[1], D=L.D)
    mode = {0: _lib.FIT_DIAG, 1: _lib.FIT_WHITE, 2: _lib.FIT_WHITE_FULL}[L.mode]
    out = eng.test_dense_fit_update(mode, shape, x, m, v, case['lr'], case['positive'], case['trainable'], L.es, case['t0'], case['packed'],
                                    case['info'], jitter=case['jitter'])
    out['final'] = (x, m, v)
    return out


def _dense_facts(eng, k):
    if _DATA.get('D') != k['shape']['D']:
        rs = np.random.RandomState(5)
        eng.set_data(rs.rand(64, k['shape']['D']), rs.rand(64, 1))
        _DATA['D'] = k['shape']['D']
    case = R.dense_case(k['mode'], k['shape'], k['ell_size'], 'exact')
    mode = {0: _lib.FIT_DIAG, 1: _lib.FIT_WHITE, 2: _lib.FIT_WHITE_FULL}[k['mode']]
    return eng.test_dense_fit_update(mode, k['shape'], case['x'], case['m'], case['v'], case['lr'], case['positive'], [1] * 11, k['ell_size'], 0, None,
                                     jitter=case['jitter'])


@pytest.mark.parametrize('tier', ('exact', 'bound'))
@pytest.mark.parametrize('name', sorted(R.DENSE_CASES))
def test_dense_update(dense_engine, name, tier):
    k = R.DENSE_CASES[name]
    dense_engine.set_pivot_rtol(8.0)
    facts = _dense_facts(dense_engine, k)
    case = R.dense_fixture(name, tier, facts=facts)
    L = case['L']
    mine = R.DenseLayout(k['mode'], k['shape'], k['ell_size']).facts      # latents_layout and the DH_* slots as restated
    assert {q: facts[q] for q in mine} == mine
    assert facts['n_packed'] == L.n_packed and facts['grid'] == -(-L.n_free // 256)
    assert all(p >= M for p, M in zip(facts['Mp'], L.M)) and facts['n_img'] >= sum(facts['Mp']) * (2 * L.D + 2)
    out = _dense_run(dense_engine, case, L.D)
    fails, ratios = R.dense_accept(case, out)
    _log('k_dense_fit_*', '%s %s' % (name, tier), 'n_free %d  %s' % (L.n_free, _fmt(ratios) or 'bits'))
    assert not fails, fails[:6]
    assert out['rc'] == 0 and out['steps_applied'] == 3
    for a, b in zip('xmv', out['final']):
        assert R.same_bits(b, out['snap_' + a][-1])
    for b, tr in enumerate(k['trainable']):
        if not tr:
            for a in 'xmv':
                assert R.same_bits(out['snap_' + a][-1][L.sl(b)], case[a][L.sl(b)])


@pytest.mark.parametrize('name', ('m0-17x5-d3-e13', 'm1-5x17-d8-e81', 'm2-17x5-d3-e13'))
def test_dense_failure_latch(dense_engine, name):
    k = R.DENSE_CASES[name]
    dense_engine.set_pivot_rtol(8.0)
    facts = _dense_facts(dense_engine, k)
    for step, info, want in ((1, (0, 7), (1, 7)), (1, (5, 9), (0, 5)), (0, (3, 0), (0, 3)), (2, (0, -2), (1, -2))):
        case = R.dense_fixture(name, 'exact', facts=facts, info={step: info})
        out = _dense_run(dense_engine, case, case['L'].D)
        fails, _ = R.dense_accept(case, out)
        assert not fails, fails[:6]
        assert out['rc'] == _lib.ZIGP_ENOTPD and out['steps_applied'] == step and tuple(out['fail'][:3]) == (1 + step,) + want
        assert np.all(np.isnan(out['elbo_data'][step:])) and np.all(np.isnan(out['kl'][step:])) and np.all(np.isfinite(out['kl'][:step]))
        if step == 0:
            for a, b in zip('xmv', out['final']):
                assert R.same_bits(b, case[a])
    case = R.dense_fixture(name, 'exact', facts=facts)
    out = _dense_run(dense_engine, case, case['L'].D)
    assert out['rc'] == 0 and not R.dense_accept(case, out)[0]
    _log('k_dense_fit_update', 'failure latch ' + name, 'ok')


def test_ordinary_fit_calls_after_the_hooks(dense_engine, engine):
    """the hooks change nothing for the calls that follow: an ordinary dense fit call and an ordinary head fit call return the same bits
    before and after a tapped call on the same context"""
    import zigp
    from conftest import make_problem
    import dense_fit_ref as dref
    import head_fit_ref as href
    X, Y, p = make_problem(600, 12, 2, seed=3)

    def dense_fit():
        dense_engine.set_data(X, Y)
        _DATA.clear()
        f = zigp.optim.DenseDeviceFit(dense_engine, dref.make_pset(p))
        hist = f.steps(None, 0, 1e-6, 1.0, n_steps=3)
        return f.x.copy(), f.m.copy(), f.v.copy(), np.array(hist)

    a = dense_fit()
    k = R.DENSE_CASES['m0-16x16-d1-e11']
    case = R.dense_fixture('m0-16x16-d1-e11', 'exact', facts=_dense_facts(dense_engine, k))
    assert _dense_run(dense_engine, case, 1)['rc'] == 0
    b = dense_fit()
    for u, w in zip(a, b):
        assert R.same_bits(u, w)

    Xk, Yk, make_pset = href.head_problem((6, 5), 'gaussian')
    x0, lr, pos, tr, shape = href.flat_state(make_pset())

    def head_fit():
        engine.set_data(Xk, Yk)
        x, m, v = x0.copy(), np.zeros_like(x0), np.zeros_like(x0)
        hist = engine.kron_head_fit_steps(shape, 'gaussian', x, m, v, lr, pos, tr, 0, [0, 500, 1000], href.BATCH, jitter=href.JITTER, scale=href.SCALE)
        return x, m, v, np.array(hist)

    a = head_fit()
    case = R.kron_fixture('gauss-15x17-d21', 'exact', facts=engine.test_kron_fit_update_facts(R.KRON_CASES['gauss-15x17-d21']['shape'], 'gaussian'))
    assert _kron_run(engine, case)['rc'] == 0
    b = head_fit()
    for u, w in zip(a, b):
        assert R.same_bits(u, w)
