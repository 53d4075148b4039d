"""Pins tests/fit_update_ref.py -- the restatement tests/test_gpu_fit_update_stages.py holds the update kernels of the device fit loops to
-- before it judges a kernel:

(i)   its float64 form equals zigp.optim.AdamGroups.step bit for bit, fed the gradients kronf_ref.assemble (Kronecker) or the packed blocks
      (dense) give, for a ParamSet of each layout; and its own chain rule equals kronf_ref.assemble;
(ii)  one step of it equals head_fit_ref.ref_head_fit_steps and dense_fit_ref.ref_fit_steps given the same gradients;
(iii) the mutation tier, on exactly the fixtures of the GPU tests: a stand-in "device" that makes one deliberate mistake must FAIL the
      acceptance rule (fit_update_ref.kron_accept / dense_accept, the function the GPU tests assert with) on every fixture on which the
      mistake changes anything; where it provably changes nothing (M0 = M1, D0 = D1, no positive block, every block trainable, ...) that is
      recognised by the unchanged long double result of every step, and every mistake is resolved on some fixture."""
from collections import OrderedDict

import numpy as np
import pytest

import fit_update_ref as R
import kronf_ref as kr
from zigp.optim import P, ParamSet, AdamGroups
from zigp.transforms import Log1pe, Identity, LowerTriangular

LD = np.longdouble


def _compact(L, blk, h):
    """(krow [2], gu, gs) of latent h out of a raw result block"""
    f = L.facts
    o = h * f['RES_SIZE']
    krow = [blk[o + f[k]:o + f[k] + L.M[h][q] * (2 + 2 * L.D[q])].reshape(L.M[h][q], 2 + 2 * L.D[q]) for q, k in enumerate(('RES_KROW0', 'RES_KROW1'))]
    n = L.M[h][0] * L.M[h][1]
    return krow, blk[o + f['RES_GU']:o + f['RES_GU'] + n], blk[o + f['RES_GS']:o + f['RES_GS'] + n]


def _assemble_grads(L, case, blk):
    """per block: kron_assemble_grads as kronf_ref.assemble restates it, at the values of the case's free state"""
    f = L.facts
    val = [R.softplus(case['x'][L.sl(b)]) if case['positive'][b] else case['x'][L.sl(b)] for b in range(L.nblocks)]
    pws = blk[f['RES_PWS']:f['RES_PWS'] + 8]
    out = [None] * L.nblocks
    for h in range(L.nlat):
        b0 = 8 * h
        krow, gu, gs = _compact(L, blk, h)
        a = kr.assemble(krow, gu, gs, [val[b0 + 4], val[b0 + 5]], [val[b0 + 6], val[b0 + 7]], pws[2 + h])
        out[b0:b0 + 8] = [a['Z'][0][0].reshape(-1), a['Z'][1][0].reshape(-1), a['u'][0], a['s'][0], a['ell'][0][0], a['ell'][1][0],
                          np.array([a['var'][0][0]]), np.array([a['var'][1][0]])]
    out[8 * L.nlat] = np.array([pws[1]])
    if L.head:
        out[9] = np.array([pws[4]])
    return out


def _pset(sizes, x, lr, positive, trainable, tri=()):
    q = OrderedDict()
    for b, n in enumerate(sizes):
        tf = LowerTriangular(tri[b]) if b in tri else (Log1pe() if positive[b] else Identity())
        p = P(np.zeros((tri[b], tri[b])) if b in tri else np.zeros(n), tf, fixed=not trainable[b], learning_rate=lr[b], name='b%d' % b)
        p.set_free(x[sum(sizes[:b]):sum(sizes[:b]) + n])
        q['b%d' % b] = p
    return ParamSet(q)


def _adam_groups(pset, sizes, x, m, v, t0):
    """AdamGroups holding exactly this free state (its own free vectors come from transform.backward, which does not round-trip)"""
    opt = AdamGroups(pset)
    opt.t = t0
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for b in range(len(sizes)):
        k = 'b%d' % b
        if k in opt.x:
            sl = slice(offs[b], offs[b + 1])
            opt.x[k], opt.m[k], opt.v[k] = x[sl].copy(), m[sl].copy(), v[sl].copy()
    return opt


KRON_PIN = ('gauss-15x17-d21', 'berno-9x50-d17', 'gauss-1x112-d77', 'onoff-10x30-30x10-d21', 'onoff-5x7-7x5-d77')


@pytest.mark.parametrize('name', KRON_PIN)
def test_kron_float64_form_is_adamgroups(name):
    case = R.kron_fixture(name, 'bound')
    L = case['L']
    tr = case['trainable'] or [1] * L.nblocks
    blk = case['blocks'][0]
    grads = _assemble_grads(L, case, blk)
    pset = _pset(L.sizes, case['x'], case['lr'], case['positive'], tr)
    opt = _adam_groups(pset, L.sizes, case['x'], case['m'], case['v'], case['t0'])
    opt.step({'b%d' % b: grads[b] for b in range(L.nblocks)})
    lrf = R.lr_factors(case['t0'] + 1)
    for b in range(L.nblocks):
        if not tr[b]:
            continue
        sl, k = L.sl(b), 'b%d' % b
        r = R.adam(grads[b], np.abs(grads[b]), case['x'][sl], case['m'][sl], case['v'][sl], case['positive'][b], case['lr'][b], lrf)
        assert R.same_bits(r['x'][0], opt.x[k]) and R.same_bits(r['m'][0], opt.m[k]) and R.same_bits(r['v'][0], opt.v[k]), b
        val = R.softplus(r['x'][0]) if case['positive'][b] else r['x'][0]
        assert R.same_bits(val, pset.params[k].value)


@pytest.mark.parametrize('name', KRON_PIN)
def test_kron_chain_rule_is_assemble(name):
    """the device's copy of the host chain rule: bit for bit where no sum is taken or numpy's sum takes the m order too (fewer than 8 rows:
    beyond that np.sum is pairwise), within 4 eps S of the long double form everywhere"""
    case = R.kron_fixture(name, 'bound')
    L = case['L']
    img = R.kron_image(L, case['x'], case['positive'], np.zeros(L.facts['n_img']))
    mine = R.kron_grads(L, case['blocks'][0], img, 0)
    truth = R.kron_grads(L, case['blocks'][0], img, 0, dt=LD)
    ref = _assemble_grads(L, case, case['blocks'][0])
    for b in range(L.nblocks):
        h, k = L.kind(b)
        if k <= 3 or k >= 8 or L.M[h][(k - 4) % 2] < 8:
            assert R.same_bits(mine[b][0], ref[b]), (b, k)
        assert np.all(np.abs(ref[b] - truth[b][0]) <= 4 * R.EPS * truth[b][1]) and np.all(np.abs(mine[b][0] - truth[b][0]) <= 4 * R.EPS * truth[b][1])


@pytest.mark.parametrize('lik', ('gaussian', 'bernoulli'))
def test_kron_one_step_is_head_fit_ref(lik):
    import head_fit_ref as href
    name = ('gauss' if lik == 'gaussian' else 'berno') + '-15x17-d21'
    case = R.kron_fixture(name, 'bound')
    L = case['L']
    grads = _assemble_grads(L, case, case['blocks'][0])
    seen = {}

    def eg(Xb, Yb, p, f_mu, jitter, scale):
        seen.update(p=p, f_mu=f_mu)
        g = dict(Zf=[grads[0], grads[1]], u_fm=grads[2], u_fs_sqrt=grads[3], ell_f=[grads[4], grads[5]], var_f=[grads[6], grads[7]], noise=grads[8],
                 f_mu=grads[9])
        return -1.5, 2.5, g

    x, m, v = case['x'].copy(), case['m'].copy(), case['v'].copy()
    href.ref_head_fit_steps(eg, np.zeros((4, 3)), np.zeros(4), L.shape, x, m, v, case['lr'], case['positive'], case['trainable'], case['t0'], [0], 2)
    lrf = R.lr_factors(case['t0'] + 1)
    img = R.kron_image(L, case['x'], case['positive'], np.zeros(L.facts['n_img']))
    f = L.facts
    assert R.same_bits(seen['p']['ell_f'][0], img[f['off_hyp'] + f['KH_ELL']:f['off_hyp'] + f['KH_ELL'] + L.D[0]])
    assert seen['p']['var_f'][1][0] == img[f['off_hyp'] + L.rec(0, 1) + f['KH_VAR']] and seen['p']['noise'] == img[f['off_hyp'] + f['KH_NOISE']]
    assert seen['f_mu'] == img[f['off_hyp'] + f['KH_FMU']]
    assert R.same_bits(seen['p']['u_fs_sqrt'].reshape(-1), img[f['off_s'][0]:f['off_s'][0] + L.sizes[3]])
    for b in range(L.nblocks):
        sl = L.sl(b)
        if not case['trainable'][b]:
            assert R.same_bits(x[sl], case['x'][sl]) and R.same_bits(m[sl], case['m'][sl])
            continue
        r = R.adam(grads[b], np.abs(grads[b]), case['x'][sl], case['m'][sl], case['v'][sl], case['positive'][b], case['lr'][b], lrf)
        assert R.same_bits(r['x'][0], x[sl]) and R.same_bits(r['m'][0], m[sl]) and R.same_bits(r['v'][0], v[sl]), b


DENSE_PIN = ('m0-17x5-d3-e13', 'm1-5x17-d8-e81', 'm2-17x5-d3-e13', 'm2-33x1-d8-e88')


@pytest.mark.parametrize('name', DENSE_PIN)
def test_dense_float64_form_is_adamgroups(name):
    case = R.dense_fixture(name, 'bound')
    L = case['L']
    grads = R.dense_grads(L, case['packed'][0])
    tri = {4: L.M[0], 5: L.M[1]} if L.tri else {}
    pset = _pset(L.sizes, case['x'], case['lr'], case['positive'], case['trainable'], tri)
    opt = _adam_groups(pset, L.sizes, case['x'], case['m'], case['v'], case['t0'])
    g = {}
    for b in range(11):
        g['b%d' % b] = grads[b][0]
        if b in tri:      # AdamGroups takes the (M, M) matrix; LowerTriangular.grad_free picks the triangle in row-major order
            A = np.zeros((tri[b], tri[b]))
            A[np.tril_indices(tri[b])] = grads[b][0]
            g['b%d' % b] = A
    opt.step(g)
    r = R.dense_step(L, case['x'], case['m'], case['v'], np.zeros(L.facts['n_img']), np.zeros(L.facts['DH_SIZE']), case['packed'][0], (0, 0),
                     case['t0'] + 1, case['lr'], case['positive'], case['trainable'], case['jitter'], case['rtol_eps'])
    f = L.facts
    for b in range(11):
        sl, k = L.sl(b), 'b%d' % b
        if not case['trainable'][b]:
            assert R.same_bits(r['x'][sl], case['x'][sl]) and R.same_bits(r['v'][sl], case['v'][sl])
            continue
        assert R.same_bits(r['x'][sl], opt.x[k]) and R.same_bits(r['m'][sl], opt.m[k]) and R.same_bits(r['v'][sl], opt.v[k]), b
    for h in range(2):      # the image holds what the ParamSet holds
        assert R.same_bits(r['img'][f['img_Z'][h]:f['img_Z'][h] + L.sizes[h]], pset.params['b%d' % h].value)
        assert R.same_bits(r['img'][f['img_u'][h]:f['img_u'][h] + L.M[h]], pset.params['b%d' % (2 + h)].value)
        assert r['H'][h * f['DH_LAT'] + f['DH_VAR']] == pset.params['b%d' % (8 + h)].value[0]
        if L.tri:
            assert R.same_bits(r['Lraw'][h], pset.params['b%d' % (4 + h)].value) and not np.any(np.signbit(np.triu(r['Lraw'][h], 1)))
        else:
            assert R.same_bits(r['img'][f['img_s'][h]:f['img_s'][h] + L.M[h]], pset.params['b%d' % (4 + h)].value)


def test_dense_one_step_is_dense_fit_ref():
    """ref_fit_steps folds a scalar lengthscale's gradient with np.sum: at D = 3 that is the d order of the kernel"""
    import dense_fit_ref as dref
    case = R.dense_fixture('m0-17x5-d3-e13', 'bound')
    L = case['L']
    p0 = case['packed'][0]
    ard = {}
    for b, k in enumerate(dref.DENSE_FIT_KEYS):
        ard[k] = p0[L.goff[b]:L.goff[b] + L.sizes[b] * L.gn[b]].copy()

    def eg(Xb, Yb, p, jitter, scale):
        return p0[0], p0[1], ard

    x, m, v = case['x'].copy(), case['m'].copy(), case['v'].copy()
    ed, kl = dref.ref_fit_steps(eg, np.zeros((4, 3)), np.zeros(4), dict(Mf=17, Mg=5, D=3), x, m, v, case['lr'], case['positive'], case['trainable'],
                                L.es, case['t0'], 1)
    r = R.dense_step(L, case['x'], case['m'], case['v'], np.zeros(L.facts['n_img']), np.zeros(L.facts['DH_SIZE']), p0, (0, 0), case['t0'] + 1,
                     case['lr'], case['positive'], case['trainable'], case['jitter'], case['rtol_eps'])
    assert R.same_bits(r['x'], x) and R.same_bits(r['m'], m) and R.same_bits(r['v'], v)
    assert (ed[0], kl[0]) == (float(r['hist'][0]), float(r['hist'][1]))


def test_sequential_sum_is_not_numpys():
    """why the reference sums by hand: from 8 entries on np.sum is pairwise, the kernels' loops are not"""
    a = np.array([2.0 ** 60, 1.0, -2.0 ** 60, 1.0, 3.0, 2.0 ** -30, 5.0, 7.0])
    assert float(R.seqsum(a, np.float64)) == 16.0 + 2.0 ** -30 and float(R.seqsum(a, np.float64)) != float(np.sum(a))


def test_float64_is_long_double_on_the_exact_tier():
    """m, v, the image and the history of the exact tier are exact in float64 only up to one rounding per operation: the float64 form is the
    yardstick there (bit for bit), the long double form agrees with it within the rule's weights"""
    for name in ('gauss-1x84-d31', 'onoff-32x32-10x12-d21'):
        case = R.kron_fixture(name, 'exact')
        L = case['L']
        img = R.kron_image(L, case['x'], case['positive'], np.zeros(L.facts['n_img']))
        kw = dict(lr=case['lr'], positive=case['positive'], trainable=case['trainable'])
        ra = R.kron_step(L, case['x'], case['m'], case['v'], img, case['blocks'][0], 0, case['t0'] + 1, **kw)
        rb = R.kron_step(L, case['x'], case['m'], case['v'], img, case['blocks'][0], 0, case['t0'] + 1, dt=LD, **kw)
        for k in 'xmv':
            assert np.all(np.abs(ra[k] - rb[k]) <= 4 * R.EPS * rb['S_' + k])


# ---- (iii) the mutation tier
def _changes_kron(case, clean, mut):
    """does the mistake change the long double result of any launch, on the inputs the clean run holds there?"""
    L = case['L']
    z = np.zeros(L.facts['n_img'])
    if not np.array_equal(R.kron_image(L, case['x'], case['positive'], z, LD), R.kron_image(L, case['x'], case['positive'], z, LD, mut), equal_nan=True):
        return True
    kw = dict(lr=case['lr'], positive=case['positive'], trainable=case['trainable'], dt=LD)
    for i, blk in enumerate(case['blocks']):
        a = (clean['snap_x'][i], clean['snap_m'][i], clean['snap_v'][i], clean['snap_img'][i], blk, i, case['t0'] + i + 1)
        r0, r1 = R.kron_step(L, *a, **kw), R.kron_step(L, *a, mut=mut, **kw)
        if r0['fail'] is not None:
            break
        if any(not np.array_equal(r0[k], r1[k], equal_nan=True) for k in ('x', 'm', 'v', 'img')) or tuple(r0['hist']) != tuple(r1['hist']):
            return True
    return False


def _kron_fixtures():
    for name in sorted(R.KRON_CASES):
        for tier in ('exact', 'bound'):
            yield '%s %s' % (name, tier), R.kron_fixture(name, tier)
    for lik in ('onoff', 'gaussian', 'bernoulli'):
        for t0 in (0, 37, 10 ** 6):
            yield 'edges %s %d' % (lik, t0), R.kron_edge_case(lik, t0)
        for ranks in (0.0, 1.0, 2.0):
            yield 'kl %s %g' % (lik, ranks), R.kron_case(R.KL_SHAPES['onoff' if lik == 'onoff' else 'head'], lik, 'exact', ranks=ranks)


_KRON_FIX = {}


def _kron_all():
    if not _KRON_FIX:
        for tag, case in _kron_fixtures():
            L = case['L']
            clean = R.kron_run(L, case['x'], case['m'], case['v'], case['blocks'], case['t0'], case['lr'], case['positive'], case['trainable'])
            _KRON_FIX[tag] = (case, clean)
    return _KRON_FIX


def test_clean_reference_is_accepted():
    for tag, (case, clean) in _kron_all().items():
        fails, _ = R.kron_accept(case, clean)
        assert not fails, (tag, fails[:3])


@pytest.mark.parametrize('mut', R.ADAM_MUTATIONS + R.KRON_MUTATIONS)
def test_kron_mutation_fails_the_rule(mut):
    resolved, unchanged = [], []
    for tag, (case, clean) in _kron_all().items():
        L = case['L']
        if not _changes_kron(case, clean, (mut,)):
            unchanged.append(tag)
            continue
        out = R.kron_run(L, case['x'], case['m'], case['v'], case['blocks'], case['t0'], case['lr'], case['positive'], case['trainable'], mut=(mut,))
        fails, _ = R.kron_accept(case, out)
        assert fails, 'the rule accepts the mistake %r on %s' % (mut, tag)
        resolved.append(tag)
    assert resolved, mut
    # where a mistake may change nothing, and nowhere else
    for tag in unchanged:
        case = _KRON_FIX[tag][0]
        L = case['L']
        why = {'sigmoid_dropped': not any(case['positive']), 'softplus_no_lower': not any(case['positive']),
               'softplus_zero_branch': not any(np.any(case['x'][L.sl(b)] == 0) for b in range(L.nblocks) if case['positive'][b]),
               'z_stride_other': L.D[0] == L.D[1] or all(M == (1, 1) for M in L.M),
               'kl_m_swapped': all(M[0] == M[1] for M in L.M) or case['blocks'][0][L.facts['RES_PWS'] + 7] == 0,
               'kl_ranks_ignored': case['blocks'][0][L.facts['RES_PWS'] + 7] == 1,
               'untrainable_not_rederived': case['trainable'] is None or all(case['trainable']),
               'noise_pws4': case['trainable'] is not None and not case['trainable'][8 * L.nlat]}.get(mut, False)
        assert why, 'the mistake %r changes nothing on %s' % (mut, tag)


def _changes_dense(case, clean, mut):
    L = case['L']
    kw = dict(lr=case['lr'], positive=case['positive'], trainable=case['trainable'], jitter=case['jitter'], rtol_eps=case['rtol_eps'], dt=LD)
    z, zh = np.zeros(L.facts['n_img']), np.zeros(L.facts['DH_SIZE'])
    i0 = R.dense_image(L, case['x'], case['positive'], z, zh, case['jitter'], case['rtol_eps'], LD)
    i1 = R.dense_image(L, case['x'], case['positive'], z, zh, case['jitter'], case['rtol_eps'], LD, mut)
    if not (np.array_equal(i0[0], i1[0]) and np.array_equal(i0[1], i1[1]) and (not L.tri or all(np.array_equal(a, b) for a, b in zip(i0[2], i1[2])))):
        return True
    for i in range(len(case['packed'])):
        a = (clean['snap_x'][i], clean['snap_m'][i], clean['snap_v'][i], clean['snap_img'][i], clean['snap_H'][i], case['packed'][i], case['info'][i],
             case['t0'] + i + 1)
        r0, r1 = R.dense_step(L, *a, **kw), R.dense_step(L, *a, mut=mut, **kw)
        if any(not np.array_equal(r0[k], r1[k], equal_nan=True) for k in ('x', 'm', 'v', 'img', 'H')):
            return True
        if L.tri and any(not np.array_equal(p, q) for p, q in zip(r0['Lraw'], r1['Lraw'])):
            return True
    return False


DENSE_ADAM_MUTATIONS = ('eps_inside', 'v_linear', 'beta_swap', 'g_sign', 'sigmoid_dropped', 'sigmoid_on_identity', 'softplus_no_lower',
                        'softplus_zero_branch')


@pytest.mark.parametrize('mut', R.DENSE_MUTATIONS + DENSE_ADAM_MUTATIONS)
def test_dense_mutation_fails_the_rule(mut):
    resolved = []
    for name in sorted(R.DENSE_CASES):
        for tier in ('exact', 'bound'):
            case = R.dense_fixture(name, tier)
            L = case['L']
            a = (L, case['x'], case['m'], case['v'], case['packed'], case['info'], case['t0'], case['lr'], case['positive'], case['trainable'],
                 case['jitter'], case['rtol_eps'])
            clean = R.dense_run(*a)
            fails, _ = R.dense_accept(case, clean)
            assert not fails, (name, tier, fails[:3])
            if not _changes_dense(case, clean, (mut,)):
                why = {'ell_first_only': not any(L.es[h] == 1 and L.D > 1 and case['trainable'][6 + h] for h in range(2)),
                       'tri_column_major': not L.tri,
                       'sigmoid_dropped': not any(case['positive']), 'softplus_no_lower': not any(case['positive']),
                       'softplus_zero_branch': not any(case['positive'])}.get(mut, False)
                assert why, 'the mistake %r changes nothing on %s %s' % (mut, name, tier)
                continue
            fails, _ = R.dense_accept(case, R.dense_run(*a, mut=(mut,)))
            assert fails, 'the rule accepts the mistake %r on %s %s' % (mut, name, tier)
            resolved.append((name, tier))
    assert resolved, mut


def test_failure_latch_of_the_reference():
    """the failure rule as the GPU tests inject it: the stand-in freezes, and a stand-in that applies the failing step is caught"""
    case = R.kron_fixture('onoff-32x32-10x12-d21', 'exact', info={1: [0, 5, 9, 9]})
    L = case['L']
    a = (L, case['x'], case['m'], case['v'], case['blocks'], case['t0'], case['lr'], case['positive'], case['trainable'])
    out = R.kron_run(*a)
    assert not R.kron_accept(case, out)[0]
    assert tuple(out['fail'][:3]) == (2, 1, 5) and out['steps_applied'] == 1 and np.isnan(out['kl'][1]) and np.isfinite(out['kl'][0])
    clean = R.kron_fixture('onoff-32x32-10x12-d21', 'exact')
    wrong = R.kron_run(L, case['x'], case['m'], case['v'], clean['blocks'], case['t0'], case['lr'], case['positive'], case['trainable'])
    assert R.kron_accept(case, wrong)[0]


def test_fixture_sizes_sit_on_the_workgroup_boundaries():
    """255 / 256 / 257 big elements for a head and for the on/off model; the dense free vectors of DENSE_NFREE"""
    for on in (False, True):
        bigs = {k['big'] for k in R.KRON_CASES.values() if (k['lik'] == 'onoff') == on}
        assert {255, 256, 257} <= bigs and max(bigs) > 512
    for mode in (0, 1, 2):
        assert tuple(R.DenseLayout(mode, dict(Mf=M[0], Mg=M[1], D=D), es).n_free for M, D, es, _ in R.DENSE_BOUNDARY[mode]) == R.DENSE_NFREE[mode]
