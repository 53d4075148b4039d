"""CPU pins of tests/path_weights_ref.py, the restatement test_gpu_path_weight_stages.py judges the weight stage of the sample paths by:
the restated sequences against zigp.pathwise.weights_np / kron_weights_np, and the catalogue of deliberate mistakes -- each applied to the
float64 sequence that stands in for the device, each failing the tier that claims it on the GPU test's own fixtures.  No GPU is used: every
figure here is float64 NumPy in the device's place."""
import numpy as np
import pytest

import path_weights_ref as pw
import kronpaths_ref as kr
from zigp import pathwise

LD = np.longdouble


def _bound(c):
    return min(max(1e-9, 1e-13 * c), 1e-6)


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


_SEQ = {}


def _dense(name, tag, dt=np.float64, mutate=None):
    key = (name, tag, dt is LD, mutate)
    if key not in _SEQ:
        inp = pw.dense_host_inputs(name, tag)
        _SEQ[key] = (inp, pw.dense_sequence(pw.DENSE_CASES[name]['mode'], inp['Kuu'], inp['W'], inp['u'], inp['s'], inp['E'], inp['fZ'], inp['tab0'],
                                            Lq=inp.get('Lq'), dt=dt, mutate=mutate, jitter=pw.DENSE_JITTER))
    return _SEQ[key]


PIN_CASES = ['m1_1', 'm50_37', 's17', 's33_matern', 'modes_white', 'modes_full', 'solve_1d', 'solve_3d']


@pytest.mark.parametrize('name', PIN_CASES)
def test_dense_sequence_is_weights_np(name):
    """Long double: Kuu V of the restated sequence (the kernel part of a path at the inducing inputs) equals that of pathwise.weights_np
    under the path bound min(max(1e-9, 1e-13 cond), 1e-6).  Float64: every launch of the sequence is within 16 eps S of its long-double
    restatement on the same operands, and the sequence passes every tier"""
    p, draws = pw.dense_problem(name)
    mode = pw.DENSE_CASES[name]['mode']
    for tag in 'fg':
        inp, ld = _dense(name, tag, LD)
        c = float(np.linalg.cond(inp['Kuu']))
        V = pathwise.weights_np(inp['Kuu'], inp['u'], p['u_%ss_sqrt' % tag], inp['E'], inp['fZ'], whiten=mode > 0, q_diag=mode < 2)
        e = _rel(inp['Kuu'] @ np.asarray(ld['V'], dtype=np.float64), inp['Kuu'] @ V)
        print('PATHW-PIN %s %s: cond(Kuu) %.2e, Kuu V against weights_np %.2e (bound %.1e)' % (name, tag, c, e, _bound(c)))
        assert e < _bound(c)
        inp, seq = _dense(name, tag)
        fail, fig = pw.check_dense(mode, inp, seq, pw.DENSE_CASES[name]['quant'])
        assert not fail, (name, tag, fail, fig)
        assert all(v <= 16 for k, v in fig.items() if k != 'solve'), fig


# mutation -> the tier:launch entries of which one must be reported wherever the mutation changes an output
DENSE_CLAIMS = {'no_refine': {'exact:V'}, 'cor_sub': {'exact:V'}, 'no_jitter': {'bound:KV'}, 'wwt': {'bound:t', 'bound:V'}, 'plus_fz': {'exact:rhs', 'bound:rhs'},
                's_squared': {'exact:rhs', 'bound:rhs'}, 'e_stride': {'exact:rhs', 'bound:rhs', 'bound:H'}, 'tile_shift': {'exact:tab'}, 'tab_unzeroed': {'exact:tab'}}


def _changed(a, b):
    return any(not np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)) for k in a if not k.startswith('S_'))


@pytest.mark.parametrize('mutation', pw.DENSE_MUTATIONS)
def test_dense_mutations_are_caught(mutation):
    """Each mistake, applied to the float64 sequence, fails the tier that claims it on every GPU fixture and latent where it changes any
    output, and changes one on at least three of them; the intact sequence passes (test_dense_sequence_is_weights_np and here)"""
    caught = 0
    for name in pw.DENSE_CASES:
        mode = pw.DENSE_CASES[name]['mode']
        for tag in 'fg':
            inp, good = _dense(name, tag)
            _, bad = _dense(name, tag, mutate=mutation)
            if not _changed(good, bad):
                continue
            fail, fig = pw.check_dense(mode, inp, bad, pw.DENSE_CASES[name]['quant'])
            assert DENSE_CLAIMS[mutation] & set(fail), (mutation, name, tag, fail)
            caught += 1
    print('PATHW-MUTATION %s: caught on %d fixture latents' % (mutation, caught))
    assert caught >= 3


def test_the_refinement_step_is_held_by_the_solve_tier():
    """The named latent is g of solve_1d, matern_ref.problem(700, 137, 137, 1) with its real right-hand side (cond(Kuu) 4e8).  Float64
    NumPy in the device's place: the residual max |rhs - Kuu V| of the intact sequence is 0.53 x that of scipy.linalg.cho_solve on
    the same operands, without the refinement step 46 x -- the bar of 8 lies a factor of two clear of both.  A subtracted
    correction and a residual taken without the jitter fail the same bar; every intact fixture latent of the Diag mode passes it.
    (Correction subtracted: 93 x; no jitter: 8e7 x.)"""
    inp, good = _dense('solve_1d', 'g')
    r = {m: pw.solve_ratio(inp['Kuu'], good['rhs'], _dense('solve_1d', 'g', mutate=m)[1]['V']) for m in (None, 'no_refine', 'cor_sub', 'no_jitter')}
    print('PATHW-SOLVE-CPU solve_1d g: intact %.3g x SciPy, no refinement %.3g x, correction subtracted %.3g x, no jitter %.3g x' % (
        r[None], r['no_refine'], r['cor_sub'], r['no_jitter']))
    assert r[None] <= pw.BAR / 2 and r['no_refine'] >= 2 * pw.BAR and r['cor_sub'] >= 2 * pw.BAR and r['no_jitter'] >= 2 * pw.BAR
    assert pw.solve_ratio(inp['Kuu'], good['rhs'], good['V0']) == r['no_refine']
    for m in ('no_refine', 'cor_sub', 'no_jitter'):
        assert 'solve:V' in pw.check_dense(0, inp, _dense('solve_1d', 'g', mutate=m)[1], False)[0]
    for name, k in pw.DENSE_CASES.items():
        if k['mode'] == 0:
            for tag in 'fg':
                inp, seq = _dense(name, tag)
                assert pw.solve_ratio(inp['Kuu'], seq['rhs'], seq['V']) <= pw.BAR / 2, (name, tag)


# ---- Kronecker ------------------------------------------------------------------------------------------------------------------------------
def _kron_fixtures():
    """(id, p, draws, tag, jitter, S, kinds) of every latent the GPU test runs: the shape cases, the five model cases, the pptr 32 x 32 init"""
    out = []
    for name, k in pw.KRON_CASES.items():
        p, draws, tags = pw.kron_problem(name)
        for t in tags:
            out.append((name + '-' + t, p, draws, t, pw.KRON_JITTER, k['S'], k.get('kinds')))
    for name in pw.KRON_SOLVE_CASES:
        p, draws, S, jitter = pw.kron_solve_problem(name)
        for t in 'fg':
            out.append((name + '-' + t, p, draws, t, jitter, S, None))
    return out


def _kron_inputs(fx):
    name, p, draws, t, jitter, S, kinds = fx
    return pw.kron_host_inputs(p, draws, t, jitter, S, kinds)


_KF = {}
_N_DYADIC = sum(len(k['grids']) for k in pw.KRON_CASES.values())      # the shape cases come first: dyadic u, s, eps


def _kron(i, dt=np.float64, mutate=None):
    key = (i, dt is LD, mutate)
    if key not in _KF:
        if ('inp', i) not in _KF:
            _KF[('inp', i)] = _kron_inputs(_kron_fixtures()[i])
        inp = _KF[('inp', i)]
        _KF[key] = (inp, pw.kron_sequence(inp['W'][0], inp['W'][1], inp['U'], inp['Sq'], inp['E'], inp['FZ'], inp['tab0'], dt=dt, mutate=mutate))
    return _KF[key]


def test_kron_sequence_is_kron_weights_np():
    """Long double: K0 V_s K1 of the restated sequence equals that of kronpaths_ref.kron_weights_ld under the path bound (cond = cond(K0)
    cond(K1)); float64: the sequence passes every tier -- the solve rule res <= 4 res_np + 16 eps S_w included, whose largest figure over
    the fixtures is printed: the Kronecker weights hold it WITHOUT a refinement step"""
    worst = 0.0
    for i, fx in enumerate(_kron_fixtures()):
        if fx[0].startswith('k128x128'):
            continue      # the long-double triangular solves of kron_weights_ld at 128 x 128 take a minute; the float64 tiers below cover it
        inp, ld = _kron(i, LD)
        S, M0, M1 = inp['FZ'].shape
        c = float(np.linalg.cond(inp['K'][0]) * np.linalg.cond(inp['K'][1]))
        V = kr.kron_weights_ld(inp['K'][0], inp['K'][1], inp['U'], inp['Sq'], inp['E'], inp['FZ'].reshape(S, -1).T)
        V = np.ascontiguousarray(V.T).reshape(S, M0, M1)
        path = lambda v: pw.kp_right(pw.kp_left(inp['K'][0], v, False, LD)[0], inp['K'][1], False, LD)[0]
        e = _rel(path(ld['V']), path(V))
        print('KPATHW-PIN %s: cond %.2e, K0 V K1 against kron_weights_ld %.2e (bound %.1e)' % (fx[0], c, e, _bound(c)))
        assert e < _bound(c)
    for i, fx in enumerate(_kron_fixtures()):
        inp, seq = _kron(i)
        fail, fig = pw.check_kron(inp, seq, i < _N_DYADIC)
        worst = max(worst, fig['solve'])
        assert not fail, (fx[0], fail, fig)
    print('KPATHW-SOLVE-CPU unrefined float64 sequence, largest residual over the fixtures: %.2f eps S_w' % worst)


KRON_CLAIMS = {'w1_not_transposed': {'bound:B1'}, 'swap_left_right': {'bound:A1'}, 'fill_ij': {'exact:tab'}}


@pytest.mark.parametrize('mutation', pw.KRON_MUTATIONS)
def test_kron_mutations_are_caught(mutation):
    """As test_dense_mutations_are_caught, on every Kronecker fixture latent (the M0 != M1 grids among them)"""
    caught, unequal = 0, 0
    for i, fx in enumerate(_kron_fixtures()):
        inp, good = _kron(i)
        bad = pw.kron_sequence(inp['W'][0], inp['W'][1], inp['U'], inp['Sq'], inp['E'], inp['FZ'], inp['tab0'], mutate=mutation)
        if not _changed(good, bad):
            continue
        fail, fig = pw.check_kron(inp, bad, i < _N_DYADIC)
        assert KRON_CLAIMS[mutation] & set(fail), (mutation, fx[0], fail)
        caught += 1
        unequal += inp['FZ'].shape[1] != inp['FZ'].shape[2]
    print('KPATHW-MUTATION %s: caught on %d fixture latents, %d of them M0 != M1' % (mutation, caught, unequal))
    assert caught >= 3 and unequal >= 1
