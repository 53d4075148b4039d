"""Stage-level parity of the weight stage of the sample paths -- what turns a draw of q(u) into the weight table the path kernels read
(csrc/zigp_paths.hip path_weight_stage; csrc/zigp_kronpaths.hip kron_path_weight_stage) -- launch by launch, through
zigp_test_path_weights / zigp_test_kron_path_weights (include/zigp_diag.h): the product's own host function with a device-to-device
snapshot behind every launch.  tests/path_weights_ref.py restates each launch on its tapped operands; tests/test_cpu_path_weights_ref.py
shows on the CPU that each of twelve deliberate mistakes fails the tier that claims it on these fixtures.

  exact tier   k_path_rhs (three modes), k_kp_rhs, both k_path_axpy uses, k_path_fill_v, k_kp_fill_v: == the float64 restatement, no
               sentinel left, exact zeros in every padding (u, s and eps are dyadic: fma(s, eps, u) and s eps + u are one number)
  bound tier   every path_gemm product and every k_kp_left / k_kp_right launch: err_gpu <= 4 err_np + 16 eps S per element against the
               long-double restatement on the tapped operands
  solve tier   dense Diag: max |rhs - Kuu V| <= 8 x that of scipy.linalg.cho_solve on the same float64 operands -- the tier that holds the
               refinement step V += W^T W (rhs - Kuu V): without it the g latent of solve_1d is at 46 x (float64 NumPy in the device's place,
               test_cpu_path_weights_ref.py).  Kronecker: rhs_s - K0 V_s K1 <= 4 res_np + 16 eps S_w per element, WITHOUT a refinement step.
  composition  the tapped V with the restated omega and amp through path_rows / kron_path_rows equals sample_paths / kron_sample_paths /
               kron_head_sample_paths with the same draws bit for bit: the hook is the product's stage, the device-built table the host-built.

Every figure is printed (the PATHW- lines of a run are profiles/path_weights_parity.log)."""
import math

import numpy as np
import pytest

import path_weights_ref as pw
import kronpaths_ref as kr

pytestmark = pytest.mark.gpu


def _fmt(fig):
    return ' '.join('%s %.2f' % (k, v) for k, v in fig.items())


def _padded_identity(A, M, what):
    assert np.all(A[:M, M:] == 0) and np.all(A[M:, :M] == 0) and np.array_equal(A[M:, M:], np.eye(A.shape[0] - M)), what


@pytest.mark.parametrize('name', list(pw.DENSE_CASES))
def test_dense_weight_stage(engine, name):
    """Every launch of the dense stage for both latents of a case: the exact, bound and solve tiers of path_weights_ref.check_dense on the
    taps; the staged inputs as the device holds them; exact zeros outside (M, S) of every (Mp, Sp) output and outside (S, M) of f_Z; no
    sentinel in any tap (A, B, V and the kernel rows of the table are sentinel-filled before the stage); the padding of Kuu and W"""
    k = pw.DENSE_CASES[name]
    p, draws = pw.dense_problem(name)
    S, mode = k['S'], k['mode']
    r = engine.test_path_weights(p, draws, S, jitter=pw.DENSE_JITTER)
    assert r['facts']['mode'] == mode and (r['facts']['nst'], r['facts']['ntile']) == pw.tiles(S)
    for h, tag in enumerate('fg'):
        tap = r['lat'][h]
        M = p['Z' + tag].shape[0]
        for key, a in tap.items():
            assert np.all(np.isfinite(a)) and not np.any(a == pw.SENT), (tag, key)
        _padded_identity(tap['Kuu'], M, 'Kuu')
        _padded_identity(tap['W'], M, 'W')
        assert np.all(np.triu(tap['W'], 1) == 0)
        var = float(np.squeeze(p['var_' + tag]))
        # k(z, z) = var up to the Matern floor (1.5e-12 var): the diagonal the residual is taken against carries the jitter
        assert np.all(np.abs(np.diag(tap['Kuu'])[:M] - (var + pw.DENSE_JITTER)) <= 1e-10 * var)
        E = np.zeros_like(tap['E'])
        E[:M, :S] = draws[tag]['eps']
        assert np.array_equal(tap['E'], E)
        u = np.zeros(tap['u'].shape)
        u[:M] = np.asarray(p['u_%sm' % tag]).reshape(-1)
        sq = np.asarray(p['u_%ss_sqrt' % tag])
        s = np.zeros(tap['s'].shape)
        s[:M] = np.diag(sq) if mode == 2 else sq.reshape(-1)
        assert np.array_equal(tap['u'], u) and np.array_equal(tap['s'], s)
        if mode == 2:
            Lq = np.zeros_like(tap['Lq'])
            Lq[:M, :M] = np.tril(sq)
            assert np.array_equal(tap['Lq'], Lq)
        ft = tap['FT'].copy()
        ft[:S, :M] = 0
        assert np.all(ft == 0)
        out = {}
        for key, a in tap.items():
            if key in ('rhs', 't', 'V0', 'KV', 'res', 't2', 'cor', 'G', 'H', 'V'):
                z = a.copy()
                z[:M, :S] = 0
                assert np.all(z == 0), (tag, key)
                out[key] = a[:M, :S]
        out['tab'] = tap['tab']
        inp = pw.dense_tap_inputs(name, h, tap)
        fail, fig = pw.check_dense(mode, inp, out, k['quant'])
        line = 'PATHW-DENSE %s %s mode %d M=%d S=%d R=%d: err / (eps S): %s' % (name, tag, mode, M, S, k['R'], _fmt(fig))
        if mode == 0:
            before = pw.solve_ratio(inp['Kuu'], out['rhs'], out['V0'])
            line += ' | residual x SciPy: refined %.2f, before the refinement %.2f' % (fig['solve'], before)
        print(line)
        assert not fail, line
        if name == 'solve_1d' and tag == 'g':      # the ill-conditioned latent: the step does its work
            assert pw.residual_ld(inp['Kuu'], out['rhs'], out['V0']) > pw.residual_ld(inp['Kuu'], out['rhs'], out['V'])


def _dense_latents(p, draws, taps, S):
    lats = []
    for h, tag in enumerate('fg'):
        Z = np.asarray(p['Z' + tag])
        M, D = Z.shape
        ell = np.broadcast_to(np.asarray(p['ell_' + tag], dtype=np.float64).reshape(-1), (D,)).copy()
        var, d = float(np.squeeze(p['var_' + tag])), draws[tag]
        R = int(d['R'])
        lats.append(dict(kind=p.get('kern_' + tag, 'rbf'), Z=Z, ell=ell, var=var, V=np.ascontiguousarray(taps[h]['V'][:M, :S]),
                         omega=d['omega0'] / ell[None, :], phase=d['phase'], amp=d['a'] * (math.sqrt(2.0 * var / R) if R else 0.0)))
    return lats


@pytest.mark.parametrize('name', ['m50_37', 's1', 's33_matern', 'modes_diag', 'modes_white', 'modes_full', 's256'])
def test_dense_composition(engine, name):
    """path_rows on the tapped final V with omega = omega0 / ell and amp = a sqrt(2 var / R) restated on the host == sample_paths with the
    same draws, f and g bit for bit (S = 129 and S = 256 among the cases); a second hook call returns the same bits"""
    p, draws = pw.dense_problem(name)
    S = pw.DENSE_CASES[name]['S']
    r = engine.test_path_weights(p, draws, S, jitter=pw.DENSE_JITTER)
    X = np.random.RandomState(5).rand(70, p['Zf'].shape[1])
    got = engine.sample_paths(p, X, n_samples=S, draws=draws, jitter=pw.DENSE_JITTER)
    rows = engine.path_rows(_dense_latents(p, draws, r['lat'], S), X, S)
    assert np.array_equal(rows[0], got['f']) and np.array_equal(rows[1], got['g'])
    again = engine.test_path_weights(p, draws, S, jitter=pw.DENSE_JITTER)
    for h in range(2):
        for key, a in r['lat'][h].items():
            assert np.array_equal(a, again['lat'][h][key]), key


def test_hooks_refuse_bad_arguments_by_name(engine, monkeypatch):
    """S beyond ZIGP_PATH_MAX_S and a negative jitter are refused with the hook's name, and the context goes on working"""
    from zigp import pathwise
    p, draws = pw.dense_problem('m50_37')
    with pytest.raises(ValueError, match='zigp_test_path_weights: jitter must be >= 0'):
        engine.test_path_weights(p, draws, 20, jitter=-1.0)
    kp, kdraws, tags = pw.kron_problem('k3x5_s17')
    with pytest.raises(ValueError, match='zigp_test_kron_path_weights: jitter must be >= 0'):
        engine.test_kron_path_weights(kp, kdraws, 17, jitter=-1.0)
    big = {t: dict(d, a=np.zeros((d['R'], 300)), eps=np.zeros((d['eps'].shape[0], 300))) for t, d in draws.items()}
    kbig = {t: dict(d, a=np.zeros((d['R'], 300)), eps=np.zeros((d['eps'].shape[0], 300))) for t, d in kdraws.items()}
    monkeypatch.setattr(pathwise, 'check_sizes', lambda D, S: None)
    monkeypatch.setattr(pathwise, 'check_kron_sizes', lambda *a: None)
    with pytest.raises(ValueError, match=r'zigp_test_path_weights: S = 300 must be in \[1, 256\]'):
        engine.test_path_weights(p, big, 300)
    with pytest.raises(ValueError, match=r'zigp_test_kron_path_weights: S = 300 must be in \[1, 256\]'):
        engine.test_kron_path_weights(kp, kbig, 300)
    monkeypatch.undo()
    a = engine.test_path_weights(p, draws, 20, jitter=pw.DENSE_JITTER)
    assert not np.any(a['lat'][0]['V'] == pw.SENT) and np.all(np.isfinite(a['lat'][1]['tab']))


# ---- Kronecker ------------------------------------------------------------------------------------------------------------------------------
def _kron_check(name, p, draws, tags, r, S, dyadic=True):
    worst = {}
    for h, tag in enumerate(tags):
        tap = r['lat'][h]
        M0, M1 = p['Z' + tag][0].shape[0], p['Z' + tag][1].shape[0]
        for key, a in tap.items():
            for b in (a if isinstance(a, list) else [a]):
                assert np.all(np.isfinite(b)) and not np.any(b == pw.SENT), (tag, key)
        assert np.array_equal(tap['E'], draws[tag]['eps'])
        assert np.array_equal(tap['U'], np.asarray(p['u_%sm' % tag]).reshape(-1)) and np.array_equal(tap['Sq'], np.asarray(p['u_%ss_sqrt' % tag]).reshape(-1))
        for q, M in enumerate((M0, M1)):
            _padded_identity(tap['K'][q], M, 'K')
            _padded_identity(tap['W'][q], M, 'W')
        inp = pw.kron_tap_inputs(p, draws, tag, tap, S)
        fail, fig = pw.check_kron(inp, tap, dyadic)
        line = 'PATHW-KRON %s %s %dx%d S=%d: err / (eps S): %s' % (name, tag, M0, M1, S, _fmt(fig))
        print(line)
        assert not fail, line
        worst[tag] = fig
    return worst


@pytest.mark.parametrize('name', list(pw.KRON_CASES))
def test_kron_weight_stage(engine, name):
    """Every launch of the Kronecker stage for every latent of a case (the on/off model and both heads): k_kp_rhs and k_kp_fill_v with ==,
    the four k_kp_left / k_kp_right launches under the bound rule, the residual rhs_s - K0 V_s K1 under the solve rule; the staged
    inputs as the device holds them; no sentinel anywhere (every work matrix is sentinel-filled before the stage)"""
    k = pw.KRON_CASES[name]
    p, draws, tags = pw.kron_problem(name)
    r = engine.test_kron_path_weights(p, draws, k['S'], lik=k['lik'], jitter=pw.KRON_JITTER)
    assert (r['facts']['nst'], r['facts']['ntile']) == pw.tiles(k['S'])
    _kron_check(name, p, draws, tags, r, k['S'])


@pytest.mark.parametrize('name', pw.KRON_SOLVE_CASES)
def test_kron_weights_need_no_refinement(engine, name):
    """The design claim of zigp_kronpaths.hip -- each W_p belongs to one factor, the weights need no refinement step -- as a test: on
    the five model cases with their seeded draws (R = 200, S = 20) and on the precipitation data's 32 x 32 initialisation, the residual of
    the device's V is within 4 res_np + 16 eps S_w per element, S_w = |K0| |V_s| |K1| + |rhs_s|, res_np the float64 restatement in the
    kernels' order on the tapped W_p; the launches' own tiers with real u, s and eps"""
    p, draws, S, jitter = pw.kron_solve_problem(name)
    r = engine.test_kron_path_weights(p, draws, S, jitter=jitter)
    fig = _kron_check(name, p, draws, 'fg', r, S, dyadic=False)
    print('PATHW-KRON-SOLVE %s: residual / (eps S_w) f %.2f (NumPy %.2f), g %.2f (NumPy %.2f)' % (
        name, fig['f']['solve'], fig['f']['solve_np'], fig['g']['solve'], fig['g']['solve_np']))


def _kron_latents(p, draws, tags, taps, S):
    lats = []
    for h, tag in enumerate(tags):
        Z = [np.asarray(z) for z in p['Z' + tag]]
        ell = [np.broadcast_to(np.asarray(p['ell_' + tag][q], dtype=np.float64).reshape(-1), (Z[q].shape[1],)).copy() for q in range(2)]
        var, d = [float(np.squeeze(v)) for v in p['var_' + tag]], draws[tag]
        R = int(d['R'])
        lat = dict(Z=Z, ell=ell, var=var, V=np.ascontiguousarray(taps[h]['V'].reshape(S, -1).T), omega=d['omega0'] / np.concatenate(ell)[None, :],
                   phase=d['phase'], amp=d['a'] * (math.sqrt(2.0 * (var[0] * var[1]) / R) if R else 0.0))
        if 'kern_' + tag in p:
            lat['kinds'] = p['kern_' + tag]
        lats.append(lat)
    return lats


@pytest.mark.parametrize('name', ['k1x1', 'k3x5_s129', 'k32x32', 'k16x112', 'k10x100_matern'])
def test_kron_composition(engine, name):
    """kron_path_rows on the tapped V with the restated omega and amp == kron_sample_paths / kron_head_sample_paths with the same draws,
    bit for bit (S = 129 among the cases); the Bernoulli head's probability plane -- the output of k_kp_probit, whose input is the f plane
    of the same call -- under the bound rule against the long-double link, S = the link's constants and its erf term times 1 + |f|"""
    k = pw.KRON_CASES[name]
    p, draws, tags = pw.kron_problem(name)
    S, D = k['S'], sum(k['D'])
    r = engine.test_kron_path_weights(p, draws, S, lik=k['lik'], jitter=pw.KRON_JITTER)
    X = np.random.RandomState(6).rand(70, D)
    rows = engine.kron_path_rows(_kron_latents(p, draws, tags, r['lat'], S), X, S, k['D'])
    if k['lik'] == 'onoff':
        got = engine.kron_sample_paths(p, X, n_samples=S, draws=draws, jitter=pw.KRON_JITTER)
        assert np.array_equal(rows[0], got['f']) and np.array_equal(rows[1], got['g'])
        return
    got = engine.kron_head_sample_paths(p, X, k['lik'], n_samples=S, draws=draws, jitter=pw.KRON_JITTER)
    assert np.array_equal(rows[0], got['f'])
    if k['lik'] == 'bernoulli':
        from scipy.special import erf
        f = got['f']
        truth = kr.link_ld(f)
        mag = 0.5 * (1 - 2e-3) + 1e-3 + 0.5 * (1 - 2e-3) * np.abs(erf(f * 0.70710678118654752440)) * (1 + np.abs(f))
        ok, ratio = pw.bound_ok(got['p'], kr.paths_ref.link(f), truth, mag)
        print('PATHW-KRON %s k_kp_probit: err / (eps S) %.2f' % (name, ratio))
        assert ok
