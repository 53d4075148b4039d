"""OnOffSVGP(..., whiten=True, q_diag=False) on the toy model of zero-inflated-gpflow.ipynb (N = 450, M = 10 - 1): the model surface of
the full-covariance q(u) -- construction, ELBO and KL against the diagonal whitened model at the same point, L-BFGS-B and host Adam on the
LowerTriangular free state, pickle round trip, refusal of the unwhitened full-covariance model."""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _toy_model(q_diag, whiten=True, num_inducing=10, seed=0, minibatch_size=None):
    """zero-inflated-gpflow.ipynb:52-135 with the two switches."""
    import scipy.io as sio
    import onoffgpf
    from onoffgpf import OnOffSVGP, OnOffLikelihood
    mat = sio.loadmat(os.path.join(GOLD, 'toydata.mat'))
    X, Y = mat['x'], mat['y']
    kf = onoffgpf.kernels.RBF(1)
    kf.lengthscales = 2.
    kf.variance = 1.
    kg = onoffgpf.kernels.RBF(1)
    kg.lengthscales = 2.
    kg.variance = 5.
    Zf = np.delete(np.linspace(min(X), max(X), num_inducing, endpoint=False), 0).transpose().reshape(-1, 1)
    np.random.seed(seed)
    m = OnOffSVGP(X, Y, kernf=kf, kerng=kg, likelihood=OnOffLikelihood(), Zf=Zf, Zg=Zf.copy(), whiten=whiten, q_diag=q_diag,
                  minibatch_size=minibatch_size)
    m.likelihood.variance = 0.01
    m.likelihood.variance.fixed = False
    return m, X, Y


def test_initial_point_equals_the_diagonal_model():
    mf, X, Y = _toy_model(False)
    md, _, _ = _toy_model(True)
    M = mf.num_inducing_f
    assert mf.q_diag is False and mf.whiten is True and md.q_diag is True
    assert mf.u_fs_sqrt.value.shape == (M, M, 1) and np.array_equal(mf.u_fs_sqrt.value[:, :, 0], np.eye(M))
    assert mf.u_gs_sqrt.value.shape == (M, M, 1) and mf.u_fs_sqrt.free().size == M * (M + 1) // 2
    v = mf._values()
    assert v['q_diag'] is False and v['whiten'] is True and 'q_diag' not in md._values()
    assert not mf._device_fit_eligible(mf._pset())
    mf.u_fm, mf.u_gm = md.u_fm.value, md.u_gm.value
    a, b = mf.compute_log_likelihood(), md.compute_log_likelihood()
    ka, kb = mf.compute_prior_KL(), md.compute_prior_KL()
    print('toy ELBO full %.12e diagonal %.12e; KL %.12e / %.12e' % (a, b, ka, kb))
    assert abs(a - b) <= 1e-10 * abs(b) and abs(ka - kb) <= 1e-10 * abs(kb)
    out_f, out_d = mf.predict_onoffgp(X), md.predict_onoffgp(X)
    assert len(out_f) == 9 and all(o.shape == (X.shape[0], 1) for o in out_f)
    for i in range(9):
        assert np.max(np.abs(out_f[i] - out_d[i])) <= 1e-9 * max(np.max(np.abs(out_d[i])), 1e-300), i


def test_optimize_keeps_the_factor_lower_triangular():
    m, X, Y = _toy_model(False)
    M = m.num_inducing_f
    e0 = m.compute_log_likelihood()
    m.optimize(maxiter=25)
    e1 = m.compute_log_likelihood()
    print('toy full-covariance ELBO %.6f -> %.6f after 25 L-BFGS-B iterations' % (e0, e1))
    assert e1 > e0
    for q in (m.u_fs_sqrt, m.u_gs_sqrt):
        L = q.value
        assert L.shape == (M, M, 1) and np.all(np.triu(L[:, :, 0], 1) == 0.0) and np.any(np.tril(L[:, :, 0], -1) != 0.0)


def test_full_family_reaches_at_least_the_diagonal_optimum():
    """The diagonal family is a subset of the full one (same starting point: Lq = I), so after optimize(maxiter=300) on both the full
    model's ELBO is not below the diagonal model's; 1e-6 (relative) for the optimiser's stopping rule."""
    mf, _, _ = _toy_model(False)
    md, _, _ = _toy_model(True)
    mf.u_fm, mf.u_gm = md.u_fm.value, md.u_gm.value
    mf.optimize(maxiter=300)
    md.optimize(maxiter=300)
    ef, ed = mf.compute_log_likelihood(), md.compute_log_likelihood()
    print('toy ELBO after 300 iterations: full %.8f diagonal %.8f' % (ef, ed))
    assert ef >= ed - 1e-6 * abs(ed)


def test_host_adam_with_minibatches_never_calls_the_device_loop(monkeypatch):
    m, X, Y = _toy_model(False, minibatch_size=100)
    calls = []
    monkeypatch.setattr(type(m._engine), 'fit_steps', lambda self, *a, **k: calls.append(1))
    before = m.u_fs_sqrt.value.copy()
    m.optimize(method='adam', maxiter=20, learning_rate=1e-3)
    assert not calls
    L = m.u_fs_sqrt.value
    assert L.shape == before.shape and not np.array_equal(L, before) and np.all(np.triu(L[:, :, 0], 1) == 0.0)
    assert np.isfinite(m.compute_log_likelihood())


def test_pickle_round_trip(tmp_path):
    m, X, Y = _toy_model(False)
    m.optimize(maxiter=5)
    f = m.savemodel(str(tmp_path / 'm.pickle'))
    m2 = pickle.load(open(f, 'rb'))
    assert m2.q_diag is False and m2.whiten is True and np.array_equal(m2.u_fs_sqrt.value, m.u_fs_sqrt.value)
    a = m.compute_log_likelihood()
    assert abs(m2.compute_log_likelihood() - a) <= 1e-12 * abs(a)
    # a pickle from before the switch existed has no q_diag: it loads as the diagonal model
    md, _, _ = _toy_model(True)
    state = md.__getstate__()
    del state['q_diag']
    old = md.__class__.__new__(md.__class__)
    old.__setstate__(state)
    assert old.q_diag is True and abs(old.compute_log_likelihood() - md.compute_log_likelihood()) <= 1e-12 * abs(a)


def test_unwhitened_full_covariance_is_refused():
    with pytest.raises(NotImplementedError, match='whiten'):
        _toy_model(False, whiten=False)
