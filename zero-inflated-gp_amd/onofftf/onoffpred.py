"""`predict_onoff` -- onofftf/onoffpred.py:15-286: rebuild the parameter set, restore the checkpoint, predict with
jitter 1e-6 (:13) and gmean shifted by -1 (:141); returns {'gfmean','fmean','pgmean'} for train (and test)."""
import os

import numpy as np

import zigp
from .model import init_params, engine_params, fused_matern_scope, load_checkpoint

jitter_level = 1e-6   # onofftf/onoffpred.py:13


def predict_onoff(Xtrain, Xtest, checkpointPath, num_inducing_f=np.array([10, 100]), num_inducing_g=np.array([10, 100]),
                  include_fmu=False, device=0, engine=None, fused_matern=False):
    # fused_matern: Matern factors of the restored model on the fused kernels for this call (DenseEngine.set_kron_matern_fused)
    # include_fmu has no effect in the reference either: its f_mu Param is commented out (onoffpred.py:27-28,89)
    pset = init_params(Xtrain, num_inducing_f, num_inducing_g, init_noisevar=0.001)
    ck = checkpointPath
    if os.path.isdir(ck):
        ck = os.path.join(ck, 'model')
    load_checkpoint(pset, ck)
    eng = engine or zigp.reference_engine(device)      # tf.cholesky's acceptance rule (pivot > 0)
    p = engine_params(pset)

    def run(X):
        o = eng.kron_predict(p, X, jitter=jitter_level, g_offset=-1.0)
        return {'gfmean': o[0].reshape(-1, 1), 'fmean': o[3].reshape(-1, 1), 'pgmean': o[7].reshape(-1, 1)}   # :273-280

    with fused_matern_scope(eng, fused_matern):
        pred_train = run(Xtrain)
        if Xtest is not None:
            return pred_train, run(Xtest)
        return pred_train


def sample_onoff(Xtrain, Xtest, checkpointPath, num_samples, num_inducing_f=np.array([10, 100]), num_inducing_g=np.array([10, 100]),
                 n_features=1024, seed=None, draws=None, device=0, engine=None):
    """Joint posterior sample paths of the restored model at Xtest, beside predict_onoff (same restore, jitter 1e-6, gmean shifted by
    -1): {'f', 'g', 'gf'}, each (num_samples, N) -- a row is one draw of the whole field, so sums over rows (basin or weekly totals)
    and sample maps come from it -- and 'draws', which gives the same paths at other inputs.  Xtrain only rebuilds the parameter set."""
    pset = init_params(Xtrain, num_inducing_f, num_inducing_g, init_noisevar=0.001)
    ck = checkpointPath
    if os.path.isdir(ck):
        ck = os.path.join(ck, 'model')
    load_checkpoint(pset, ck)
    eng = engine or zigp.reference_engine(device)
    return eng.kron_sample_paths(engine_params(pset), Xtest, n_samples=int(num_samples), n_features=n_features, rng=seed, draws=draws,
                                 jitter=jitter_level, g_offset=-1.0)


def score_onoff_paths(Xtrain, Xtest, Ytest, checkpointPath, groups=None, num_samples=16, num_inducing_f=np.array([10, 100]),
                      num_inducing_g=np.array([10, 100]), member='gf', noise_eps=None, weights=None, energy=True, totals=True, variogram=None,
                      fair=False, n_features=1024, seed=None, draws=None, device=0, engine=None):
    """Scores of the restored model's joint sample paths at Xtest against Ytest, beside sample_onoff (same restore, jitter 1e-6, gmean
    shifted by -1): the paths stay on the device and only the scores come back (DenseEngine.kron_path_scores_device) -- per group of
    `groups` (None, boundaries, or integer labels such as a basin or week index) the weighted totals of every member and of Ytest, the
    CRPS of the totals, the energy score and, with variogram = 0.5 / 1 / 2, the variogram score, as NumPy arrays, plus 'draws'.  The
    members are the noise-free paths unless noise_eps, (num_samples, N) standard normals, is given.  The reference logs RMSE / MAE only."""
    import torch
    pset = init_params(Xtrain, num_inducing_f, num_inducing_g, init_noisevar=0.001)
    ck = checkpointPath
    if os.path.isdir(ck):
        ck = os.path.join(ck, 'model')
    load_checkpoint(pset, ck)
    eng = engine or zigp.reference_engine(device)
    dev = torch.device('cuda', eng.device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Y = np.asarray(Ytest, dtype=np.float64).reshape(-1)
    r = eng.kron_path_scores_device(engine_params(pset), up(Xtest), up(Y), groups=groups, n_samples=int(num_samples), member=member,
                                    noise_eps=up(noise_eps), weights=up(weights), energy=energy, totals=totals, variogram=variogram, fair=fair,
                                    n_features=n_features, rng=seed, draws=draws, jitter=jitter_level, g_offset=-1.0)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in r.items()}
