"""`predict_svgp` -- onofftf/svgppred.py:15-203 (Gaussian-likelihood Kronecker SVGP): returns {'fmean','fvar'} for the
training inputs (and the test inputs when given)."""
import numpy as np

from .heads import restore_and_predict

jitter_level = 1e-6   # onofftf/svgppred.py:13


def predict_svgp(Xtrain, Xtest, checkpointPath, num_inducing_f=np.array([10, 100]), include_fmu=False, device=0, engine=None,
                 fused_matern=False):
    # include_fmu only defines an unused initial value in the reference (svgppred.py:26-27)
    return restore_and_predict('gaussian', Xtrain, Xtest, checkpointPath, num_inducing_f, False,
                               (('fmean', 0), ('fvar', 1)), device=device, engine=engine, fused_matern=fused_matern)       # :180-186


def sample_svgp(Xtrain, Xtest, checkpointPath, num_samples, num_inducing_f=np.array([10, 100]), n_features=1024, seed=None, draws=None,
                device=0, engine=None):
    """Joint posterior sample paths of the restored regression model at Xtest: {'f': (num_samples, N), 'draws'}"""
    from .heads import restore_and_sample
    return restore_and_sample('gaussian', Xtrain, Xtest, checkpointPath, num_inducing_f, False, num_samples, n_features=n_features, seed=seed,
                              draws=draws, device=device, engine=engine)
