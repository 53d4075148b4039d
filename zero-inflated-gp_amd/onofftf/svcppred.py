"""`predict_scgp` -- onofftf/svcppred.py:15-224 (Bernoulli / probit Kronecker classifier): returns {'pfmean','pfvar'}
(class-1 probability probit(fmean / sqrt(1 + fvar)) and its Bernoulli variance) for train (and test)."""
import numpy as np

from .heads import restore_and_predict

jitter_level = 1e-6   # onofftf/svcppred.py:13


def predict_scgp(Xtrain, Xtest, checkpointPath, num_inducing_f=np.array([10, 100]), include_f_mu=False, device=0, engine=None,
                 fused_matern=False):
    return restore_and_predict('bernoulli', Xtrain, Xtest, checkpointPath, num_inducing_f, include_f_mu,
                               (('pfmean', 2), ('pfvar', 3)), device=device, engine=engine, fused_matern=fused_matern)


def sample_scgp(Xtrain, Xtest, checkpointPath, num_samples, num_inducing_f=np.array([10, 100]), include_f_mu=False, n_features=1024, seed=None,
                draws=None, device=0, engine=None):
    """Joint posterior sample paths of the restored classifier at Xtest: {'f', 'p': (num_samples, N) each, 'draws'}; p is the class-1
    probability of each path through the reference's link (svcppred.py's probit with its 1e-3 clamp)."""
    from .heads import restore_and_sample
    return restore_and_sample('bernoulli', Xtrain, Xtest, checkpointPath, num_inducing_f, include_f_mu, num_samples, n_features=n_features,
                              seed=seed, draws=draws, device=device, engine=engine)
