"""gpflow.likelihoods look-alikes for onoffgpf.SVGP (GPflow 0.4.0): the two likelihoods of the reference's baselines.  `lik` is the engine's
name of the head (DenseEngine.head_elbo / head_predict, zigp_head_elbo)."""
import numpy as np

from zigp.transforms import positive
from .param import Param, Parameterized


class Likelihood(Parameterized):
    lik = None


class Gaussian(Likelihood):
    """y | f ~ N(f, variance) (gpflow.likelihoods.Gaussian: variance = 1.0, positive); scripts/svgp.py:198-200."""
    lik = 'gaussian'

    def __init__(self, variance=1.0):
        self.variance = Param(variance, positive)

    def variational_expectations(self, Fmu, Fvar, Y):
        """Closed form on host arrays (for inspection; the engine's point-wise kernel fuses it)."""
        v = float(self.variance.value.reshape(-1)[0])
        return -0.5 * np.log(2 * np.pi) - 0.5 * np.log(v) - 0.5 * (np.square(Y - Fmu) + Fvar) / v


class Bernoulli(Likelihood):
    """P(y = 1 | f) = probit(f) through the reference's clamp, p = Phi(x) (1 - 2e-3) + 1e-3 (scripts/classifier.py:216-217); the label 1 is
    'on', anything else 'off' (tf.equal(y, 1), :214).  The bound uses the closed form of E_q[probit(f)], p at x = fmean / sqrt(1 + fvar)
    (:139), as the reference's classifier does -- not GPflow's Gauss-Hermite expectation of log p.  No parameters."""
    lik = 'bernoulli'

    def variational_expectations(self, Fmu, Fvar, Y):
        from scipy.special import erf
        p = 0.5 * (1.0 + erf(Fmu / np.sqrt(1.0 + Fvar) / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
        return np.log(np.where(Y == 1, p, 1 - p))
