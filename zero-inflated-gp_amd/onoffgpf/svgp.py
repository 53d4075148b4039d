"""gpflow.svgp.SVGP look-alike (GPflow 0.4.0) on the dense engine's heads: ONE latent f under likelihoods.Gaussian or likelihoods.Bernoulli
-- the baselines the reference compares its zero-inflated model against (scripts/svgp.py, scripts/classifier.py; scripts/hurdle.py is
two of these), here for scattered inducing inputs, D up to 64 and the Matern kernels (DenseEngine.head_elbo / head_predict,
zigp_head_elbo).

  SVGP(X, Y, kern, likelihood, Z, mean_function=None, q_diag=False, whiten=True, minibatch_size=None)     GPflow's names and defaults
  .Z .q_mu .q_sqrt .kern.lengthscales .kern.variance .likelihood.variance (Gaussian)
  .compute_log_likelihood() .compute_prior_KL() .optimize() .predict_f() .predict_y() .predict_density()

num_latent is 1.  The unwhitened full-covariance model (q_diag=False, whiten=False) raises NotImplementedError, as OnOffSVGP does.
optimize(method='adam') runs the host loop (the device fit loops fit the OnOff model).  Minibatches, the row sampling rule, the free-state
packing and the optimisers are OnOffSVGP's (zigp/optim.py).
"""
from collections import OrderedDict

import numpy as np

import zigp
from zigp.optim import ParamSet, lbfgsb, AdamGroups
from zigp.transforms import positive, LowerTriangular
from zigp._lib import MAX_D, DEVICE_FIT_MAX_D, KERNELS, MATERN_MAX_D
from .param import Param, DataHolder, Parameterized
from .mean_functions import MeanFunction, Zero, Linear
from .likelihoods import Likelihood
from .OnOffSVGP import OnOffSVGP, JITTER


class SVGP(Parameterized):
    def __init__(self, X, Y, kern, likelihood, Z, mean_function=None, q_diag=False, whiten=True, minibatch_size=None, name='svgp', device=0):
        self.mean_function = mean_function or Zero()
        if not isinstance(self.mean_function, MeanFunction):
            raise TypeError('mean_function must be an onoffgpf.mean_functions.{Zero, Constant, Linear}')
        if not isinstance(likelihood, Likelihood) or likelihood.lik not in ('gaussian', 'bernoulli'):
            raise TypeError('likelihood must be an onoffgpf.likelihoods.Gaussian or Bernoulli (the OnOff likelihood belongs to OnOffSVGP)')
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise ValueError('Y must be (N,1): num_latent is 1')
        if X.ndim != 2 or not 1 <= X.shape[1] <= MAX_D or X.shape[0] != Y.shape[0]:
            raise ValueError('X must be (N, D) with 1 <= D <= %d and as many rows as Y, not %s' % (MAX_D, X.shape))
        if X.shape[1] > DEVICE_FIT_MAX_D and type(self.mean_function) is Linear:
            raise ValueError('a Linear mean function covers D <= %d input columns (D = %d); Zero and Constant work at every D'
                             % (DEVICE_FIT_MAX_D, X.shape[1]))
        kind = getattr(kern, 'kind', 'rbf')
        if kind not in KERNELS:
            raise ValueError('kern has the unknown kernel kind %r: onoffgpf.kernels has RBF, Matern32 and Matern52' % (kind,))
        if kind != 'rbf' and X.shape[1] > MATERN_MAX_D:
            raise ValueError('kern is a %s kernel and D = %d: the Matern kernels cover D <= %d input columns'
                             % (type(kern).__name__, X.shape[1], MATERN_MAX_D))
        self.whiten, self.q_diag = bool(whiten), bool(q_diag)
        if not self.q_diag and not self.whiten:
            raise NotImplementedError('q_diag=False is implemented for the whitened model only (whiten=True); the unwhitened '
                                      'full-covariance q(u) is not')
        Z = np.array(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError('Z must be (M, %d), not %s' % (X.shape[1], Z.shape))
        self.name = name
        self.kern, self.likelihood = kern, likelihood
        self.X, self.Y = DataHolder(X), DataHolder(Y)
        self.Xtrain, self.Ytrain = self.X, self.Y                    # the names OnOffSVGP's row plumbing reads
        self.num_data, self.num_latent = X.shape[0], 1
        self.minibatch_size = self.num_data if minibatch_size is None else int(minibatch_size)
        self._rng = np.random.RandomState(0)
        self.Z = Param(Z)
        self.num_inducing = Z.shape[0]
        self.q_mu = Param(np.zeros((self.num_inducing, 1)))          # gpflow.svgp.SVGP: zeros / ones / identity
        if self.q_diag:
            self.q_sqrt = Param(np.ones((self.num_inducing, 1)), positive)
        else:
            self.q_sqrt = Param(np.eye(self.num_inducing)[:, :, None], LowerTriangular(self.num_inducing))
        self._device = int(device)
        self._engine_obj = None
        self._resident = False

    @property
    def _engine(self):
        """made at the first call that needs the GPU (raises if libzigp.so / the GPU is missing: no CPU fallback)"""
        if self._engine_obj is None:
            self._engine_obj = zigp.reference_engine(self._device)
        return self._engine_obj

    # ---- parameter plumbing (OnOffSVGP's, for one latent) ----
    def _pset(self):
        items = [('Zf', self.Z), ('u_fm', self.q_mu), ('u_fs_sqrt', self.q_sqrt), ('ell_f', self.kern.lengthscales), ('var_f', self.kern.variance)]
        if self.likelihood.lik == 'gaussian':
            items.append(('noise', self.likelihood.variance))
        return ParamSet(OrderedDict(items + list(self.mean_function.trainables().items())))

    def _values(self):
        a, b = self.mean_function.linear_form(self.X.value.shape[1])
        v = {k: w for k, w in (('mean_a', a), ('mean_b', b)) if w is not None}
        if self.whiten:
            v['whiten'] = True
        if not self.q_diag:
            v['q_diag'] = False
        if getattr(self.kern, 'kind', 'rbf') != 'rbf':
            v['kern_f'] = self.kern.kind
        v.update(Zf=self.Z.value, u_fm=self.q_mu.value, u_fs_sqrt=self.q_sqrt.value, ell_f=self.kern.ell_vector(),
                 var_f=float(self.kern.variance.value.reshape(-1)[0]))
        if self.likelihood.lik == 'gaussian':
            v['noise'] = float(self.likelihood.variance.value.reshape(-1)[0])
        return v

    def _fold_grads(self, g):
        """engine gradient -> the shapes of the Params (a scalar lengthscale sums its D copies)"""
        out = dict(g)
        if self.kern.lengthscales.value.size == 1:
            out['ell_f'] = np.array([np.sum(g['ell_f'])])
        for k in ('var_f', 'noise'):
            out[k] = np.array([g[k]])
        if not self.q_diag:
            out['u_fs_sqrt'] = np.asarray(g['u_fs_sqrt'])[:, :, None]
        if 'mean_b' in g:
            out['mean_b'] = np.array([g['mean_b']])
        return out

    _sample_rows = OnOffSVGP._sample_rows
    _make_resident = OnOffSVGP._make_resident
    _load_batch = OnOffSVGP._load_batch

    def _elbo(self, need_grad):
        scale = self._load_batch()
        ed, kl, g = self._engine.head_elbo(self._values(), self.likelihood.lik, jitter=JITTER, scale=scale, need_grad=need_grad)
        return ed - kl, (self._fold_grads(g) if need_grad else None)

    # ---- GPflow's surface ----
    def compute_log_likelihood(self):
        """the bound: scaled expected log-likelihood minus KL[q(u) || p(u)]"""
        return self._elbo(False)[0]

    def compute_prior_KL(self):
        """KL[q(u) || p(u)] of latent f (a value-only call on one resident row: the KL does not depend on the rows)"""
        self._make_resident()
        self._engine.select_rows(None)
        return self._engine.head_elbo(self._values(), self.likelihood.lik, jitter=JITTER, rows=(0, 1), need_grad=False)[1]

    def optimize(self, method='L-BFGS-B', maxiter=1000, disp=False, callback=None, learning_rate=0.01, **kw):
        """GPflow Model.optimize: scipy L-BFGS-B on the free state (default), or Adam when method='adam' -- every iteration a host step
        (select_rows + head_elbo + AdamGroups); the device fit loops do not take the heads."""
        pset = self._pset()
        if str(method).lower() in ('l-bfgs-b', 'lbfgsb'):
            return lbfgsb(pset, lambda _values: self._elbo(True), maxiter=maxiter, disp=disp, callback=callback, **kw)
        if str(method).lower() == 'adam':
            for p in pset.params.values():
                p.learning_rate = learning_rate
            opt = AdamGroups(pset)
            for it in range(maxiter):
                elbo, g = self._elbo(True)
                opt.step(g)
                if callback is not None:
                    callback(it, elbo)
            return None
        raise ValueError('unknown method %r' % (method,))

    def _predict(self, Xnew):
        return self._engine.head_predict(self._values(), np.asarray(Xnew, dtype=np.float64), self.likelihood.lik, jitter=JITTER)

    def predict_f(self, Xnew):
        """mean and variance of the latent f at Xnew (mean function included), each (N,1)"""
        out = self._predict(Xnew)
        return out[0].reshape(-1, 1), out[1].reshape(-1, 1)

    def predict_y(self, Xnew):
        """mean and variance of y at Xnew, each (N,1) -- Gaussian: fmean, fvar + variance; Bernoulli: p, p - p^2"""
        out = self._predict(Xnew)
        return out[2].reshape(-1, 1), out[3].reshape(-1, 1)

    def predict_density(self, Xnew, Ynew):
        """log p(Ynew | Xnew) per row, (N,1): the rows of head_predict through the engine's density_rows (closed form for both heads)"""
        out = self._predict(Xnew)
        noise = float(self.likelihood.variance.value.reshape(-1)[0]) if self.likelihood.lik == 'gaussian' else 1.0
        rows, _ = self._engine.density_rows(self.likelihood.lik, out[0], out[1], None, None, np.asarray(Ynew, dtype=np.float64).reshape(-1), noise)
        return rows[0].reshape(-1, 1)

    def __getstate__(self):
        d = dict(self.__dict__)
        d['_engine_obj'] = None
        d['_resident'] = False
        return d
