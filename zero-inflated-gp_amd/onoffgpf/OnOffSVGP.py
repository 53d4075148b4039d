"""OnOffSVGP look-alike (onoffgpf/OnOffSVGP.py:18-204) driving the MI355X engine through the C-ABI.

Same constructor signature, attributes and methods the reference exposes / its notebook and plotter use:
  OnOffSVGP(X, Y, kernf, kerng, likelihood, Zf, Zg, mean_function=None, minibatch_size=None, name='model')
  .optimize(maxiter=...)  .compute_log_likelihood()  .predict_onoffgp(Xnew)  .compute_prior_KL()  .savemodel(fname)
  .Xtrain .Ytrain .Zf .Zg .u_fm .u_gm .u_fs_sqrt .u_gs_sqrt .kernf .kerng .likelihood.variance
q_diag=True is hard-coded in the reference (:33-34) and so is whiten=False there, although build_prior_KL and build_predict carry the
whitened branch (:88-91,133,137): here `whiten` is a trailing keyword (default False) that switches the engine to the whitened
parametrisation q(u) = N(L u_m, L diag(u_s_sqrt^2) L^T), L = chol(Kuu).  `q_diag` (trailing keyword, default True) opens the other
switch for the whitened model: q_diag=False makes u_*s_sqrt (M, M, 1) lower-triangular factors (transforms.LowerTriangular, identity at
the start, :65-71) and q(u) = N(L u_m, L Lq Lq^T L^T) (gauss_kl_white, :88-89; the 3-d q_sqrt branch of the conditional).  The
unwhitened full-covariance model (gauss_kl, :102-104) is not implemented: q_diag=False with whiten=False raises NotImplementedError.  mean_function (:29,134): onoffgpf.mean_functions.Zero
(default), Constant or Linear -- evaluated, and differentiated, inside the engine's point-wise kernel.
kernf / kerng: onoffgpf.kernels.RBF, Matern32 or Matern52, each latent its own (:22); a Matern latent covers D <= 8 input columns and is
fitted by L-BFGS-B or the host Adam loop (the device fit loops fit RBF latents).
"""
import pickle
import time
from collections import OrderedDict

import numpy as np

import zigp
from zigp.optim import ParamSet, lbfgsb, AdamGroups, DenseDeviceFit, WhiteDeviceFit
from zigp.transforms import positive, Log1pe, Identity, LowerTriangular
from .param import Param, DataHolder, Parameterized
from .mean_functions import MeanFunction, Zero, Linear
from zigp._lib import MAX_D, DEVICE_FIT_MAX_D, KERNELS, MATERN_MAX_D

JITTER = 1e-6   # gpflow settings.numerics.jitter_level default (OnOffSVGP.py:96-97) [GPflow-recall]
DEVICE_FIT_CALL = 200   # iterations per zigp_fit_steps / zigp_fit_steps_mode call of optimize(method='adam'): one synchronisation each


class OnOffSVGP(Parameterized):
    def __init__(self, X, Y, kernf, kerng, likelihood, Zf, Zg, mean_function=None, minibatch_size=None, name='model',
                 device=0, whiten=False, q_diag=True):
        self.mean_function = mean_function or Zero()                 # :29
        if not isinstance(self.mean_function, MeanFunction):
            raise TypeError('mean_function must be an onoffgpf.mean_functions.{Zero, Constant, Linear}')
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise ValueError('Y must be (N,1): num_latent is 1 (OnOffSVGP.py:45)')
        if X.ndim != 2 or not 1 <= X.shape[1] <= MAX_D:
            raise ValueError('X must be (N, D) with 1 <= D <= %d, not %s' % (MAX_D, X.shape))
        if X.shape[1] > DEVICE_FIT_MAX_D and type(self.mean_function) is Linear:
            raise ValueError('a Linear mean function covers D <= %d input columns (D = %d); Zero and Constant work at every D'
                             % (DEVICE_FIT_MAX_D, X.shape[1]))
        for tag, kern in (('kernf', kernf), ('kerng', kerng)):
            kind = getattr(kern, 'kind', 'rbf')
            if kind not in KERNELS:
                raise ValueError("%s has the unknown kernel kind %r: onoffgpf.kernels has RBF, Matern32 and Matern52" % (tag, kind))
            if kind != 'rbf' and X.shape[1] > MATERN_MAX_D:
                raise ValueError('%s is a %s kernel and D = %d: the Matern kernels cover D <= %d input columns'
                                 % (tag, type(kern).__name__, X.shape[1], MATERN_MAX_D))
        self.name = name
        self.kernf, self.kerng, self.likelihood = kernf, kerng, likelihood
        self.whiten, self.q_diag = bool(whiten), bool(q_diag)        # :33-34 (whiten: the branch of :88-91,133,137; q_diag: :59-71,88-89)
        if not self.q_diag and not self.whiten:
            raise NotImplementedError('q_diag=False is implemented for the whitened model only (whiten=True); the unwhitened '
                                      'full-covariance q(u) (gauss_kl, OnOffSVGP.py:102-104) is not')
        self.Xtrain, self.Ytrain = DataHolder(X), DataHolder(Y)      # :37-39
        self.num_data = X.shape[0]
        self.num_latent = Y.shape[1]
        self.minibatch_size = self.num_data if minibatch_size is None else int(minibatch_size)   # :42-43
        self._rng = np.random.RandomState(0)                         # :46-47 (same seed for X and Y)
        self.Zf, self.Zg = Param(np.array(Zf, dtype=np.float64)), Param(np.array(Zg, dtype=np.float64))   # :50-51
        self.num_inducing_f, self.num_inducing_g = self.Zf.value.shape[0], self.Zg.value.shape[0]
        self.u_fm = Param(np.random.randn(self.num_inducing_f, self.num_latent) * 0.01)   # :56 (unseeded, as the reference)
        self.u_gm = Param(np.random.randn(self.num_inducing_g, self.num_latent) * 0.01)   # :57
        if self.q_diag:
            self.u_fs_sqrt = Param(np.ones((self.num_inducing_f, self.num_latent)), positive)  # :60-61
            self.u_gs_sqrt = Param(np.ones((self.num_inducing_g, self.num_latent)), positive)  # :62-63
        else:                                                                                  # :65-71 (num_latent = 1: one identity each)
            self.u_fs_sqrt = Param(np.eye(self.num_inducing_f)[:, :, None], LowerTriangular(self.num_inducing_f))
            self.u_gs_sqrt = Param(np.eye(self.num_inducing_g)[:, :, None], LowerTriangular(self.num_inducing_g))
        self._device = int(device)
        self._engine = zigp.reference_engine(self._device)  # raises if libzigp.so / GPU is missing: no CPU fallback; tf.cholesky's pivot rule
        self._resident = False

    # ---- parameter plumbing -----------------------------------------------------------------
    def _pset(self):
        return ParamSet(OrderedDict([
            ('Zf', self.Zf), ('Zg', self.Zg), ('u_fm', self.u_fm), ('u_gm', self.u_gm),
            ('u_fs_sqrt', self.u_fs_sqrt), ('u_gs_sqrt', self.u_gs_sqrt),
            ('ell_f', self.kernf.lengthscales), ('ell_g', self.kerng.lengthscales),
            ('var_f', self.kernf.variance), ('var_g', self.kerng.variance), ('noise', self.likelihood.variance)]
            + list(self.mean_function.trainables().items())))

    def _values(self):
        a, b = self.mean_function.linear_form(self.Xtrain.value.shape[1])
        mf = {k: v for k, v in (('mean_a', a), ('mean_b', b)) if v is not None}
        if self.whiten:
            mf['whiten'] = True          # the engine sets its mode from this on every call
        if not self.q_diag:
            mf['q_diag'] = False         # likewise (full-covariance q(u): u_*s_sqrt are (M, M, 1))
        for tag, kern in (('kern_f', self.kernf), ('kern_g', self.kerng)):
            if getattr(kern, 'kind', 'rbf') != 'rbf':
                mf[tag] = kern.kind      # likewise (Matern32 / Matern52; a kernel pickled before the kinds existed is an RBF)
        return dict(mf, Zf=self.Zf.value, Zg=self.Zg.value, u_fm=self.u_fm.value, u_gm=self.u_gm.value,
                    u_fs_sqrt=self.u_fs_sqrt.value, u_gs_sqrt=self.u_gs_sqrt.value,
                    ell_f=self.kernf.ell_vector(), ell_g=self.kerng.ell_vector(),
                    var_f=float(self.kernf.variance.value.reshape(-1)[0]), var_g=float(self.kerng.variance.value.reshape(-1)[0]),
                    noise=float(self.likelihood.variance.value.reshape(-1)[0]))

    def _fold_grads(self, g):
        """ARD engine gradient -> the shape of the Param (a scalar lengthscale sums its D copies)."""
        out = dict(g)
        for k, kern in (('ell_f', self.kernf), ('ell_g', self.kerng)):
            if kern.lengthscales.value.size == 1:
                out[k] = np.array([np.sum(g[k])])
        for k in ('var_f', 'var_g', 'noise'):
            out[k] = np.array([g[k]])
        if not self.q_diag:              # (M, M) from the engine -> the Param's (M, M, 1)
            for k in ('u_fs_sqrt', 'u_gs_sqrt'):
                out[k] = np.asarray(g[k])[:, :, None]
        if 'mean_b' in g:
            out['mean_b'] = np.array([g['mean_b']])
        return out

    def _sample_rows(self):
        """One step's row sample from self._rng (MinibatchData, :46-47), or None for the full batch."""
        if self.minibatch_size >= self.num_data:
            return None
        # GPflow 0.4 MinibatchData picks its index manager by the batch fraction [GPflow-recall; not in the reference tree, unverified]:
        # up to one half sampling WITH replacement (rng.randint), ABOVE one half a fresh permutation's head (without replacement) -- the
        # boundary case of exactly one half goes with randint, as the `fraction > 0.5` test of that recollection says
        if 2 * self.minibatch_size <= self.num_data:
            return self._rng.randint(self.num_data, size=self.minibatch_size)
        return self._rng.permutation(self.num_data)[:self.minibatch_size]

    def _make_resident(self):
        if not self._resident:
            self._engine.set_data(self.Xtrain.value, self.Ytrain.value)
            self._resident = True

    def _load_batch(self):
        """X and Y go to HBM once; a minibatch (MinibatchData, :46-47) is a row-index sample gathered on the device per step."""
        self._make_resident()
        idx = self._sample_rows()
        if idx is None:
            self._engine.select_rows(None)       # back to the full resident set (a minibatch_size raised after a minibatch step must not leave its last sample active)
            return 1.0
        self._engine.select_rows(idx)
        return float(self.num_data) / float(self.minibatch_size)          # :119-120

    def _matern_kernel(self):
        """'kernf is a Matern52 kernel' for the first Matern latent, None when both are RBF"""
        for tag, kern in (('kernf', self.kernf), ('kerng', self.kerng)):
            if getattr(kern, 'kind', 'rbf') != 'rbf':
                return '%s is a %s kernel' % (tag, type(kern).__name__)
        return None

    def _device_fit_eligible(self, pset):
        """the Adam loop can run on the device (zigp_fit_steps): unwhitened, diagonal q(u), Zero mean function, RBF kernels, every transform
        Identity or Log1pe(1e-6), at most DEVICE_FIT_MAX_D input columns"""
        return self._matern_kernel() is None and self.Xtrain.value.shape[1] <= DEVICE_FIT_MAX_D and not self.whiten and self.q_diag and type(self.mean_function) is Zero and all(
            type(q.transform) is Identity or (isinstance(q.transform, Log1pe) and q.transform._lower == 1e-6) for q in pset.params.values())

    def _adam_on_device(self, pset, maxiter):
        """maxiter Adam iterations in calls of at most DEVICE_FIT_CALL: the row samples are drawn from self._rng in the order and by the
        rule of _load_batch (the run sees the minibatches the host loop would), uploaded once per call and gathered on the device.
        A whitened model (diagonal or full-covariance q(u)) goes through WhiteDeviceFit (zigp_fit_steps_mode)."""
        self._make_resident()
        self._engine.select_rows(None)
        fit = (WhiteDeviceFit if self.whiten else DenseDeviceFit)(self._engine, pset)
        done = 0
        while done < maxiter:
            n = min(DEVICE_FIT_CALL, maxiter - done)
            if self.minibatch_size >= self.num_data:
                fit.steps(None, 0, JITTER, 1.0, n_steps=n)
            else:
                rows = np.stack([self._sample_rows() for _ in range(n)])
                fit.steps(rows, self.minibatch_size, JITTER, float(self.num_data) / float(self.minibatch_size))
            done += n

    def _elbo(self, need_grad):
        scale = self._load_batch()
        ed, kl, g = self._engine.elbo(self._values(), jitter=JITTER, scale=scale, need_grad=need_grad)
        return ed - kl, (self._fold_grads(g) if need_grad else None)

    # ---- reference surface ------------------------------------------------------------------
    def compute_log_likelihood(self):
        """build_likelihood value (OnOffSVGP.py:107-122)."""
        return self._elbo(False)[0]

    def compute_prior_KL(self):
        """build_prior_KL (OnOffSVGP.py:73-105,164-166)."""
        return float(np.sum(self._engine.prior_kl(self._values(), jitter=JITTER)))

    def predict_onoffgp(self, Xnew):
        """build_predict (OnOffSVGP.py:124-152,160-162): 9 arrays of shape (N,1), order of :152."""
        out = self._engine.predict(self._values(), np.asarray(Xnew, dtype=np.float64), jitter=JITTER)
        return tuple(out[i].reshape(-1, 1) for i in range(9))

    def predict_y(self, Xnew):
        """GPflow's predict_y: mean and variance of y at Xnew, each (N,1) -- ymean = gfmean, yvar = (gfvar + gfmeanu) + noise, from the
        rows of build_predict (the reference's likelihood leaves conditional moments out, OnOffLikelihood.py:28)."""
        out = self._engine.predict(self._values(), np.asarray(Xnew, dtype=np.float64), jitter=JITTER)
        noise = float(self.likelihood.variance.value.reshape(-1)[0])
        return out[0].reshape(-1, 1), ((out[1] + out[2]) + noise).reshape(-1, 1)

    def predict_density(self, Xnew, Ynew, n_quad=64, centre='mean'):
        """GPflow's predict_density: log p(Ynew | Xnew) per row, (N,1) -- f integrated in closed form, g by Gauss-Hermite quadrature with
        n_quad nodes on the device (zigp_predict_density).  centre='mean' centres the rule on gm: a row whose mass lies in the far tail
        of q(g), or in a spike between two nodes, is beyond it; centre='mode' shifts and scales the rule to each row's mode
        (zigp_predict_density_centred)."""
        kw = {} if centre == 'mean' else {'centre': centre}
        out, _ = self._engine.predict_density(self._values(), np.asarray(Xnew, dtype=np.float64), np.asarray(Ynew, dtype=np.float64),
                                              jitter=JITTER, n_quad=n_quad, **kw)
        return out[0].reshape(-1, 1)

    # Scores of the predictive distribution of y: the finite Gaussian mixture over the Gauss-Hermite rule centred on gm that predict_density
    # (centre='mean') defines (zigp_predict_scores).  The fixed rule only: a rule that moves with y is not one
    # distribution per row.
    def predict_cdf(self, Xnew, Ynew, n_quad=64):
        """(F, SF), each (N,1): P(y <= Ynew) and P(y > Ynew) per row, each its own sum (the small tail keeps its relative accuracy)"""
        r = self._engine.predict_scores(self._values(), np.asarray(Xnew, dtype=np.float64), np.asarray(Ynew, dtype=np.float64), jitter=JITTER,
                                        n_quad=n_quad, crps=False)
        return r['cdf'].reshape(-1, 1), r['sf'].reshape(-1, 1)

    def predict_quantiles(self, Xnew, levels, n_quad=64):
        """(N, L): the quantiles of y at the L levels (each strictly inside (0, 1); at most 16 per call), in the caller's order"""
        r = self._engine.predict_scores(self._values(), np.asarray(Xnew, dtype=np.float64), None, jitter=JITTER, n_quad=n_quad, levels=levels)
        if r['quantiles'] is None:
            return np.zeros((np.asarray(Xnew).shape[0], 0))
        return np.ascontiguousarray(r['quantiles'].T)

    def predict_crps(self, Xnew, Ynew, n_quad=64):
        """(N,1): the continuous ranked probability score of Ynew under the predictive distribution, per row (closed form of the mixture)"""
        r = self._engine.predict_scores(self._values(), np.asarray(Xnew, dtype=np.float64), np.asarray(Ynew, dtype=np.float64), jitter=JITTER,
                                        n_quad=n_quad, cdf=False)
        return r['crps'].reshape(-1, 1)

    def predict_onoffgp_samples(self, Xnew, num_samples, n_features=1024, seed=None):
        """GPflow's predict_f_samples for the three latent quantities: joint posterior sample paths (f, g, gf = Phi~(g) f) at Xnew, each
        (num_samples, N, 1), by pathwise conditioning with n_features random features per latent (zigp_sample_paths; DESIGN.md section
        10c): nothing of size N x N is formed.  The same seed gives the same arrays; at most 256 samples per call, D <= 8."""
        r = self._engine.sample_paths(self._values(), np.asarray(Xnew, dtype=np.float64), n_samples=int(num_samples), n_features=int(n_features),
                                      rng=np.random.RandomState(seed), jitter=JITTER)
        return tuple(np.ascontiguousarray(r[k])[:, :, None] for k in ('f', 'g', 'gf'))

    def predict_path_scores(self, Xnew, Ynew, groups=None, num_samples=16, member='gf', noise_eps=None, weights=None, energy=True, totals=True,
                            variogram=None, fair=False, n_features=1024, seed=None):
        """Scores of joint posterior sample paths at Xnew against Ynew per group of rows (zigp_ensemble_scores_device; DESIGN.md section
        10f): dict of NumPy arrays -- 'total' (num_samples, G) and 'total_obs' (G), the weighted group sums of every path and of Ynew;
        'crps_total', the ensemble CRPS of the totals; 'energy', the energy score over the group's rows; 'variogram' (p = 0.5, 1 or 2), the
        variogram score; 'offsets', 'labels'.  groups: None, G + 1 boundaries or N integer labels (a basin or week index).  The paths are
        drawn and scored on the device; only the scores come back.  The members are the NOISE-FREE paths `member` ('f', 'g' or 'gf')
        unless noise_eps, (num_samples, N) standard normals of the caller, is given: then gf + sqrt(noise variance) noise_eps."""
        import torch
        eng = self._engine
        dev = torch.device('cuda', eng.device)
        up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
        r = eng.path_scores_device(self._values(), up(Xnew), up(np.asarray(Ynew, dtype=np.float64).reshape(-1)), groups=groups,
                                   n_samples=int(num_samples), member=member, noise_eps=up(noise_eps), weights=up(weights), energy=energy,
                                   totals=totals, variogram=variogram, fair=fair, n_features=int(n_features), rng=np.random.RandomState(seed),
                                   jitter=JITTER)
        return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in r.items() if k != 'draws'}

    def optimize(self, method='L-BFGS-B', maxiter=1000, disp=False, callback=None, learning_rate=0.01, device_loop=None, **kw):
        """GPflow Model.optimize: scipy L-BFGS-B on the free state (default), or Adam when method='adam'
        (the commented alternative at zero-inflated-gpflow.ipynb:155).  Adam without a callback runs its loop on the device
        (zigp_fit_steps, DEVICE_FIT_CALL iterations per call) when the mean function is Zero, whiten is off and q_diag is on; otherwise, or with a callback, every
        iteration is a host step (select_rows + elbo + AdamGroups) -- the same minibatches and, to rounding, the same trajectory.
        device_loop (method='adam' only): None is that rule; True runs the loop on the device for the whitened models as well (whiten=True,
        with q_diag True or False: zigp_fit_steps_mode) and raises ValueError where it cannot -- a callback, a mean function other than
        Zero, an unsupported transform; False forces the host loop."""
        pset = self._pset()

        def vg(_values):
            return self._elbo(True)

        if str(method).lower() in ('l-bfgs-b', 'lbfgsb'):
            return lbfgsb(pset, vg, maxiter=maxiter, disp=disp, callback=callback, **kw)
        if str(method).lower() == 'adam':
            for p in pset.params.values():
                p.learning_rate = learning_rate
            if device_loop:
                if callback is not None:
                    raise ValueError('device_loop=True: a callback wants the host every step (device_loop=False, or no callback)')
                if type(self.mean_function) is not Zero:
                    raise ValueError('device_loop=True: the device loop fits the Zero mean function only (mean-function parameters stay with the host loop)')
                if self._matern_kernel() is not None:
                    raise ValueError('device_loop=True: %s and the device loop fits RBF latents only; device_loop=False or None runs the '
                                     'host loop' % self._matern_kernel())
                if self.Xtrain.value.shape[1] > DEVICE_FIT_MAX_D:
                    raise ValueError('device_loop=True: the device loop covers D <= %d input columns (D = %d); device_loop=False or None '
                                     'runs the host loop' % (DEVICE_FIT_MAX_D, self.Xtrain.value.shape[1]))
                self._adam_on_device(pset, maxiter)      # DenseDeviceFit / WhiteDeviceFit raise ValueError for a transform they do not implement
                return None
            if device_loop is None and callback is None and self._device_fit_eligible(pset):      # the whole loop on the device; a callback wants the host every step
                self._adam_on_device(pset, maxiter)
                return None
            opt = AdamGroups(pset)
            for it in range(maxiter):
                elbo, g = self._elbo(True)
                opt.step(g)
                if callback is not None:
                    callback(it, elbo)
            return None
        raise ValueError('unknown method %r' % (method,))

    def savemodel(self, fname=None):
        """pickle.dump of the model (OnOffSVGP.py:154-158); the engine handle is dropped and re-made on load."""
        if fname is None:
            fname = 'pm_' + time.strftime('%Y%m%d-%H%M') + '_' + str(self.name) + '.pickle'
        with open(fname, 'wb') as f:
            pickle.dump(self, f)
        return fname

    def __getstate__(self):
        d = dict(self.__dict__)
        d['_engine'] = None
        d['_resident'] = False
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.__dict__.setdefault('mean_function', Zero())
        self.__dict__.setdefault('whiten', False)
        self.__dict__.setdefault('q_diag', True)
        self.__dict__['_engine'] = zigp.reference_engine(self.__dict__.setdefault('_device', 0))   # the device it was fitted on

    @staticmethod
    def ProbitExpectations(gmean, gvar):
        """Host (NumPy) evaluation of OnOffSVGP.py:168-204 for inspection; the engine fuses the same formulas."""
        from scipy.special import erf
        z = gmean / np.sqrt(1. + gvar)
        a = 1 / np.sqrt(1. + (2 * gvar))
        cdfz = 0.5 * (1.0 + erf(z / np.sqrt(2.0))) * (1. - 2.e-3) + 1.e-3
        tz = np.arctan(a) / (2 * np.pi) * np.exp(-0.5 * np.square(z) * (np.square(a) + 1))
        pgmeansq = cdfz - 2. * tz
        pgvar = cdfz - 2. * tz - np.square(cdfz)
        return cdfz, (pgmeansq + np.abs(pgmeansq)) / 2., (pgvar + np.abs(pgvar)) / 2.
