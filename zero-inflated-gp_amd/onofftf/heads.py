"""Single-latent Kronecker SVGP models shared by the reference's baselines: the parameter set that scripts/svgp.py:51-112,
scripts/hurdle.py:64-124 and scripts/classifier.py:56-112 declare (TF scopes f_kern/, likelihood/, f_ind/), the Adam fit loop
of svgp.py:240-330 and the restore-and-predict step of onofftf/svgppred.py / onofftf/svcppred.py -- on libzigp's
zigp_kron_head_fit_steps / zigp_kron_head_elbo / zigp_kron_head_predict (include/zigp.h).  The fit loop runs on the device
(`HeadDeviceFit`, one host synchronisation per 100 iterations); `fit_head(..., device_loop=False)` steps it from the host with
zigp.optim.AdamGroups, one call per iteration (the checker of the device loop)."""
import logging
import os
import time
from collections import OrderedDict

import numpy as np

import zigp
from zigp.optim import AdamGroups, ParamSet
from zigp.transforms import Log1pe, positive
from .main import DataSet, Param
from .model import fused_matern_scope, get_kernels, has_matern, load_checkpoint, save_checkpoint, set_kernels

TRAIN_JITTER = 1e-5     # scripts/svgp.py:18, classifier.py:19, hurdle.py:18
PREDICT_JITTER = 1e-6   # onofftf/svgppred.py:13, onofftf/svcppred.py:13


def init_head_params(Xtrain, num_inducing_f, lik, init_ell=(5., 5.), u_scale=0.01, init_noisevar=0.01, include_f_mu=False,
                     kern_lr=1e-3, indp_lr=1e-3, rng=None, kmeans_seed=None, kmeans='scipy', engine=None):
    """svgp.py:51-112 (ell [5,5],[5/1000]; var 20; noise 0.01; u 0.01*randn; s 1); the predictors rebuild the same set with
    ell [8,8], u 0.1*randn, noise 0.001 before restoring (svgppred.py:21-37) -- those values are overwritten by the restore.
    kmeans: 'scipy' (the reference's host call, svgp.py:64) or 'device' (onofftf.model.device_kmeans, on `engine`)."""
    if kmeans not in ('scipy', 'device'):
        raise ValueError("kmeans must be 'scipy' or 'device', not %r" % (kmeans,))
    if kmeans == 'device':
        from .model import device_kmeans

        def kmeans(X2, M, seed=None):
            return (device_kmeans(Xtrain, M, seed, engine),)
    else:
        from scipy.cluster.vq import kmeans
    rng = rng or np.random
    M0, M1 = int(num_inducing_f[0]), int(num_inducing_f[1])
    Zs = kmeans(Xtrain[:, 0:2], M0, seed=kmeans_seed)[0]                          # svgp.py:64
    if Zs.shape[0] < M0:                                                          # kmeans may return fewer centroids
        Zs = np.vstack([Zs, Xtrain[rng.choice(Xtrain.shape[0], M0 - Zs.shape[0], replace=False), 0:2] + 1e-3])
    Zt = np.linspace(Xtrain[:, 2].min(), Xtrain[:, 2].max(), M1)[:, None]        # :65
    ells = [np.array(init_ell, dtype=np.float64), np.array([5. / 1000])]          # :58
    p = OrderedDict()
    for i in range(2):
        p['f_kern/lengthscale_%d' % i] = Param(ells[i], Log1pe(), name='lengthscale', learning_rate=kern_lr)
        p['f_kern/variance_%d' % i] = Param([20.], Log1pe(), name='variance', learning_rate=kern_lr)      # :59
    if lik == 'gaussian':
        p['likelihood/variance'] = Param(init_noisevar, Log1pe(), name='variance', learning_rate=kern_lr)  # :93-95
    if include_f_mu:
        p['f_mu'] = Param(0., name='fmu', learning_rate=indp_lr)                                           # classifier.py:70-72
    p['f_ind/z_0'] = Param(Zs.copy(), name='z', learning_rate=indp_lr)
    p['f_ind/z_1'] = Param(Zt.copy(), name='z', learning_rate=indp_lr)
    p['f_ind/value'] = Param(rng.randn(M0 * M1, 1) * u_scale, name='value', learning_rate=indp_lr)         # :68
    p['f_ind/variance'] = Param(np.ones((M0 * M1, 1)), positive, name='variance', learning_rate=indp_lr)   # :69,104-106
    return ParamSet(p)


def head_engine_params(pset):
    v = {k: q.value for k, q in pset.params.items()}
    out = dict(Zf=[v['f_ind/z_0'], v['f_ind/z_1']], ell_f=[v['f_kern/lengthscale_0'], v['f_kern/lengthscale_1']],
               var_f=[v['f_kern/variance_0'], v['f_kern/variance_1']], u_fm=v['f_ind/value'], u_fs_sqrt=v['f_ind/variance'])
    if 'likelihood/variance' in v:
        out['noise'] = v['likelihood/variance']
    out['kern_f'] = get_kernels(pset, ('f',))['f']
    return out


def head_f_mu(pset):
    return float(pset.params['f_mu'].value.reshape(-1)[0]) if 'f_mu' in pset.params else 0.0


def named_head_grads(g):
    out = {'likelihood/variance': np.array([g['noise']]), 'f_mu': np.array([g['f_mu']]),
           'f_ind/value': np.asarray(g['u_fm']), 'f_ind/variance': np.asarray(g['u_fs_sqrt'])}
    for i in range(2):
        out['f_kern/lengthscale_%d' % i] = np.asarray(g['ell_f'][i])
        out['f_kern/variance_%d' % i] = np.array([g['var_f'][i]])
        out['f_ind/z_%d' % i] = np.asarray(g['Zf'][i])
    return out


# block order of zigp_kron_head_fit_steps' free-state vector (include/zigp.h): Z0, Z1, u, s, ell0, ell1, var0, var1, noise, f_mu
HEAD_FIT_BLOCK_NAMES = ('f_ind/z_0', 'f_ind/z_1', 'f_ind/value', 'f_ind/variance', 'f_kern/lengthscale_0', 'f_kern/lengthscale_1',
                        'f_kern/variance_0', 'f_kern/variance_1', 'likelihood/variance', 'f_mu')
LOG_EVERY = 100         # fit_head's log cadence (the reference's heads print every 100 iterations, svgp.py:300)


class HeadDeviceFit:
    """The Adam state of a single-latent head fit in the layout of zigp_kron_head_fit_steps, for a ParamSet made by init_head_params --
    the single-latent twin of onofftf.model.KronDeviceFit: the flat free state x and the moments m, v live here between calls (the
    engine updates them in place), `steps` advances them on the device and writes the constrained values back into the ParamSet.
    A fixed parameter is a block with trainable = 0: the device leaves its x, m, v alone and its .value is never written back.  All ten
    blocks are always there: a ParamSet without `f_mu` (include_f_mu=False) gets an untrainable block with free value 0, one without
    `likelihood/variance` (the classifier) an untrainable noise of 1 that the Bernoulli head never reads.  zigp.optim.AdamGroups on the
    same ParamSet is the host-side checker."""

    def __init__(self, engine, pset, lik, beta1=0.9, beta2=0.999, eps=1e-8):
        if lik not in ('gaussian', 'bernoulli'):
            raise ValueError("lik must be 'gaussian' or 'bernoulli', not %r" % (lik,))
        self.engine, self.pset, self.lik = engine, pset, lik
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        missing = [k for k in HEAD_FIT_BLOCK_NAMES[:8] if k not in pset.params]
        extra = [k for k in pset.params if k not in HEAD_FIT_BLOCK_NAMES]
        if missing or extra:
            raise ValueError('the head device fit loop trains the parameters of init_head_params (missing: %s; unknown: %s)'
                             % (', '.join(missing) or '-', ', '.join(extra) or '-'))
        if lik == 'gaussian' and 'likelihood/variance' not in pset.params:
            raise ValueError("the Gaussian head needs the parameter 'likelihood/variance'")
        for k, q in self._present():
            if not isinstance(q.transform, Log1pe) and type(q.transform).__name__ != 'Identity':
                raise ValueError('unsupported transform %r of %s' % (q.transform, k))
            if isinstance(q.transform, Log1pe) and q.transform._lower != 1e-6:
                raise ValueError('the device fit loop implements Log1pe with lower = 1e-6')
        v = pset.params
        Z0, Z1 = v['f_ind/z_0'].value, v['f_ind/z_1'].value
        self.shape = dict(M0f=Z0.shape[0], M1f=Z1.shape[0], D0=Z0.shape[1], D1=Z1.shape[1],
                          kern_f=get_kernels(pset, ('f',))['f'])      # a Matern factor: kron_head_fit_steps refuses by name
        M = Z0.shape[0] * Z1.shape[0]
        want = [Z0.size, Z1.size, M, M, Z0.shape[1], Z1.shape[1], 1, 1, 1, 1]
        self.sizes = want
        for (k, q), n in zip(self._blocks(), want):
            if q is not None and q.value.size != n:
                raise ValueError('%s has %d entries, not %d' % (k, q.value.size, n))
        self.positive = [q is not None and isinstance(q.transform, Log1pe) for k, q in self._blocks()]
        self.m, self.v = np.zeros(sum(want)), np.zeros(sum(want))
        self.t = 0
        self.resync()

    def _blocks(self):
        return [(k, self.pset.params.get(k)) for k in HEAD_FIT_BLOCK_NAMES]

    def _present(self):
        return [(k, q) for k, q in self._blocks() if q is not None]

    def _slices(self):
        o = 0
        for (k, q), n in zip(self._blocks(), self.sizes):
            yield k, q, slice(o, o + n)
            o += n

    def steps(self, row_begin, batch, jitter, scale, Xw=None, Yw=None, include_kl=True):
        """len(row_begin) iterations on the resident data set (engine.set_data): returns (elbo_data, kl) per step; the ParamSet holds the
        constrained values after the last one.  If the engine raises in step k (a Cholesky failure), x / m / v are the state after the k
        updates that WERE applied, self.t has advanced by k, and the exception carries `steps_applied`, `elbo_data`, `kl` of those steps.
        The ParamSet is read again when something other than this object changed it since the last call (load_checkpoint, an assignment
        to .value, a parameter fixed or un-fixed, a new learning rate): see resync()."""
        if self._stale():
            self.resync()
        try:
            out = self.engine.kron_head_fit_steps(self.shape, self.lik, self.x, self.m, self.v, self.lr, self.positive, self.trainable, self.t,
                                                  row_begin, batch, jitter=jitter, scale=scale, Xw=Xw, Yw=Yw, beta1=self.beta1, beta2=self.beta2,
                                                  eps=self.eps, include_kl=include_kl)
            self.t += len(row_begin)
        except Exception as e:
            self.t += int(getattr(e, 'steps_applied', 0))
            raise
        finally:
            self.sync_params()
        return out

    def _stale(self):
        """did anyone else write the ParamSet since sync_params?  equal_nan: a parameter that HAS gone NaN is still the value this object
        wrote (NaN != NaN must not turn every later call into a resync from free(NaN))"""
        return (any(not np.array_equal(q.value, w, equal_nan=True) for (k, q), w in zip(self._present(), self._written))
                or [q is not None and not q.fixed for k, q in self._blocks()] != self.trainable
                or [float(q.learning_rate) if q is not None else 0.0 for k, q in self._blocks()] != self.lr)

    def resync(self, reset=False):
        """Take the free state, the fixed flags and the learning rates from the ParamSet again (after load_checkpoint or a manual
        assignment).  Adam's moments and the iteration count are kept unless reset=True (parameters unrelated to the ones trained so
        far: load_checkpoint(..., fitter=...) of another run)."""
        # an absent block: f_mu = 0 (classifier.py:136-137 adds nothing); a noise of 1 for the head that has none (never read)
        self.x = np.concatenate([q.free() if q is not None else np.array([1.0 if k == 'likelihood/variance' else 0.0]) for k, q in self._blocks()])
        self.trainable = [q is not None and not q.fixed for k, q in self._blocks()]
        self.lr = [float(q.learning_rate) if q is not None else 0.0 for k, q in self._blocks()]
        if reset:
            self.m[:] = 0.0
            self.v[:] = 0.0
            self.t = 0
        self._written = [q.value.copy() for k, q in self._present()]

    def sync_params(self):
        for (k, q, sl), tr in zip(self._slices(), self.trainable):
            if tr:
                q.set_free(self.x[sl])
        self._written = [q.value.copy() for k, q in self._present()]


def head_device_loop_covers(num_inducing_f, D0=2, D1=1):
    """the grids of the fused Kronecker kernels (<= 32 x <= 32 or <= 16 x <= 112 points, <= 7 columns per factor): what
    zigp_kron_head_fit_steps accepts"""
    m0, m1 = int(num_inducing_f[0]), int(num_inducing_f[1])
    return ((m0 <= 32 and m1 <= 32) or (m0 <= 16 and m1 <= 112)) and D0 <= 7 and D1 <= 7


def _device_loop(eng, pset, lik, train_data, num_iter, num_minibatch, scale, save_every, ckpt, logger, history):
    """svgp.py:289-330 / classifier.py:276-316 with the loop body on the device (zigp_kron_head_fit_steps), run as
    onofftf/onoff.py:_device_loop runs the on/off fit: the iterations between two log lines are ONE call.  The batch sequence is
    DataSet's (onofftf/main.py:98-133): the permuted epoch is resident, a call ends at the one wrap-around batch of an epoch (its rows
    go down with the call), at a checkpoint iteration, or after LOG_EVERY steps."""
    fitter = HeadDeviceFit(eng, pset, lik)
    resident, i = None, 0
    while i < num_iter:
        n_target = min(num_iter - i, LOG_EVERY - (i % LOG_EVERY))
        if ckpt and save_every:
            n_target = min(n_target, save_every - (i % save_every) if i % save_every else 1)       # a checkpoint iteration ends its call
        t0 = time.time()
        rbs, wrap = [], None
        while len(rbs) < n_target:
            gen, lo, hi, wrap = train_data.next_span(num_minibatch)
            if wrap is not None:
                rbs.append(-1)
                break
            if gen != resident:              # only ever at the start of a call: a generation changes right after a wrap-around batch
                eng.set_data(train_data.xtrain, train_data.ytrain)
                resident = gen
            rbs.append(lo)
        ed, kl = fitter.steps(rbs, num_minibatch, TRAIN_JITTER, scale, *(wrap if wrap is not None else (None, None)))
        if history is not None:
            history.extend((-(ed - kl)).tolist())
        per_it = (time.time() - t0) / len(rbs)
        for j in range(i, i + len(rbs)):
            if j % LOG_EVERY == 0:
                logger.info('{:>16d}'.format(j) + '{:>6.3f}'.format(per_it / 60))
            if ckpt and save_every and j % save_every == 0:
                save_checkpoint(pset, ckpt)
        i += len(rbs)


def fit_head(pset, lik, Xtrain, Ytrain, num_iter, num_minibatch, logger, ckpt=None, eng=None, save_every=10000, history=None,
             device_loop=True, kernels=None, fused_matern=False):
    """fit_head's loop (_fit_head) under the fused Matern option: fused_matern=True runs Matern factors on the fused kernels for this
    call (DenseEngine.set_kron_matern_fused; the engine's setting comes back afterwards), so that a Matern head takes the device_loop
    branch an RBF head takes.  Not kept in the checkpoint."""
    with fused_matern_scope(eng, fused_matern):
        return _fit_head(pset, lik, Xtrain, Ytrain, num_iter, num_minibatch, logger, ckpt, eng, save_every, history, device_loop, kernels,
                         fused_matern)


def _fit_head(pset, lik, Xtrain, Ytrain, num_iter, num_minibatch, logger, ckpt, eng, save_every, history, device_loop, kernels, fused_matern):
    """The optimisation loop of svgp.py:289-330 / classifier.py:276-316: Adam per learning-rate group on
    cost = -(sum(var_exp) * num_data / num_minibatch - kl).  device_loop: run it on the device (_device_loop) where the inducing grid
    is within the fused kernels; False, or a larger grid, steps it from the host, one engine call per iteration.
    kernels: the factor kinds of f -- a name or a pair (space, time) of 'rbf', 'matern32', 'matern52' (None: what the parameter set
    holds, RBF by default).  With a Matern factor the host loop runs also when device_loop=True (the device loop fits RBF factors),
    unless fused_matern."""
    if kernels is not None:
        set_kernels(pset, kernels, ('f',))
    if device_loop and num_iter > 0 and has_matern(pset, ('f',)) and not fused_matern:
        logger.info('Matern factor kernel %s: the host Adam loop runs (the device loop fits RBF factors only)' % (get_kernels(pset, ('f',))['f'],))
        device_loop = False
    train_data = DataSet(Xtrain, Ytrain)                                          # svgp.py:43
    scale = float(Xtrain.shape[0]) / float(num_minibatch)                         # :212
    logger.info('*******  started optimization at ' + time.strftime('%Y%m%d-%H%M') + ' *******')
    logger.info('{:>16s}'.format('iteration') + '{:>6s}'.format('time'))
    Z0, Z1 = pset.params['f_ind/z_0'].value, pset.params['f_ind/z_1'].value
    if (device_loop and num_iter > 0 and head_device_loop_covers((Z0.shape[0], Z1.shape[0]), Z0.shape[1], Z1.shape[1])
            and num_minibatch <= Xtrain.shape[0]):
        try:
            _device_loop(eng, pset, lik, train_data, num_iter, num_minibatch, scale, save_every, ckpt, logger, history)
        except KeyboardInterrupt:
            print('Stopping training')
        num_iter = 0
    opt = AdamGroups(pset) if num_iter else None                                  # :225-252
    for i in range(num_iter):
        t0 = time.time()
        xb, yb = train_data.next_batch(num_minibatch)
        try:
            ed, kl, g = eng.kron_head_elbo(head_engine_params(pset), xb, yb, lik, jitter=TRAIN_JITTER, scale=scale, f_mu=head_f_mu(pset))
            opt.step(named_head_grads(g))
            if history is not None:
                history.append(-(ed - kl))
            if i % 100 == 0:
                logger.info('{:>16d}'.format(i) + '{:>6.3f}'.format((time.time() - t0) / 60))
            if ckpt and save_every and i % save_every == 0:
                save_checkpoint(pset, ckpt)
        except KeyboardInterrupt:
            print('Stopping training')
            break
    if ckpt:
        save_checkpoint(pset, ckpt)
    return pset


def log_kernel_summary(logger, pset):
    v = {k: q.value for k, q in pset.params.items()}
    if 'likelihood/variance' in v:
        logger.info('Noise variance          = ' + str(v['likelihood/variance']))
    logger.info('Kf spatial lengthscale  = ' + str(v['f_kern/lengthscale_0']))
    logger.info('Kf spatial variance     = ' + str(v['f_kern/variance_0']))
    logger.info('Kf temporal lengthscale = ' + str(v['f_kern/lengthscale_1']))
    logger.info('Kf temporal variance    = ' + str(v['f_kern/variance_1']))


def open_logger(path):
    logger = logging.getLogger('log')
    logger.setLevel(logging.DEBUG)
    handler = logging.FileHandler(path) if path else logging.NullHandler()
    logger.addHandler(handler)
    return logger, handler


def close_logger(logger, handler):
    handler.close()
    logger.removeHandler(handler)


def _restore_head(lik, Xtrain, checkpointPath, num_inducing_f, include_f_mu, device, engine):
    """svgppred.py:15-203 / svcppred.py:15-224: rebuild the parameter set and restore it; (engine, engine parameters, f_mu)"""
    pset = init_head_params(Xtrain, num_inducing_f, lik, init_ell=(8., 8.), u_scale=0.1, init_noisevar=0.001,
                            include_f_mu=include_f_mu, kern_lr=1e-4, indp_lr=1e-4)
    ck = os.path.join(checkpointPath, 'model') if os.path.isdir(checkpointPath) else checkpointPath
    load_checkpoint(pset, ck)
    eng = engine or zigp.reference_engine(device)      # tf.cholesky's acceptance rule (pivot > 0)
    return eng, head_engine_params(pset), head_f_mu(pset)


def restore_and_predict(lik, Xtrain, Xtest, checkpointPath, num_inducing_f, include_f_mu, rows, device=0, engine=None, fused_matern=False):
    """Restore (_restore_head), then evaluate with jitter 1e-6.  fused_matern: Matern factors on the fused kernels for this call."""
    eng, p, f_mu = _restore_head(lik, Xtrain, checkpointPath, num_inducing_f, include_f_mu, device, engine)

    def run(X):
        o = eng.kron_head_predict(p, X, lik, jitter=PREDICT_JITTER, f_mu=f_mu)
        return {name: o[r].reshape(-1, 1) for name, r in rows}

    with fused_matern_scope(eng, fused_matern):
        pred_train = run(Xtrain)
        if Xtest is not None:
            return pred_train, run(Xtest)
        return pred_train


def restore_and_sample(lik, Xtrain, Xtest, checkpointPath, num_inducing_f, include_f_mu, num_samples, n_features=1024, seed=None, draws=None,
                       device=0, engine=None):
    """Restore (_restore_head), then joint sample paths of the head at Xtest (DenseEngine.kron_head_sample_paths, jitter 1e-6)."""
    eng, p, f_mu = _restore_head(lik, Xtrain, checkpointPath, num_inducing_f, include_f_mu, device, engine)
    return eng.kron_head_sample_paths(p, Xtest, lik, n_samples=int(num_samples), n_features=n_features, rng=seed, draws=draws,
                                      jitter=PREDICT_JITTER, f_mu=f_mu)
