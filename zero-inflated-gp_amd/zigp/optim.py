"""Optimiser loops around the ELBO step (host side).

* `ParamSet` maps named constrained parameters <-> one flat free-state vector (the role of GPflow's
  Parameterized.get_free_state / set_state and of onofftf.main.Param, onofftf/main.py:137-184).
* `lbfgsb` is GPflow 0.4.0 Model.optimize's default (scipy.optimize.minimize(method='L-BFGS-B', jac=True)).
* `AdamGroups` reproduces scripts/onoff.py:325-350: one tf.train.AdamOptimizer per distinct learning
  rate (TF defaults beta1=0.9, beta2=0.999, eps=1e-8; update lr_t = lr*sqrt(1-b2^t)/(1-b1^t)).
* `DenseDeviceFit` keeps the same Adam state in the layout of zigp_fit_steps and advances it on the device
  (the dense counterpart of onofftf.model.KronDeviceFit); `AdamGroups` is its host-side checker.  `WhiteDeviceFit` is the same for the
  whitened models, diagonal and full-covariance (zigp_fit_steps_mode).
"""
import numpy as np

from .transforms import Identity


class P:
    """One trainable (or fixed) parameter: constrained value + transform (+ learning rate for Adam groups)."""

    def __init__(self, value, transform=None, fixed=False, learning_rate=0.001, name=None):
        self.transform = transform or Identity()
        self.value = np.array(value, dtype=np.float64)
        self.fixed = fixed
        self.learning_rate = learning_rate
        self.name = name

    @property
    def shape(self):
        return self.value.shape

    def free(self):
        return np.asarray(self.transform.backward(self.value), dtype=np.float64).reshape(-1)

    def free_size(self):
        """entries of the free vector: the value's size unless the transform says otherwise (LowerTriangular: N(N+1)/2 for N x N)"""
        fs = getattr(self.transform, 'free_size', None)
        return int(fs()) if fs is not None else self.value.size

    def set_free(self, x):
        self.value = np.asarray(self.transform.forward(x), dtype=np.float64).reshape(self.value.shape)


class ParamSet:
    def __init__(self, params):
        """params: ordered dict name -> P"""
        self.params = params

    def names(self, trainable_only=True):
        return [k for k, p in self.params.items() if not (trainable_only and p.fixed)]

    def get_free(self):
        xs = [self.params[k].free() for k in self.names()]
        return np.concatenate(xs) if xs else np.zeros(0)

    def set_free(self, x):
        o = 0
        for k in self.names():
            p = self.params[k]
            n = p.free_size()
            p.set_free(np.asarray(x[o:o + n]))
            o += n

    def values(self):
        return {k: p.value for k, p in self.params.items()}

    def free_grad(self, grads):
        """Chain constrained gradients (dict name -> array) to the flat free-state gradient."""
        gs = []
        for k in self.names():
            p = self.params[k]
            x = p.free()
            gs.append(np.asarray(p.transform.grad_free(x, np.asarray(grads[k], dtype=np.float64).reshape(-1))).reshape(-1))
        return np.concatenate(gs) if gs else np.zeros(0)


def lbfgsb(pset, value_and_grad, maxiter=1000, disp=False, callback=None, ftol=2.220446049250313e-09, gtol=1e-5):
    """Minimise -ELBO.  value_and_grad(values dict) -> (elbo, grads dict w.r.t. constrained values)."""
    from scipy.optimize import minimize

    def obj(x):
        pset.set_free(x)
        elbo, g = value_and_grad(pset.values())
        return -elbo, -pset.free_grad(g)

    res = minimize(obj, pset.get_free(), method='L-BFGS-B', jac=True, callback=callback,
                   options=dict(maxiter=maxiter, disp=disp, ftol=ftol, gtol=gtol))
    pset.set_free(res.x)
    return res


class AdamGroups:
    """One Adam per learning rate on the FREE state (TensorFlow's variables are the unconstrained values: scripts/onoff.py:88-123 builds
    the positive parameters as transforms of them, and the optimisers of :325-350 update the variables).  The free vectors are kept
    across steps (initialised from the constrained values once); every step writes the constrained values back into the ParamSet."""

    def __init__(self, pset, beta1=0.9, beta2=0.999, eps=1e-8):
        self.pset = pset
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.t = 0
        self.m = {k: np.zeros(pset.params[k].free_size()) for k in pset.names()}
        self.v = {k: np.zeros(pset.params[k].free_size()) for k in pset.names()}
        self.resync()

    def resync(self, reset=False):
        """Take the free vectors from the ParamSet again.  step() does this by itself for any parameter whose constrained value is no
        longer the one it wrote (load_checkpoint, an assignment to .value): the cached free vector would silently overwrite such a change.
        The moments and the iteration count are kept unless reset=True (parameters unrelated to the ones trained so far)."""
        if reset:
            self.t = 0
            for k in self.m:
                self.m[k][:] = 0.0
                self.v[k][:] = 0.0
        self.x = {k: self.pset.params[k].free().copy() for k in self.pset.names()}
        self._written = {k: self.pset.params[k].value.copy() for k in self.pset.names()}

    def step(self, grads):
        """One minimisation step of cost = -ELBO given d ELBO / d (constrained)."""
        self.t += 1
        for k in self.pset.names():
            p = self.pset.params[k]
            if k not in self.m:                                    # un-fixed since construction: it joins with fresh moments
                self.m[k], self.v[k] = np.zeros(p.free_size()), np.zeros(p.free_size())
                self._written[k] = None
            if self._written[k] is None or not np.array_equal(p.value, self._written[k], equal_nan=True):   # changed behind our back: start from what the ParamSet holds now
                self.x[k] = p.free().copy()
            x = self.x[k]
            g = -np.asarray(p.transform.grad_free(x, np.asarray(grads[k], dtype=np.float64).reshape(-1))).reshape(-1)
            self.m[k] = self.b1 * self.m[k] + (1 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1 - self.b2) * g * g
            lr_t = p.learning_rate * np.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
            self.x[k] = x - lr_t * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
            p.set_free(self.x[k])
            self._written[k] = p.value.copy()


# block order of zigp_fit_steps' free-state vector (include/zigp.h): the order of OnOffSVGP._pset / zigp.engine.PARAM_KEYS
DENSE_FIT_KEYS = ('Zf', 'Zg', 'u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')


class DenseDeviceFit:
    """The Adam state of the dense on/off fit in the layout of zigp_fit_steps, for a ParamSet with the keys DENSE_FIT_KEYS (the one
    OnOffSVGP._pset builds for a Zero mean function): the flat free state x and the moments m, v live here between calls (the engine
    updates them in place), `steps` advances them on the device and writes the constrained values back into the ParamSet.
    A fixed parameter is a block with trainable = 0: the device leaves its x, m, v alone and its .value is never written back (on the
    device it is the transform of its free value: for a fixed Log1pe parameter that is forward(backward(value)), equal to the value to
    rounding).  A lengthscale Param with one entry is ONE lengthscale for all D columns (ell_size = 1).  AdamGroups on the same ParamSet
    is the host-side checker."""

    def __init__(self, engine, pset, beta1=0.9, beta2=0.999, eps=1e-8):
        from .transforms import Log1pe
        self.engine, self.pset = engine, pset
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        extra = [k for k in pset.params if k not in DENSE_FIT_KEYS]
        if extra or any(k not in pset.params for k in DENSE_FIT_KEYS):
            raise ValueError('the dense device fit loop trains exactly %s (got also / not: %s): mean-function parameters stay with the host loop'
                             % (', '.join(DENSE_FIT_KEYS), ', '.join(extra) or 'a key is missing'))
        ps = [pset.params[k] for k in DENSE_FIT_KEYS]
        for q in ps:
            if not isinstance(q.transform, Log1pe) and type(q.transform).__name__ != 'Identity':
                raise ValueError('unsupported transform %r' % (q.transform,))
            if isinstance(q.transform, Log1pe) and q.transform._lower != 1e-6:
                raise ValueError('the device fit loop implements Log1pe with lower = 1e-6')
        Zf, Zg = ps[0].value, ps[1].value
        if Zf.ndim != 2 or Zg.ndim != 2 or Zf.shape[1] != Zg.shape[1]:
            raise ValueError('Zf and Zg must be (M,D) with equal D')
        D = Zf.shape[1]
        self.shape = dict(Mf=Zf.shape[0], Mg=Zg.shape[0], D=D)
        self.sizes = [q.value.size for q in ps]
        want = [Zf.size, Zg.size, Zf.shape[0], Zg.shape[0], Zf.shape[0], Zg.shape[0], None, None, 1, 1, 1]
        for k, n, w in zip(DENSE_FIT_KEYS, self.sizes, want):
            if (w is None and n not in (1, D)) or (w is not None and n != w):
                raise ValueError('%s has %d entries' % (k, n))
        self.ell_size = (self.sizes[6], self.sizes[7])
        self.positive = [isinstance(q.transform, Log1pe) for q in ps]
        self.m, self.v = np.zeros(sum(self.sizes)), np.zeros(sum(self.sizes))
        self.t = 0
        self.resync()

    def _blocks(self):
        o = 0
        for k, n in zip(DENSE_FIT_KEYS, self.sizes):
            yield k, self.pset.params[k], slice(o, o + n)
            o += n

    def steps(self, rows, batch, jitter, scale, n_steps=None, include_kl=True):
        """Iterations on the resident data set (engine.set_data): rows = int64 [n_steps, batch] row indices, one row of it per step, or None
        for n_steps iterations over the active rows (full batch).  Returns (elbo_data, kl) per step; the ParamSet holds the constrained
        values after the last one.  If the engine raises in step k (a Cholesky failure), x / m / v are the state after the k updates that
        WERE applied, self.t has advanced by k, and the exception carries `steps_applied`, `elbo_data`, `kl` of those steps.  The ParamSet
        is read again when something other than this object changed it since the last call (an assignment to .value, a parameter fixed
        or un-fixed, a new learning rate): see resync()."""
        if rows is not None:
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64)).reshape(-1)
            if int(batch) <= 0 or rows.size % int(batch) or (n_steps is not None and rows.size != int(n_steps) * int(batch)):
                raise ValueError('rows must hold whole steps of `batch` indices')
            n_steps = rows.size // int(batch)
        elif n_steps is None:
            raise ValueError('full-batch steps (rows=None) need n_steps')
        if self._stale():
            self.resync()
        try:
            out = self._engine_call(n_steps, rows=rows, batch=batch, jitter=jitter, scale=scale, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                                    include_kl=include_kl)
            self.t += int(n_steps)
        except Exception as e:
            self.t += int(getattr(e, 'steps_applied', 0))
            raise
        finally:
            self.sync_params()
        return out

    def _engine_call(self, n_steps, **kw):
        return self.engine.fit_steps(self.shape, self.x, self.m, self.v, self.lr, self.positive, self.trainable, self.ell_size, self.t, n_steps, **kw)

    def _stale(self):
        """did anyone else write the ParamSet since sync_params?  equal_nan: a parameter that HAS gone NaN is still the value this object
        wrote (NaN != NaN must not turn every later call into a resync from free(NaN))"""
        return (any(not np.array_equal(q.value, w, equal_nan=True) for (k, q, sl), w in zip(self._blocks(), self._written))
                or [not q.fixed for k, q, sl in self._blocks()] != self.trainable
                or [float(q.learning_rate) for k, q, sl in self._blocks()] != self.lr)

    def resync(self, reset=False):
        """Take the free state, the fixed flags and the learning rates from the ParamSet again.  Adam's moments and the iteration count
        are kept unless reset=True (parameters unrelated to the ones trained so far)."""
        self.x = np.concatenate([q.free() for k, q, sl in self._blocks()])
        self.trainable = [not q.fixed for k, q, sl in self._blocks()]
        self.lr = [float(q.learning_rate) for k, q, sl in self._blocks()]
        if reset:
            self.m[:] = 0.0
            self.v[:] = 0.0
            self.t = 0
        self._written = [q.value.copy() for k, q, sl in self._blocks()]

    def sync_params(self):
        for (k, q, sl), tr in zip(self._blocks(), self.trainable):
            if tr:
                q.set_free(self.x[sl])
        self._written = [q.value.copy() for k, q, sl in self._blocks()]


class WhiteDeviceFit(DenseDeviceFit):
    """DenseDeviceFit for the whitened models (zigp_fit_steps_mode): a ParamSet with the keys DENSE_FIT_KEYS whose u_fs_sqrt / u_gs_sqrt are
    BOTH Log1pe(1e-6) vectors -- the whitened diagonal q(u), ZIGP_FIT_WHITE, the 11 blocks of DenseDeviceFit -- or BOTH
    transforms.LowerTriangular(M) matrices, values (M, M) or (M, M, 1) -- the full-covariance q(u), ZIGP_FIT_WHITE_FULL: their blocks of
    x / m / v are the M (M + 1) / 2 lower-triangle entries in row-major order, LowerTriangular's free vector, and sync_params writes the
    matrices back with an exactly zero strict upper triangle.  One latent full and the other diagonal is refused.  steps / resync /
    sync_params / the detection of outside changes are DenseDeviceFit's; AdamGroups on the same ParamSet is the host-side checker.
    The engine's own whiten / q_full settings are neither read nor changed."""

    def __init__(self, engine, pset, beta1=0.9, beta2=0.999, eps=1e-8):
        from . import _lib
        from .transforms import Log1pe, LowerTriangular
        self.engine, self.pset = engine, pset
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        extra = [k for k in pset.params if k not in DENSE_FIT_KEYS]
        if extra or any(k not in pset.params for k in DENSE_FIT_KEYS):
            raise ValueError('the dense device fit loop trains exactly %s (got also / not: %s): mean-function parameters stay with the host loop'
                             % (', '.join(DENSE_FIT_KEYS), ', '.join(extra) or 'a key is missing'))
        ps = [pset.params[k] for k in DENSE_FIT_KEYS]
        tri = [isinstance(ps[b].transform, LowerTriangular) for b in (4, 5)]
        if tri[0] != tri[1]:
            raise ValueError('u_fs_sqrt and u_gs_sqrt must both be LowerTriangular matrices (full-covariance q(u)) or both Log1pe vectors '
                             '(diagonal q(u)): got %r and %r' % (ps[4].transform, ps[5].transform))
        self.full = tri[0]
        self.mode = _lib.FIT_WHITE_FULL if self.full else _lib.FIT_WHITE
        for b, q in enumerate(ps):
            if self.full and b in (4, 5):
                continue
            if b in (4, 5) and not isinstance(q.transform, Log1pe):
                raise ValueError('%s: the diagonal q(u) of the whitened model is a Log1pe(1e-6) vector, not %r' % (DENSE_FIT_KEYS[b], q.transform))
            if not isinstance(q.transform, Log1pe) and type(q.transform).__name__ != 'Identity':
                raise ValueError('unsupported transform %r' % (q.transform,))
            if isinstance(q.transform, Log1pe) and q.transform._lower != 1e-6:
                raise ValueError('the device fit loop implements Log1pe with lower = 1e-6')
        Zf, Zg = ps[0].value, ps[1].value
        if Zf.ndim != 2 or Zg.ndim != 2 or Zf.shape[1] != Zg.shape[1]:
            raise ValueError('Zf and Zg must be (M,D) with equal D')
        D, M = Zf.shape[1], (Zf.shape[0], Zg.shape[0])
        self.shape = dict(Mf=M[0], Mg=M[1], D=D)
        if self.full:
            for b in (4, 5):
                q, Mh = ps[b], M[b - 4]
                if q.transform.N != Mh or q.value.shape not in ((Mh, Mh), (Mh, Mh, 1)):
                    raise ValueError('%s must be a LowerTriangular(%d) matrix of shape (%d, %d) or (%d, %d, 1), not %r of shape %r'
                                     % (DENSE_FIT_KEYS[b], Mh, Mh, Mh, Mh, Mh, q.transform, q.value.shape))
        self.sizes = [q.free_size() for q in ps]       # entries of the FREE vectors: M (M + 1) / 2 for a full factor
        ns = [Mh * (Mh + 1) // 2 if self.full else Mh for Mh in M]
        want = [Zf.size, Zg.size, M[0], M[1], ns[0], ns[1], None, None, 1, 1, 1]
        for k, n, w in zip(DENSE_FIT_KEYS, self.sizes, want):
            if (w is None and n not in (1, D)) or (w is not None and n != w):
                raise ValueError('%s has %d entries' % (k, n))
        self.ell_size = (self.sizes[6], self.sizes[7])
        self.positive = [isinstance(q.transform, Log1pe) for q in ps]
        self.m, self.v = np.zeros(sum(self.sizes)), np.zeros(sum(self.sizes))
        self.t = 0
        self.resync()

    def _engine_call(self, n_steps, **kw):
        return self.engine.fit_steps_mode(self.mode, self.shape, self.x, self.m, self.v, self.lr, self.positive, self.trainable, self.ell_size,
                                          self.t, n_steps, **kw)
