"""Host-side yardsticks of the dense device fit loop for the whitened models (zigp_fit_steps_mode, modes ZIGP_FIT_WHITE = 1 and
ZIGP_FIT_WHITE_FULL = 2), shared by test_cpu_white_fit.py and test_gpu_white_fit.py.  The companions of dense_fit_ref.py, whose
host_loop / block_distance / hist_distance work on these ParamSets as they are.

* `problem` turns a make_problem parameter dict into the mode's (mode 2: full factors from fullcov_ref.make_lq).
* `make_pset` builds the ParamSet OnOffSVGP._pset builds for whiten=True (mode 1: Log1pe vectors) or whiten=True, q_diag=False (mode 2:
  transforms.LowerTriangular matrices).
* `ModeEngine` gives any engine's elbo the mode's `whiten` / `q_diag` entries, so that dense_fit_ref.host_loop runs the mode's model.
* `RefEngine` stands in for DenseEngine without a GPU (whiten_ref / fullcov_ref: torch autograd on the CPU).
* `ref_fit_steps` restates engine.fit_steps_mode in NumPy: block order, triangular blocks with the identity transform, Log1pe chain, Adam.
"""
from collections import OrderedDict

import numpy as np

from zigp.optim import P, ParamSet, DENSE_FIT_KEYS
from zigp.transforms import Log1pe, Identity, LowerTriangular

WHITE, WHITE_FULL = 1, 2
POSITIVE = ('u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')
S_KEYS = ('u_fs_sqrt', 'u_gs_sqrt')


def problem(p, mode, lq_seed=0, negative=0):
    """the parameter dict of the mode's model: whiten=True and, for mode 2, q_diag=False with (M, M) factors (fullcov_ref.make_lq)"""
    if mode == WHITE_FULL:
        import fullcov_ref
        return fullcov_ref.make_lq(p, seed=lq_seed, negative=negative)
    return dict(p, whiten=True)


def make_pset(p, mode, scalar_ell=(False, False), fixed=(), lr=0.01, trailing_axis=False):
    """lr: one number, or a dict key -> learning rate; trailing_axis: mode-2 factors as (M, M, 1), the model's own shape"""
    q = OrderedDict()
    for k in DENSE_FIT_KEYS:
        v = np.array(p[k], dtype=np.float64)
        if mode == WHITE_FULL and k in S_KEYS:
            tr = LowerTriangular(v.shape[0])
            v = np.tril(v)[:, :, None] if trailing_axis else np.tril(v)
        else:
            v = np.atleast_1d(v)
            if k in ('ell_f', 'ell_g') and scalar_ell[k == 'ell_g']:
                v = v[:1].copy()
            tr = Log1pe() if k in POSITIVE else Identity()
        q[k] = P(v, tr, fixed=k in fixed, learning_rate=lr[k] if isinstance(lr, dict) else lr, name=k)
    return ParamSet(q)


def flags(mode):
    return dict(whiten=True, q_diag=False) if mode == WHITE_FULL else dict(whiten=True)


class ModeEngine:
    """select_rows / elbo of `eng` with the mode's flags added to the parameter dict (dense_fit_ref.values knows the 11 keys only)"""

    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def select_rows(self, idx=None):
        return self.eng.select_rows(idx)

    def elbo(self, p, **kw):
        q = dict(p, **flags(self.mode))
        if self.mode == WHITE_FULL:
            for k in S_KEYS:
                q[k] = np.asarray(q[k]).reshape(np.asarray(q[k]).shape[0], -1)
        return self.eng.elbo(q, **kw)


def ref_elbo_grad(mode):
    """(Xb, Yb, p, jitter, scale) -> (scale * data term, kl, grads w.r.t. the constrained values) from the mode's CPU reference"""
    if mode == WHITE_FULL:
        import fullcov_ref as ref
    else:
        import whiten_ref as ref

    def eg(Xb, Yb, p, jitter, scale):
        q = {k: v for k, v in p.items() if k not in ('whiten', 'q_diag')}
        elbo, data, kl, g = ref.elbo_and_grad(Xb, Yb, q, jitter, scale=scale)
        return scale * data, kl, g
    return eg


class RefEngine:
    """select_rows / elbo of DenseEngine for the mode's model, computed by whiten_ref / fullcov_ref"""

    def __init__(self, X, Y, mode):
        self.X, self.Y, self.mode = np.asarray(X), np.asarray(Y).reshape(-1, 1), mode
        self.eg = ref_elbo_grad(mode)
        self.sel = None

    def select_rows(self, idx=None):
        self.sel = None if idx is None or len(idx) == 0 else np.asarray(idx, dtype=np.int64)

    def elbo(self, p, jitter=1e-6, scale=1.0, **kw):
        X, Y = (self.X, self.Y) if self.sel is None else (self.X[self.sel], self.Y[self.sel])
        q = dict(p)
        if self.mode == WHITE_FULL:
            for k in S_KEYS:
                q[k] = np.asarray(q[k]).reshape(np.asarray(q[k]).shape[0], -1)
        return self.eg(X, Y, q, jitter, scale)


def block_sizes(mode, shape, ell_size):
    Mf, Mg, D = shape['Mf'], shape['Mg'], shape['D']
    ns = [M * (M + 1) // 2 if mode == WHITE_FULL else M for M in (Mf, Mg)]
    return [Mf * D, Mg * D, Mf, Mg, ns[0], ns[1], ell_size[0], ell_size[1], 1, 1, 1]


def flat_state(pset):
    """(free state, free sizes, learning rates, positive, trainable) in the block order of the call"""
    ps = [pset.params[k] for k in DENSE_FIT_KEYS]
    return (np.concatenate([q.free() for q in ps]), [q.free_size() for q in ps], [float(q.learning_rate) for q in ps],
            [isinstance(q.transform, Log1pe) for q in ps], [not q.fixed for q in ps])


def ref_fit_steps(mode, elbo_grad, X, Y, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6,
                  scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, lower=1e-6):
    """engine.fit_steps_mode restated for modes 1 and 2: elbo_grad(Xb, Yb, p, jitter, scale) -> (elbo_data, kl, grads w.r.t. the
    constrained values, ARD lengthscales; mode 2: (M, M) blocks for the factors).  Mode 2: blocks 4 and 5 are the lower triangles in
    row-major order, identity transform; the matrix handed to elbo_grad has an exactly zero strict upper triangle and the block's gradient
    is the lower triangle of the (M, M) gradient.  x, m, v are updated in place; returns (elbo_data[n], kl[n])."""
    assert mode in (WHITE, WHITE_FULL)
    Mf, Mg, D = shape['Mf'], shape['Mg'], shape['D']
    sizes = block_sizes(mode, shape, ell_size)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert x.size == offs[-1]
    tri = {4: np.tril_indices(Mf), 5: np.tril_indices(Mg)}
    if mode == WHITE_FULL:
        assert not positive[4] and not positive[5]
    X, Y = np.asarray(X), np.asarray(Y).reshape(-1, 1)
    ed, kl = np.zeros(n_steps), np.zeros(n_steps)
    for i in range(n_steps):
        p = {}
        for b, k in enumerate(DENSE_FIT_KEYS):
            xb = x[offs[b]:offs[b + 1]]
            if mode == WHITE_FULL and b in tri:
                M = (Mf, Mg)[b - 4]
                p[k] = np.zeros((M, M))
                p[k][tri[b]] = xb
            else:
                p[k] = np.logaddexp(0.0, xb) + lower if positive[b] else xb.copy()
        p['Zf'], p['Zg'] = p['Zf'].reshape(Mf, D), p['Zg'].reshape(Mg, D)
        for k in ('ell_f', 'ell_g'):
            if p[k].size == 1:
                p[k] = np.full(D, p[k][0])
        for k in ('var_f', 'var_g', 'noise'):
            p[k] = float(p[k][0])
        idx = slice(None) if rows is None else np.asarray(rows).reshape(-1)[i * batch:(i + 1) * batch]
        ed[i], kl[i], g = elbo_grad(X[idx], Y[idx], p, jitter, scale)
        t = t0 + i + 1
        for b, k in enumerate(DENSE_FIT_KEYS):
            if not trainable[b]:
                continue
            sl = slice(offs[b], offs[b + 1])
            if mode == WHITE_FULL and b in tri:
                gc = np.asarray(g[k], dtype=np.float64).reshape(p[k].shape)[tri[b]]
            else:
                gc = np.asarray(g[k], dtype=np.float64).reshape(-1)
                if sizes[b] == 1 and gc.size > 1:
                    gc = np.array([np.sum(gc)])
            gx = -(gc * (0.5 * (1.0 + np.tanh(0.5 * x[sl]))) if positive[b] else gc)
            m[sl] = beta1 * m[sl] + (1 - beta1) * gx
            v[sl] = beta2 * v[sl] + (1 - beta2) * gx * gx
            x[sl] = x[sl] - lr[b] * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m[sl] / (np.sqrt(v[sl]) + eps)
    return ed, kl
