"""Host-side yardsticks of the dense device fit loop (zigp_fit_steps), shared by test_cpu_dense_fit.py and test_gpu_dense_fit.py.

* `make_pset` builds the ParamSet OnOffSVGP._pset builds (same keys, same order, same transforms) from a make_problem parameter dict.
* `host_loop` is the loop the device loop replaces: select_rows + elbo + AdamGroups, one step per row sample; with `nudge_seed` every
  free-state element is moved by a seeded +-1 ulp after every step (the measure of how far two legitimate runs drift apart).
* `OracleEngine` stands in for DenseEngine on a machine without a GPU (oracle/zigp_oracle_torch.py: torch autograd on the CPU).
* `ref_fit_steps` restates engine.fit_steps in NumPy on top of an elbo-and-gradient function: block order, Log1pe chain, Adam.
"""
from collections import OrderedDict

import numpy as np

from zigp.optim import P, ParamSet, AdamGroups, DENSE_FIT_KEYS
from zigp.transforms import Log1pe, Identity

POSITIVE = ('u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')


def make_pset(p, scalar_ell=(False, False), fixed=(), lr=0.01):
    """lr: one number, or a dict key -> learning rate"""
    q = OrderedDict()
    for k in DENSE_FIT_KEYS:
        v = np.atleast_1d(np.array(p[k], dtype=np.float64))
        if k in ('ell_f', 'ell_g') and scalar_ell[k == 'ell_g']:
            v = v[:1].copy()
        q[k] = P(v, Log1pe() if k in POSITIVE else Identity(), fixed=k in fixed, learning_rate=lr[k] if isinstance(lr, dict) else lr, name=k)
    return ParamSet(q)


def values(pset):
    """the engine's parameter dict (a one-entry lengthscale broadcasts over the D columns)"""
    D = pset.params['Zf'].value.shape[1]
    out = {}
    for k, q in pset.params.items():
        v = q.value
        if k in ('ell_f', 'ell_g'):
            v = np.full(D, float(v[0])) if v.size == 1 else v.reshape(-1)
        elif k in ('var_f', 'var_g', 'noise'):
            v = float(v.reshape(-1)[0])
        out[k] = v
    return out


def fold(pset, g):
    """ARD engine gradient -> the shape of each parameter (OnOffSVGP._fold_grads: a scalar lengthscale sums its D copies)"""
    out = {}
    for k, q in pset.params.items():
        a = np.asarray(g[k], dtype=np.float64).reshape(-1)
        out[k] = np.array([np.sum(a)]) if q.value.size == 1 and a.size > 1 else a
    return out


class OracleEngine:
    """select_rows / elbo of DenseEngine, computed by the CPU oracle"""

    def __init__(self, X, Y):
        import zigp_oracle_torch as ot
        self.ot, self.X, self.Y = ot, np.asarray(X), np.asarray(Y).reshape(-1, 1)
        self.sel = None

    def select_rows(self, idx=None):
        self.sel = None if idx is None or len(idx) == 0 else np.asarray(idx, dtype=np.int64)

    def elbo(self, p, jitter=1e-6, scale=1.0, **kw):
        X, Y = (self.X, self.Y) if self.sel is None else (self.X[self.sel], self.Y[self.sel])
        elbo, data, kl, g = self.ot.elbo_and_grad(X, Y, p, jitter, scale=scale)
        return scale * data, kl, g


def host_loop(eng, pset, rows, jitter, scale, n_steps=None, nudge_seed=None, callback=None):
    """rows: [n_steps, batch] row samples, or None for n_steps full-batch iterations over the rows that are active.  Returns the history
    [(elbo_data, kl)] -- each entry at the parameters before its step's update."""
    opt = AdamGroups(pset)
    rs = None if nudge_seed is None else np.random.RandomState(nudge_seed)
    hist = []
    for i in range(len(rows) if rows is not None else n_steps):
        if rows is not None:
            eng.select_rows(rows[i])
        ed, kl, g = eng.elbo(values(pset), jitter=jitter, scale=scale)
        hist.append((ed, kl))
        opt.step(fold(pset, g))
        if rs is not None:
            for k in pset.names():
                x = opt.x[k]
                opt.x[k] = np.nextafter(x, np.where(rs.randint(2, size=x.size) == 1, np.inf, -np.inf))
                pset.params[k].set_free(opt.x[k])
                opt._written[k] = pset.params[k].value.copy()
        if callback is not None:
            callback(i)
    if rows is not None:
        eng.select_rows(None)
    return np.array(hist)


def block_distance(pset_a, pset_b):
    """worst parameter block: max |a - b| relative to the block's largest entry"""
    worst = 0.0
    for k in DENSE_FIT_KEYS:
        a, b = pset_a.params[k].value.reshape(-1), pset_b.params[k].value.reshape(-1)
        worst = max(worst, float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)))
    return worst


def hist_distance(ha, hb):
    """ELBO history: worst relative difference of the data term and of the KL over the steps"""
    ha, hb = np.asarray(ha, dtype=np.float64).reshape(-1, 2), np.asarray(hb, dtype=np.float64).reshape(-1, 2)
    return float(np.max(np.abs(ha - hb) / np.maximum(np.abs(hb), 1e-300)))


def ref_fit_steps(elbo_grad, X, Y, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6, scale=1.0,
                  beta1=0.9, beta2=0.999, eps=1e-8, lower=1e-6):
    """engine.fit_steps restated: elbo_grad(Xb, Yb, p, jitter, scale) -> (elbo_data, kl, grads w.r.t. the constrained values, ARD
    lengthscales).  x, m, v are updated in place; returns (elbo_data[n], kl[n])."""
    Mf, Mg, D = shape['Mf'], shape['Mg'], shape['D']
    sizes = [Mf * D, Mg * D, Mf, Mg, Mf, Mg, ell_size[0], ell_size[1], 1, 1, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert x.size == offs[-1]
    X, Y = np.asarray(X), np.asarray(Y).reshape(-1, 1)
    ed, kl = np.zeros(n_steps), np.zeros(n_steps)
    for i in range(n_steps):
        p = {}
        for b, k in enumerate(DENSE_FIT_KEYS):
            xb = x[offs[b]:offs[b + 1]]
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
            gc = np.asarray(g[k], dtype=np.float64).reshape(-1)
            if sizes[b] == 1 and gc.size > 1:
                gc = np.array([np.sum(gc)])
            gx = -(gc * (0.5 * (1.0 + np.tanh(0.5 * x[sl]))) if positive[b] else gc)
            m[sl] = beta1 * m[sl] + (1 - beta1) * gx
            v[sl] = beta2 * v[sl] + (1 - beta2) * gx * gx
            x[sl] = x[sl] - lr[b] * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m[sl] / (np.sqrt(v[sl]) + eps)
    return ed, kl
