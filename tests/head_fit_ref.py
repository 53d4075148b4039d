"""Host-side yardsticks of the heads' device fit loop (zigp_kron_head_fit_steps), shared by test_cpu_head_fit.py and test_gpu_head_fit.py.

* `ref_head_fit_steps` restates the call in NumPy on top of an elbo-and-gradient function: block order, Log1pe chain, Adam, row ranges
  and host wrap-around batches, untrainable blocks (the single-latent twin of dense_fit_ref.ref_fit_steps).
* `host_loop` is the loop the device loop replaces: kron_head_elbo + AdamGroups, one step per batch; with `nudge_seed` every free-state
  element is moved by a seeded +-1 ulp after every step (the measure of how far two legitimate runs drift apart).
* `OracleHeadEngine` stands in for DenseEngine on a machine without a GPU (oracle/zigp_oracle_torch.kron_head_elbo_and_grad).
* `head_problem` is the well-conditioned problem both files fit.
"""
import numpy as np

from zigp.optim import AdamGroups
from onofftf.heads import HEAD_FIT_BLOCK_NAMES, head_engine_params, head_f_mu, init_head_params, named_head_grads

N_ROWS, BATCH, JITTER = 3000, 500, 1e-5
SCALE = N_ROWS / BATCH
GRAD_KEYS = (('Zf', 0), ('Zf', 1), ('u_fm', None), ('u_fs_sqrt', None), ('ell_f', 0), ('ell_f', 1), ('var_f', 0), ('var_f', 1), ('noise', None),
             ('f_mu', None))      # the engine's gradient entry of each block of HEAD_FIT_BLOCK_NAMES


def head_problem(grid, lik):
    """make_kron_problem(3000, 4, 4, seed=21) rows; init_head_params with kmeans_seed 3, RandomState(9); ell_0 = [1.2, 1.5],
    ell_1 = 1.5 / (M1 - 1), variances 2.0 / 1.5, noise 0.05 (cond(K_p) ~ 1e2-1e3); 0/1 labels Y > 0 for the classifier.
    Returns (X, Y, make_pset): make_pset() builds a fresh, identical ParamSet."""
    from test_gpu_kron import make_kron_problem
    X, Y, _ = make_kron_problem(N_ROWS, 4, 4, seed=21)
    if lik == 'bernoulli':
        Y = (Y > 0) * 1.0

    def make_pset():
        ps = init_head_params(X, grid, lik, include_f_mu=(lik == 'bernoulli'), kmeans_seed=3, rng=np.random.RandomState(9))
        ps.params['f_kern/lengthscale_0'].value = np.array([1.2, 1.5])
        ps.params['f_kern/lengthscale_1'].value = np.array([1.5 / max(grid[1] - 1, 1)])
        ps.params['f_kern/variance_0'].value = np.array([2.0])
        ps.params['f_kern/variance_1'].value = np.array([1.5])
        if lik == 'gaussian':
            ps.params['likelihood/variance'].value = np.array(0.05)
        return ps

    return X, Y, make_pset


def rows_with_a_wrap(n_steps, seed=2):
    """n_steps row offsets into the resident set with ONE host wrap-around batch (-1) mid-way, and the rows of that batch"""
    rs = np.random.RandomState(seed)
    seq = [int(r) for r in rs.randint(0, N_ROWS - BATCH, size=n_steps)]
    seq[n_steps // 2] = -1
    return seq, rs.permutation(N_ROWS)[:BATCH]


def oracle_eg(lik):
    """elbo-and-gradient function on the CPU oracle: (Xb, Yb, p, f_mu, jitter, scale) -> (scale * data, kl, grads)"""
    import zigp_oracle_torch as ot

    def eg(Xb, Yb, p, f_mu, jitter, scale):
        elbo, data, kl, g = ot.kron_head_elbo_and_grad(Xb, Yb, p, lik, jitter, scale=scale, f_mu=f_mu)
        return scale * data, kl, g
    return eg


def block_sizes(shape):
    M0, M1, D0, D1 = shape['M0f'], shape['M1f'], shape['D0'], shape['D1']
    return [M0 * D0, M1 * D1, M0 * M1, M0 * M1, D0, D1, 1, 1, 1, 1]


def flat_state(pset):
    """(x, lr, positive, trainable, shape) of a ParamSet in the block layout of include/zigp.h, as HeadDeviceFit builds them"""
    from onofftf.heads import HeadDeviceFit
    f = HeadDeviceFit(None, pset, 'gaussian' if 'likelihood/variance' in pset.params else 'bernoulli')
    return f.x.copy(), list(f.lr), list(f.positive), list(f.trainable), dict(f.shape)


def ref_head_fit_steps(elbo_grad, Xres, Yres, shape, x, m, v, lr, positive, trainable, t0, row_begin, batch, jitter=1e-5, scale=1.0,
                       Xw=None, Yw=None, beta1=0.9, beta2=0.999, eps=1e-8, lower=1e-6):
    """engine.kron_head_fit_steps restated: elbo_grad(Xb, Yb, p, f_mu, jitter, scale) -> (elbo_data, kl, grads w.r.t. the constrained
    values).  x, m, v are updated in place; returns (elbo_data[n], kl[n]), each entry at the parameters before its step's update."""
    sizes = block_sizes(shape)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert x.size == offs[-1]
    M0, M1, D0, D1 = shape['M0f'], shape['M1f'], shape['D0'], shape['D1']
    Xres, Yres = np.asarray(Xres), np.asarray(Yres).reshape(-1, 1)
    n = len(row_begin)
    ed, kl = np.zeros(n), np.zeros(n)
    for i, rb in enumerate(row_begin):
        val = [np.logaddexp(0.0, x[offs[b]:offs[b + 1]]) + lower if positive[b] else x[offs[b]:offs[b + 1]].copy() for b in range(10)]
        p = dict(Zf=[val[0].reshape(M0, D0), val[1].reshape(M1, D1)], u_fm=val[2].reshape(-1, 1), u_fs_sqrt=val[3].reshape(-1, 1),
                 ell_f=[val[4], val[5]], var_f=[val[6], val[7]], noise=float(val[8][0]))
        if rb >= 0:
            Xb, Yb = Xres[rb:rb + batch], Yres[rb:rb + batch]
        else:
            k = -int(rb) - 1
            Xb, Yb = np.asarray(Xw)[k * batch:(k + 1) * batch], np.asarray(Yw).reshape(-1, 1)[k * batch:(k + 1) * batch]
        ed[i], kl[i], g = elbo_grad(Xb, Yb, p, float(val[9][0]), jitter, scale)
        t = t0 + i + 1
        for b, (key, q) in enumerate(GRAD_KEYS):
            if not trainable[b]:
                continue
            sl = slice(offs[b], offs[b + 1])
            gc = np.asarray(g[key] if q is None else g[key][q], dtype=np.float64).reshape(-1)
            gx = -(gc * (0.5 * (1.0 + np.tanh(0.5 * x[sl]))) if positive[b] else gc)
            m[sl] = beta1 * m[sl] + (1 - beta1) * gx
            v[sl] = beta2 * v[sl] + (1 - beta2) * gx * gx
            x[sl] = x[sl] - lr[b] * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m[sl] / (np.sqrt(v[sl]) + eps)
    return ed, kl


class OracleHeadEngine:
    """set_data / kron_head_elbo / kron_head_fit_steps of DenseEngine, computed by the CPU oracle; records its calls"""
    LIK = ('gaussian', 'bernoulli')

    def __init__(self):
        self.X = self.Y = None
        self.fit_calls, self.elbo_calls = [], 0

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64).reshape(-1, 1)

    def kron_head_elbo(self, p, X=None, Y=None, lik=None, jitter=1e-5, scale=1.0, f_mu=0.0, include_kl=True, need_grad=True, rows=None):
        self.elbo_calls += 1
        if rows is not None:
            X, Y = self.X[rows[0]:rows[1]], self.Y[rows[0]:rows[1]]
        q = dict(p)
        q.setdefault('noise', 1.0)
        return oracle_eg(lik)(X, Y, q, f_mu, jitter, scale)

    def kron_head_fit_steps(self, shape, lik, x, m, v, lr, positive, trainable, t0, row_begin, batch, jitter=1e-5, scale=1.0, Xw=None, Yw=None,
                            beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        self.fit_calls.append(dict(lik=lik, t0=t0, row_begin=list(row_begin), batch=batch, lr=list(lr), positive=list(positive),
                                   trainable=list(trainable)))
        return ref_head_fit_steps(oracle_eg(lik), self.X, self.Y, shape, x, m, v, lr, positive, trainable, t0, row_begin, batch, jitter=jitter,
                                  scale=scale, Xw=Xw, Yw=Yw, beta1=beta1, beta2=beta2, eps=eps)


def host_loop(eng, pset, lik, rows_seq, batch, jitter, scale, Xres, Yres, wraps=None, nudge_seed=None):
    """one kron_head_elbo + AdamGroups step per entry of rows_seq (>= 0: rows of (Xres, Yres); -(1 + k): batch k of wraps).  Returns the
    history [(elbo_data, kl)] -- each entry at the parameters before its step's update."""
    opt = AdamGroups(pset)
    rs = None if nudge_seed is None else np.random.RandomState(nudge_seed)
    hist = []
    for rb in rows_seq:
        if rb >= 0:
            xb, yb = Xres[rb:rb + batch], Yres[rb:rb + batch]
        else:
            k = -rb - 1
            xb, yb = wraps[0][k * batch:(k + 1) * batch], wraps[1][k * batch:(k + 1) * batch]
        ed, kl, g = eng.kron_head_elbo(head_engine_params(pset), xb, yb, lik, jitter=jitter, scale=scale, f_mu=head_f_mu(pset))
        hist.append((ed, kl))
        ng = named_head_grads(g)
        opt.step({k: ng[k] for k in pset.names()})
        if rs is not None:
            for k in pset.names():
                x = opt.x[k]
                opt.x[k] = np.nextafter(x, np.where(rs.randint(2, size=x.size) == 1, np.inf, -np.inf))
                pset.params[k].set_free(opt.x[k])
                opt._written[k] = pset.params[k].value.copy()
    return np.array(hist)


def block_distance(pset_a, pset_b):
    """worst parameter block: max |a - b| relative to the block's largest entry"""
    worst = 0.0
    for k in HEAD_FIT_BLOCK_NAMES:
        if k in pset_b.params:
            a, b = pset_a.params[k].value.reshape(-1), pset_b.params[k].value.reshape(-1)
            worst = max(worst, float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)))
    return worst


def hist_distance(ha, hb):
    """ELBO history: worst relative difference of the data term and of the KL over the steps"""
    ha, hb = np.asarray(ha, dtype=np.float64).reshape(-1, 2), np.asarray(hb, dtype=np.float64).reshape(-1, 2)
    return float(np.max(np.abs(ha - hb) / np.maximum(np.abs(hb), 1e-300)))


def bound(d):
    """how far the device loop may lie from the clean host run, d being the distance of the +-1-ulp-nudged host run: at every step the
    device's softplus and sigmoid may each differ from NumPy's by up to 2 ulp, in the value and in the chain factor (4), times 2 for the
    other summation order of the sums over points; 1e-13 ~ 2 eps x n_steps (the bound of tests/test_gpu_dense_fit.py)"""
    return max(8.0 * d, 1e-13)
