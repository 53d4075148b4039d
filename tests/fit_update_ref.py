"""The update kernels of the device fit loops restated as pure functions (tests/test_cpu_fit_update_ref.py pins them, tests/
test_gpu_fit_update_stages.py holds the kernels to them).

* `kron_step` is one launch of k_fit_update<HEAD> with update = 1 (csrc/zigp_kronf.hip): (x, m, v, parameter image with both
  hyperparameter blocks, raw result block) -> the same after the update, the history entry and the failure record.  `kron_image` is the
  launch with update = 0.
* `dense_step` is k_dense_fit_update followed by k_dense_fit_image (+ k_dense_fit_image_tri), `dense_image` the image launches alone
  (csrc/zigp_kernels.h).

Each exists for dtype = np.float64 -- operation for operation as the kernels and zigp.optim.AdamGroups do it, contraction off -- and for
np.longdouble (the truth of the bound tier; the inputs are the same doubles).  The two factors of the learning rate that depend on t come
from the host in double in the kernels, so they are inputs here too: `lr_factors`.

`mut`: a set of names of deliberate mistakes (KRON_MUTATIONS, DENSE_MUTATIONS, ADAM_MUTATIONS); the mutation tier of the CPU test shows
that the acceptance rule of the GPU tests resolves every one of them on the fixtures those tests use.

Every function returns, next to a value, its first-order error weight S (nested absolute values): a sum weighs the absolute values of
its terms, a product or quotient its own absolute value, sigmoid = 0.5 (1 + tanh) weighs 0.5 (1 + |tanh|) -- the cancellation at
negative x belongs to the formula.  Through the Adam step:
  S_g = S_gc S_sig;  S_m = b1 |m| + (1 - b1) S_g;  S_v = b2 |v| + 2 (1 - b2) |g| S_g;
  S_x = |x| + S_step,  S_step = lr_t S_m / (sqrt v' + eps) + |step| (S_v / (2 v')) sqrt v' / (sqrt v' + eps)   (terms with v' = 0 drop out).
"""
import numpy as np

EPS = np.finfo(np.float64).eps
KUF_C = float.fromhex('0x1.337cc2183b050p+2')      # sqrt(16 / ln 2): csrc/zigp_kernels.h
LOWER = 1e-6
ADAM_MUTATIONS = ('eps_inside', 'v_linear', 'beta_swap', 'g_sign', 'sigmoid_dropped', 'sigmoid_on_identity', 'softplus_no_lower',
                  'softplus_zero_branch')
KRON_MUTATIONS = ('z_ell_power', 'ell_ell_power', 'z_stride_other', 'dz_col_for_dell', 'var_cross_dropped', 'var_cross_own',
                  'var_cross_other_pws', 'noise_pws4', 'hyp_from_written', 'kl_m_swapped', 'kl_ranks_ignored', 'untrainable_not_rederived')
DENSE_MUTATIONS = ('ell_first_only', 'tri_column_major', 'zs_order')


def lr_factors(t, beta1=0.9, beta2=0.999):
    """(sqrt(1 - beta2^t), 1 - beta1^t) as kf_fit_run / dense_fit_steps and AdamGroups.step compute them: Python floats, t an int"""
    t = int(t)
    return float(np.sqrt(1 - float(beta2) ** t)), float(1 - float(beta1) ** t)


def softplus(x, dt=np.float64, mut=()):
    """kfit_softplus: np.logaddexp(0, x) + 1e-6 with numpy's branches (x < 0: log1p(exp(x)); x == 0: ln 2; else x + log1p(exp(-x)))"""
    x = np.asarray(x, dtype=dt)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        sp = np.logaddexp(dt(0.0), x)
    if 'softplus_zero_branch' in mut:
        sp = np.where(x == 0, dt(0.0), sp)
    return sp if 'softplus_no_lower' in mut else sp + dt(LOWER)


def sigmoid(x, dt=np.float64):
    """(value, S): 0.5 (1 + tanh(0.5 x)), zigp.transforms.Log1pe.grad_free"""
    x = np.asarray(x, dtype=dt)
    th = np.tanh(dt(0.5) * x)
    return dt(0.5) * (dt(1.0) + th), dt(0.5) * (dt(1.0) + np.abs(th))


def adam(gc, S_gc, x, m, v, positive, lr, lrf, beta1=0.9, beta2=0.999, eps=1e-8, dt=np.float64, mut=()):
    """kfit_adam on a block: gc = d ELBO / d (constrained value).  Returns dict x, m, v -> (value, S)."""
    gc, S_gc, x, m, v = (np.asarray(a, dtype=dt) for a in (gc, S_gc, x, m, v))
    b1, b2 = (dt(beta2), dt(beta1)) if 'beta_swap' in mut else (dt(beta1), dt(beta2))
    chain = (bool(positive) and 'sigmoid_dropped' not in mut) or (not positive and 'sigmoid_on_identity' in mut)
    with np.errstate(all='ignore'):
        if chain:
            sg, S_sg = sigmoid(x, dt)
            g, S_g = -(gc * sg), S_gc * S_sg
        else:
            g, S_g = -gc, S_gc
        if 'g_sign' in mut:
            g = -g
        mn = b1 * m + (dt(1.0) - b1) * g
        vn = b2 * v + ((dt(1.0) - b2) * g if 'v_linear' in mut else (dt(1.0) - b2) * g * g)
        S_m = b1 * np.abs(m) + (dt(1.0) - b1) * S_g
        S_v = b2 * np.abs(v) + dt(2.0) * (dt(1.0) - b2) * np.abs(g) * S_g
        lr_t = dt(lr) * dt(lrf[0]) / dt(lrf[1])
        den = np.sqrt(vn + dt(eps)) if 'eps_inside' in mut else np.sqrt(vn) + dt(eps)
        step = lr_t * mn / den
        xn = x - step
        rel_v = np.where(vn > 0, S_v / np.where(vn > 0, dt(2.0) * vn, dt(1.0)) * np.sqrt(vn) / den, dt(0.0))
        S_x = np.abs(x) + lr_t * S_m / den + np.abs(step) * rel_v
    return dict(x=(xn, S_x), m=(mn, S_m), v=(vn, S_v))


def seqsum(a, dt):
    """sum in index order from 0.0, as the kernels' loops (numpy's pairwise sum takes another order from 8 entries on)"""
    s = dt(0.0)
    for q in np.asarray(a, dtype=dt).reshape(-1):
        s = s + q
    return s


# =============================================================================================================================
# Kronecker loops: k_fit_update
# =============================================================================================================================
class KronLayout:
    """Blocks of the free vector and of the parameter image for a shape dict(M0f, M1f[, M0g, M1g], D0, D1) and lik 'onoff' (17 blocks) or a
    head (10).  `facts`: what zigp_test_kron_fit_update returns (DenseEngine.test_kron_fit_update_facts), or None: facts_for() computes
    the same numbers from kf_prepare's formulas (the CPU tests; the GPU tests compare the two)."""
    KH = dict(KH_SIZE=4 * 26 + 4, KH_FAC=26, KH_INV=0, KH_ZC=8, KH_ELL=16, KH_VAR=24, KH_NOISE=104, KH_FMU=105)      # MAXD = 8 (zigp_kernels.h)

    def __init__(self, shape, lik='onoff', facts=None):
        self.shape, self.lik, self.head = dict(shape), lik, lik != 'onoff'
        self.nlat = 1 if self.head else 2
        self.D = (int(shape['D0']), int(shape['D1']))
        self.M = [(int(shape['M0' + t]), int(shape['M1' + t])) for t in ('fg'[:self.nlat])]
        sizes = []
        for M0, M1 in self.M:
            sizes += [M0 * self.D[0], M1 * self.D[1], M0 * M1, M0 * M1, self.D[0], self.D[1], 1, 1]
        sizes += [1, 1] if self.head else [1]
        self.sizes = sizes
        self.offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        self.n_free = int(self.offs[-1])
        self.nblocks = len(sizes)
        self.facts = facts if facts is not None else self.facts_for()

    def kind(self, b):
        """(latent, kind): 0 Z0, 1 Z1, 2 u, 3 s, 4 ell0, 5 ell1, 6 var0, 7 var1, 8 noise, 9 f_mu"""
        if self.head:
            return 0, b
        return (b // 8, 8 if b == 16 else b % 8)

    def sl(self, b):
        return slice(int(self.offs[b]), int(self.offs[b + 1]))

    def facts_for(self):
        m0, m1 = max(M[0] for M in self.M), max(M[1] for M in self.M)
        if self.D[0] > 7 or self.D[1] > 7 or not ((m0 <= 32 and m1 <= 32) or (m0 <= 16 and m1 <= 112)):
            raise ValueError('grid beyond the fused kernels')
        R0, R1 = (32, 32) if (m0 <= 32 and m1 <= 32) else (16, 112)
        f = dict(RES_KLV=0, RES_KROW0=8)
        f['RES_KROW1'] = 8 + R0 * 18
        f['RES_GU'] = f['RES_KROW1'] + R1 * 18
        f['RES_GS'] = f['RES_GU'] + R0 * R1
        f['RES_SIZE'] = f['RES_GS'] + R0 * R1
        f['RES_PWS'] = 2 * f['RES_SIZE']
        f['RES_INFO'] = f['RES_PWS'] + 8
        f['n_res'] = f['RES_INFO'] + 8
        off, oz, ou, os_ = 0, [-1] * 4, [-1] * 2, [-1] * 2
        for h, (M0, M1) in enumerate(self.M):
            oz[2 * h] = off; off += M0 * self.D[0]
            oz[2 * h + 1] = off; off += M1 * self.D[1]
            ou[h] = off; off += M0 * M1
            os_[h] = off; off += M0 * M1
        f.update(off_z=oz, off_u=ou, off_s=os_, off_hyp=off, off_hyp2=off + self.KH['KH_SIZE'], n_img=off + 2 * self.KH['KH_SIZE'])
        big = [b for b in range(self.nblocks) if b < 8 * self.nlat and b % 8 <= 3]
        hyp = [b for b in range(self.nblocks) if b not in big]
        bo, ho = list(np.cumsum([0] + [self.sizes[b] for b in big])), list(np.cumsum([0] + [self.sizes[b] for b in hyp]))
        f['big_off'] = [int(a) for a in bo + [bo[-1]] * (9 - len(bo))]
        f['hyp_off'] = [int(a) for a in ho + [ho[-1]] * (10 - len(ho))]
        f['grid'] = (f['big_off'][8] + 255) // 256 + 1
        f.update(self.KH)
        return f

    def dst(self, b):
        """image offset of a plain block (Z0, Z1, u, s)"""
        h, k = self.kind(b)
        f = self.facts
        return (f['off_z'][2 * h], f['off_z'][2 * h + 1], f['off_u'][h], f['off_s'][h])[k]

    def rec(self, h, q):
        return (2 * h + q) * self.facts['KH_FAC']

    def element_map(self):
        """kfit_element for every (workgroup, thread) of the launch: list of (block, index) or None, from the facts' offsets"""
        f = self.facts
        big = [b for b in range(self.nblocks) if b < 8 * self.nlat and b % 8 <= 3]
        hyp = [b for b in range(self.nblocks) if b not in big]
        out = []
        for wg in range(f['grid']):
            last = wg == f['grid'] - 1
            off, blk, nb = (f['hyp_off'], hyp, 9) if last else (f['big_off'], big, 8)
            for t in range(256):
                j = t if last else wg * 256 + t
                if j >= off[nb]:
                    out.append(None)
                    continue
                k = sum(1 for q in range(1, nb) if j >= off[q])
                out.append((blk[k], j - off[k]))
        return out


def kron_store(L, img, Hn, b, val, dt):
    """kfit_store_value for a whole block; Hn = offset of the hyperparameter block written"""
    f = L.facts
    h, k = L.kind(b)
    val = np.asarray(val, dtype=dt).reshape(-1)
    if k <= 3:
        img[L.dst(b):L.dst(b) + val.size] = val
    elif k <= 5:
        R = Hn + L.rec(h, k - 4)
        img[R + f['KH_ELL']:R + f['KH_ELL'] + val.size] = val
        with np.errstate(all='ignore'):
            img[R + f['KH_INV']:R + f['KH_INV'] + val.size] = dt(1.0) / val
    elif k <= 7:
        img[Hn + L.rec(h, k - 6) + f['KH_VAR']] = val[0]
    elif k == 8:
        img[Hn + f['KH_NOISE']] = val[0]
    else:
        img[Hn + f['KH_FMU']] = val[0]


def kron_image(L, x, positive, img, dt=np.float64, mut=()):
    """the launch with update = 0: free state -> image, hyperparameter block 0.  img: float64 [n_img] as the call's memset left it (the
    hyperparameter blocks zero); returns the new image in dt"""
    out = np.asarray(img, dtype=dt).copy()
    for b in range(L.nblocks):
        xb = np.asarray(x[L.sl(b)], dtype=dt)
        kron_store(L, out, L.facts['off_hyp'], b, softplus(xb, dt, mut) if positive[b] else xb, dt)
    return out


def kron_failed(L, res):
    """the failure rule: (job, pivot) of the first factor job whose status int is not 0, or None"""
    f = L.facts
    ints = np.ascontiguousarray(res[f['RES_INFO']:f['RES_INFO'] + 8]).view(np.int32)
    for j in range(2 * L.nlat):
        if ints[2 * j] != 0:
            return j, int(ints[2 * j])
    return None


def kron_grads(L, res, img, step, dt=np.float64, mut=()):
    """The device chain rule: per block (gc, S) from the raw result block and the hyperparameter block the step read (block step % 2 of img)"""
    f = L.facts
    res = np.asarray(res, dtype=dt)
    img = np.asarray(img, dtype=dt)
    Ho = f['off_hyp2'] if step & 1 else f['off_hyp']
    if 'hyp_from_written' in mut:
        Ho = f['off_hyp'] if step & 1 else f['off_hyp2']
    pws = res[f['RES_PWS']:f['RES_PWS'] + 8]
    out = []
    with np.errstate(all='ignore'):
        for b in range(L.nblocks):
            h, k = L.kind(b)
            R = h * f['RES_SIZE']
            n = L.sizes[b]
            if k <= 1:
                q, D, Do = k, L.D[k], L.D[1 - k]
                Dm = Do if 'z_stride_other' in mut else D
                i = np.arange(n)
                mm, dd = i // Dm, i - (i // Dm) * Dm
                num = res[R + f[('RES_KROW0', 'RES_KROW1')[q]] + mm * (2 + 2 * Dm) + 1 + dd]
                ell = img[Ho + L.rec(h, q) + f['KH_ELL'] + dd]
                gc = num / ell if 'z_ell_power' in mut else num / (ell * ell)
                S = np.abs(gc)
            elif k <= 3:
                o = R + f['RES_GU' if k == 2 else 'RES_GS']
                gc = res[o:o + n].copy()
                S = np.abs(gc)
            elif k <= 5:
                q, D = k - 4, L.D[k - 4]
                W, M = 2 + 2 * D, L.M[h][k - 4]
                o = R + f[('RES_KROW0', 'RES_KROW1')[q]]
                ell = img[Ho + L.rec(h, q) + f['KH_ELL']:Ho + L.rec(h, q) + f['KH_ELL'] + D]
                c0 = 1 if 'dz_col_for_dell' in mut else 1 + D
                sm = np.array([seqsum(res[o + np.arange(M) * W + c0 + d], dt) for d in range(D)], dtype=dt)
                sa = np.array([seqsum(np.abs(res[o + np.arange(M) * W + c0 + d]), dt) for d in range(D)], dtype=dt)
                den = ell * ell if 'ell_ell_power' in mut else ell * ell * ell
                gc, S = sm / den, sa / np.abs(den)
            elif k <= 7:
                q, D = k - 6, L.D[k - 6]
                W, M = 2 + 2 * D, L.M[h][k - 6]
                o = R + f[('RES_KROW0', 'RES_KROW1')[q]]
                var = img[Ho + L.rec(h, q) + f['KH_VAR']]
                vo = img[Ho + L.rec(h, 1 - q) + f['KH_VAR']]
                col = res[o + np.arange(M) * W]
                pw = pws[2 + ((1 - h) if 'var_cross_other_pws' in mut else h)]
                cross = pw * (var if 'var_cross_own' in mut else vo)
                if 'var_cross_dropped' in mut:
                    cross = dt(0.0) * cross
                gc = np.array([seqsum(col, dt) / var + cross], dtype=dt)
                S = np.array([seqsum(np.abs(col), dt) / np.abs(var) + np.abs(cross)], dtype=dt)
            else:
                gc = np.array([pws[4 if (k == 9 or 'noise_pws4' in mut) else 1]], dtype=dt)
                S = np.abs(gc)
            out.append((gc, S))
    return out


def kron_history(L, res, dt=np.float64, mut=()):
    """(data term, KL) as k_fit_update's thread 64 assembles them (kron_kl, csrc/zigp_kronc.h)"""
    f = L.facts
    res = np.asarray(res, dtype=dt)
    pws = res[f['RES_PWS']:f['RES_PWS'] + 8]
    ranks = dt(1.0) if 'kl_ranks_ignored' in mut else pws[7]
    kl = dt(0.0)
    if ranks > 0:
        for h in range(L.nlat):
            vk = res[h * f['RES_SIZE']:h * f['RES_SIZE'] + 5]
            M0, M1 = (L.M[h][1], L.M[h][0]) if 'kl_m_swapped' in mut else L.M[h]
            kl = kl + dt(0.5) * (vk[0] - ranks * dt(L.M[h][0]) * dt(L.M[h][1]) - vk[1] + vk[2] + dt(M1) * vk[3] + dt(M0) * vk[4])
    return pws[0], kl


def kron_step(L, x, m, v, img, res, step, t, lr, positive, trainable=None, beta1=0.9, beta2=0.999, eps=1e-8, dt=np.float64, mut=(),
              x_image=None):
    """One launch with update = 1.  x, m, v, img, res: float64 (the device's own values).  x_image: the free state the image is derived
    from in place of this function's own new x (the bound tier hands in the device's new x, so that the image is judged as a function of
    its own input).  Returns dict(x, m, v, img: new values in dt;
    S_x, S_m, S_v, S_img: weights; hist: (data, kl) or None; fail: None or (job, pivot)).  A failing step changes nothing."""
    f = L.facts
    bad = kron_failed(L, res)
    xs, ms, vs, im = (np.asarray(a, dtype=dt).copy() for a in (x, m, v, img))
    S = dict(S_x=np.abs(xs), S_m=np.abs(ms), S_v=np.abs(vs), S_img=np.abs(im))
    if bad is not None:
        return dict(x=xs, m=ms, v=vs, img=im, hist=None, fail=bad, **S)
    Hn = f['off_hyp'] if step & 1 else f['off_hyp2']
    lrf = lr_factors(t, beta1, beta2)
    grads = kron_grads(L, res, img, step, dt, mut)
    for b in range(L.nblocks):
        sl = L.sl(b)
        xb = xs[sl]
        if trainable is None or trainable[b]:
            r = adam(grads[b][0], grads[b][1], x[sl], m[sl], v[sl], positive[b], lr[b], lrf, beta1, beta2, eps, dt, mut)
            xs[sl], ms[sl], vs[sl] = r['x'][0], r['m'][0], r['v'][0]
            S['S_x'][sl], S['S_m'][sl], S['S_v'][sl] = r['x'][1], r['m'][1], r['v'][1]
            xb = r['x'][0]
        elif 'untrainable_not_rederived' in mut:
            continue
        if x_image is not None:
            xb = np.asarray(x_image[sl], dtype=dt)
        kron_store(L, im, Hn, b, softplus(xb, dt, mut) if positive[b] else xb, dt)
    with np.errstate(all='ignore'):
        S['S_img'] = np.abs(im)
    return dict(x=xs, m=ms, v=vs, img=im, hist=kron_history(L, res, dt, mut), fail=None, **S)


def kron_run(L, x, m, v, blocks, t0, lr, positive, trainable=None, beta1=0.9, beta2=0.999, eps=1e-8, mut=()):
    """The whole call in float64, as zigp_test_kron_fit_update returns it: dict(snap_x, snap_m, snap_v [1 + n][n_free], snap_img, hist,
    fail [4], elbo_data, kl, steps_applied, rc)"""
    n = len(blocks)
    img = kron_image(L, x, positive, np.zeros(L.facts['n_img']), np.float64, mut)
    sx, sm, sv, si = [np.array(x, dtype=np.float64)], [np.array(m, dtype=np.float64)], [np.array(v, dtype=np.float64)], [img]
    hist, fail = np.zeros((n, 2)), np.zeros(4, dtype=np.int32)
    for i in range(n):
        if fail[0]:
            r = dict(x=sx[-1], m=sm[-1], v=sv[-1], img=si[-1])
        else:
            r = kron_step(L, sx[-1], sm[-1], sv[-1], si[-1], blocks[i], i, t0 + i + 1, lr, positive, trainable, beta1, beta2, eps, np.float64, mut)
            if r['fail'] is not None:
                fail[:3] = (1 + i, r['fail'][0], r['fail'][1])
            else:
                hist[i] = r['hist']
        sx.append(r['x']); sm.append(r['m']); sv.append(r['v']); si.append(r['img'])
    done = int(fail[0]) - 1 if fail[0] else n
    ed = np.where(np.arange(n) < done, hist[:, 0], np.nan)
    kl = np.where(np.arange(n) < done, hist[:, 1], np.nan)
    return dict(snap_x=np.array(sx), snap_m=np.array(sm), snap_v=np.array(sv), snap_img=np.array(si), hist=hist, fail=fail, elbo_data=ed, kl=kl,
                steps_applied=done, rc=-3 if fail[0] else 0)


# =============================================================================================================================
# dense loop: k_dense_fit_image, k_dense_fit_image_tri, k_dense_fit_update
# =============================================================================================================================
class DenseLayout:
    """Blocks of the free vector (DENSE_FIT_KEYS order), the packed result vector and the parameter image.  mode 0 diag, 1 white, 2 full.
    `facts`: what zigp_test_dense_fit_update returns, or None: computed from latents_layout's rule (Mp = M rounded up to 128, per latent
    Z (Mp D), ell (8), u (Mp), s (Mp), Zs (Mp D)); test_dense_update asserts that the two are equal."""
    DH = dict(DH_SIZE=2 * 26 + 2, DH_LAT=26, DH_INV=0, DH_ELL=8, DH_SCALE=16, DH_VAR=24, DH_PIVTOL=25, DH_NOISE=52)

    def __init__(self, mode, shape, ell_size, facts=None):
        self.mode, self.tri = int(mode), int(mode) == 2
        self.M, self.D, self.es = (int(shape['Mf']), int(shape['Mg'])), int(shape['D']), (int(ell_size[0]), int(ell_size[1]))
        M, D = self.M, self.D
        ns = [q * (q + 1) // 2 if self.tri else q for q in M]
        self.sizes = [M[0] * D, M[1] * D, M[0], M[1], ns[0], ns[1], self.es[0], self.es[1], 1, 1, 1]
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)
        self.n_free = int(self.offs[-1])
        self.goff, self.gn = [0] * 11, [1] * 11
        g = 16
        for h in range(2):
            self.goff[h], self.goff[2 + h], self.goff[4 + h] = g, g + M[h] * D, g + M[h] * D + M[h]
            self.goff[6 + h] = g + M[h] * D + M[h] + ns[h]
            self.gn[6 + h] = D if self.es[h] == 1 else 1
            g += M[h] * D + M[h] + ns[h] + D
        self.goff[8], self.goff[9], self.goff[10] = 2, 3, 4
        self.n_packed = g
        self.facts = facts if facts is not None else self.facts_for()

    def facts_for(self):
        f, off = dict(self.DH), 0
        Mp = [-(-q // 128) * 128 for q in self.M]
        names = ('img_Z', 'img_ell', 'img_u', 'img_s', 'img_Zs')
        for k in names:
            f[k] = [0, 0]
        for h in range(2):
            for k, n in zip(names, (Mp[h] * self.D, 8, Mp[h], Mp[h], Mp[h] * self.D)):
                f[k][h] = off
                off += n
        f.update(Mp=Mp, n_img=off, n_packed=self.n_packed, grid=-(-self.n_free // 256))
        return f

    def sl(self, b):
        return slice(int(self.offs[b]), int(self.offs[b + 1]))


def dense_image(L, x, positive, img, H, jitter, rtol_eps, dt=np.float64, mut=()):
    """k_dense_fit_image (+ _tri) on the image / block H as they are (float64).  Returns (img, H, Lraw [2] or None) in dt."""
    f, D = L.facts, L.D
    img, H = np.asarray(img, dtype=dt).copy(), np.asarray(H, dtype=dt).copy()
    val = [softplus(np.asarray(x[L.sl(b)], dtype=dt), dt, mut) if positive[b] else np.asarray(x[L.sl(b)], dtype=dt) for b in range(11)]
    Lraw = None
    with np.errstate(all='ignore'):
        for h in range(2):
            ell = np.full(D, val[6 + h][0], dtype=dt) if L.es[h] == 1 else val[6 + h]
            Z = val[h].reshape(L.M[h], D)
            Zs = (Z * dt(KUF_C)) / ell if 'zs_order' in mut else Z * (dt(KUF_C) * (dt(1.0) / ell))
            img[f['img_Z'][h]:f['img_Z'][h] + Z.size] = Z.reshape(-1)
            img[f['img_Zs'][h]:f['img_Zs'][h] + Z.size] = Zs.reshape(-1)
            img[f['img_u'][h]:f['img_u'][h] + L.M[h]] = val[2 + h]
            if not L.tri:
                img[f['img_s'][h]:f['img_s'][h] + L.M[h]] = val[4 + h]
            img[f['img_ell'][h]:f['img_ell'][h] + D] = ell
            R = h * f['DH_LAT']
            H[R + f['DH_ELL']:R + f['DH_ELL'] + D] = ell
            H[R + f['DH_INV']:R + f['DH_INV'] + D] = dt(1.0) / ell
            H[R + f['DH_SCALE']:R + f['DH_SCALE'] + D] = dt(KUF_C) * (dt(1.0) / ell)
            H[R + f['DH_VAR']] = val[8 + h][0]
            H[R + f['DH_PIVTOL']] = dt(rtol_eps) * (val[8 + h][0] + dt(jitter))
        H[f['DH_NOISE']] = val[10][0]
        if L.tri:
            Lraw = []
            for h in range(2):
                M = L.M[h]
                A = np.zeros((M, M), dtype=dt)
                r, c = np.tril_indices(M)
                if 'tri_column_major' in mut:
                    A.T[np.triu_indices(M)] = val[4 + h]      # column by column down from the diagonal
                else:
                    A[r, c] = val[4 + h]
                Lraw.append(A)
                img[f['img_s'][h]:f['img_s'][h] + M] = np.diag(A)
    return img, H, Lraw


def dense_grads(L, packed, dt=np.float64, mut=()):
    """per block (gc, S): the packed entries, a scalar lengthscale the sum of its D entries in d order"""
    p = np.asarray(packed, dtype=dt)
    out = []
    for b in range(11):
        n, gn = L.sizes[b], L.gn[b]
        g = p[L.goff[b]:L.goff[b] + n * gn].reshape(n, gn)
        if gn > 1 and 'ell_first_only' in mut:
            g = g[:, :1]
        out.append((np.array([seqsum(r, dt) for r in g], dtype=dt), np.array([seqsum(np.abs(r), dt) for r in g], dtype=dt)) if gn > 1
                   else (g[:, 0].copy(), np.abs(g[:, 0])))
    return out


def dense_step(L, x, m, v, img, H, packed, info, t, lr, positive, trainable, jitter, rtol_eps, beta1=0.9, beta2=0.999, eps=1e-8,
               dt=np.float64, mut=(), x_image=None):
    """k_dense_fit_update, then the image launches.  Returns dict(x, m, v, img, H, Lraw, S_x, S_m, S_v, hist, fail)."""
    xs, ms, vs = (np.asarray(a, dtype=dt).copy() for a in (x, m, v))
    S = dict(S_x=np.abs(xs), S_m=np.abs(ms), S_v=np.abs(vs))
    bad = (0, int(info[0])) if info[0] != 0 else ((1, int(info[1])) if info[1] != 0 else None)
    hist = None
    if bad is None:
        hist = (dt(packed[0]), dt(packed[1]))
        lrf = lr_factors(t, beta1, beta2)
        grads = dense_grads(L, packed, dt, mut)
        for b in range(11):
            if not trainable[b]:
                continue
            sl = L.sl(b)
            r = adam(grads[b][0], grads[b][1], x[sl], m[sl], v[sl], positive[b], lr[b], lrf, beta1, beta2, eps, dt, mut)
            xs[sl], ms[sl], vs[sl] = r['x'][0], r['m'][0], r['v'][0]
            S['S_x'][sl], S['S_m'][sl], S['S_v'][sl] = r['x'][1], r['m'][1], r['v'][1]
    im, Hn, Lraw = dense_image(L, xs if x_image is None else x_image, positive, img, H, jitter, rtol_eps, dt, mut)
    return dict(x=xs, m=ms, v=vs, img=im, H=Hn, Lraw=Lraw, hist=hist, fail=bad, **S)


def dense_run(L, x, m, v, packed, info, t0, lr, positive, trainable, jitter, rtol_eps, beta1=0.9, beta2=0.999, eps=1e-8, mut=()):
    """The whole call in float64, as zigp_test_dense_fit_update returns it (the image launches run after a failing step too: they rewrite
    the same values)"""
    n = len(packed)
    img, H, Lraw = dense_image(L, x, positive, np.zeros(L.facts['n_img']), np.zeros(L.facts['DH_SIZE']), jitter, rtol_eps, np.float64, mut)
    sx, sm, sv, si, sh, sl = [np.array(x, dtype=np.float64)], [np.array(m, dtype=np.float64)], [np.array(v, dtype=np.float64)], [img], [H], [Lraw]
    hist, fail = np.zeros((n, 2)), np.zeros(4, dtype=np.int32)
    for i in range(n):
        inf = (0, 0) if fail[0] else info[i]
        r = dense_step(L, sx[-1], sm[-1], sv[-1], si[-1], sh[-1], packed[i], inf, t0 + i + 1, lr, positive,
                       trainable if not fail[0] else [0] * 11, jitter, rtol_eps, beta1, beta2, eps, np.float64, mut)
        if not fail[0]:
            if r['fail'] is not None:
                fail[:3] = (1 + i, r['fail'][0], r['fail'][1])
            else:
                hist[i] = r['hist']
        sx.append(r['x']); sm.append(r['m']); sv.append(r['v']); si.append(r['img']); sh.append(r['H']); sl.append(r['Lraw'])
    done = int(fail[0]) - 1 if fail[0] else n
    ed = np.where(np.arange(n) < done, hist[:, 0], np.nan)
    kl = np.where(np.arange(n) < done, hist[:, 1], np.nan)
    return dict(snap_x=np.array(sx), snap_m=np.array(sm), snap_v=np.array(sv), snap_img=np.array(si), snap_H=np.array(sh),
                snap_Lraw=None if not L.tri else [np.array([q[h] for q in sl]) for h in range(2)], hist=hist, fail=fail, elbo_data=ed, kl=kl,
                steps_applied=done, rc=-3 if fail[0] else 0)


# =============================================================================================================================
# the acceptance rule
# =============================================================================================================================
def rule(dev, a, truth, S):
    """err_gpu <= 4 err_np + 16 eps S, element-wise; returns (ok, largest err_gpu / (eps S) over the elements whose eps S is a normal number).  An element
    whose truth is not finite must agree with (a) bit for bit (inf / nan are values the kernels reproduce, not errors to bound)."""
    dev, a = np.asarray(dev, dtype=np.float64).reshape(-1), np.asarray(a, dtype=np.float64).reshape(-1)
    truth, S = np.asarray(truth, dtype=np.longdouble).reshape(-1), np.asarray(S, dtype=np.longdouble).reshape(-1)
    fin = np.isfinite(truth) & np.isfinite(S)
    ok = bool(np.all(dev[~fin].view(np.int64) == a[~fin].view(np.int64)))
    with np.errstate(all='ignore'):
        eg, en = np.abs(dev[fin] - truth[fin]), np.abs(a[fin] - truth[fin])
        ok = ok and bool(np.all(eg <= 4 * en + 16 * EPS * S[fin])) and bool(np.all(np.isfinite(dev[fin])))
        pos = S[fin] > 2.0 ** -960      # below, eps S is no normal number: underflow, not rounding, sets the error (covered by err_np)
        ratio = float(np.max(eg[pos] / (EPS * S[fin][pos]))) if np.any(pos) else 0.0
    return ok, ratio


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


def bits_equal_msg(name, dev, ref, fails):
    if not same_bits(np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)):
        d, r = np.asarray(dev, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
        bad = np.flatnonzero(d.view(np.int64) != r.view(np.int64)) if d.shape == r.shape else [-1]
        fails.append('%s: %d elements differ in bits (first at %d)' % (name, len(bad), int(bad[0])))


# =============================================================================================================================
# fixtures (shared by the mutation tier of the CPU tests and by the GPU tests) and the acceptance checks
# =============================================================================================================================
SENT = float(np.frombuffer(bytes([0x7f]) * 8, dtype=np.float64)[0])      # ZIGP_STAGE_SENTINEL_BYTE in every byte


def kron_block(L, lats, pws, info=()):
    """DenseEngine.kron_result_block on this layout's facts"""
    from zigp.engine import DenseEngine
    return DenseEngine.kron_result_block(L.facts, L.shape, L.lik, lats, pws, info)


def _kron_lats(L, step, rs=None):
    """compact result arrays of one step: exact tier (rs None) -- integers times powers of two, distinct per element, mixed magnitudes down
    every column so that a sum depends on its order -- or random (bound tier)"""
    lats = []
    for h, (M0, M1) in enumerate(L.M):
        krow = []
        for q, (M, D) in enumerate(zip((M0, M1), L.D)):
            W = 2 + 2 * D
            mm, cc = np.meshgrid(np.arange(M), np.arange(W), indexing='ij')
            if rs is None:
                ident = 1.0 + cc + W * mm + 4000.0 * (2 * h + q) + 100000.0 * step
                kr = np.where((mm + cc) % 3 == 0, -1.0, 1.0) * ident * 2.0 ** (((3 * mm + 5 * cc) % 9) * 6 - 24)
            else:
                kr = rs.standard_normal((M, W)) * 10.0 ** rs.uniform(-2, 2, size=(M, W))
            kr[:, W - 1] = SENT      # the last column is not the update's to read
            krow.append(kr)
        e = np.arange(M0 * M1, dtype=np.float64)
        if rs is None:
            gu, gs = (10.0 + e + 3.0 * step + 50000.0 * h) / 8.0, -(7.0 + e + 5.0 * step + 70000.0 * h) / 4.0
            klv = np.array([3.5 + h, -1.25, 7.0 + step, 0.375 * (h + 1), -2.5])
        else:
            gu, gs = rs.standard_normal(M0 * M1) * 3.0, rs.standard_normal(M0 * M1) * 30.0
            klv = rs.standard_normal(5) * 100.0
        lats.append(dict(klv=klv, krow=krow, gu=gu, gs=gs))
    return lats


def kron_case(shape, lik, tier='exact', n_steps=3, t0=0, ranks=1.0, trainable=None, info=None, seed=0, facts=None):
    """A fixture of zigp_test_kron_fit_update: dict(L, x, m, v, lr, positive, trainable, t0, blocks [n][n_res], tier).
    tier 'exact': positive = 0 everywhere, ell powers of two, var powers of four, gradients distinct scaled integers, a learning rate per
    block.  tier 'bound': the transforms the models set (s, ell, var, noise positive), random state and gradients.
    info: {step: statuses of the factor jobs} injected Cholesky failures."""
    L = KronLayout(shape, lik, facts)
    rs = None if tier == 'exact' else np.random.RandomState(1000 + seed)
    x, positive = np.zeros(L.n_free), [0] * L.nblocks
    for b in range(L.nblocks):
        h, k = L.kind(b)
        i = np.arange(L.sizes[b], dtype=np.float64)
        if tier == 'exact':
            x[L.sl(b)] = ((i % 17 - 8) / 8.0 if k <= 1 else (i % 23 - 11) / 4.0 if k == 2 else 1.0 + i % 5 if k == 3 else
                          2.0 ** ((i + k + h) % 4 - 1) if k <= 5 else 4.0 ** ((h + k) % 3 - 1) if k <= 7 else 0.25 if k == 8 else 0.5)
        else:
            x[L.sl(b)] = rs.standard_normal(L.sizes[b]) * (2.0 if k != 9 else 0.5)
            positive[b] = int(3 <= k <= 8)
    e = np.arange(L.n_free, dtype=np.float64)
    if tier == 'exact':
        m, v = ((e * 7) % 13 - 6) / 1024.0, ((e * 5) % 11) / 2.0 ** 20
    else:
        m, v = rs.standard_normal(L.n_free) * 0.1, np.abs(rs.standard_normal(L.n_free)) * 1e-2
    lr = [1e-3 * (1 + b) for b in range(L.nblocks)]
    blocks = []
    for i in range(n_steps):
        pws = [-100.5 - i, 3.0 + i, 5.0 + 2 * i, 7.0 - i, 11.0 + i, SENT, SENT, ranks]
        if rs is not None:
            pws[:5] = list(rs.standard_normal(5) * 50.0)
        blocks.append(kron_block(L, _kron_lats(L, i, rs), pws, (info or {}).get(i, ())))
    return dict(L=L, x=x, m=m, v=v, lr=lr, positive=positive, trainable=trainable, t0=t0, blocks=np.array(blocks), tier=tier)


# x, |g|, (m, v) of the transform-edge fixture: every combination, in the s block (Log1pe) of a head or of latent g of the on/off model
EDGE_X = [s * a for a in (0.0, 5e-324, 1e-8, 1.0, 36.0, 37.5, 40.0, 709.0, 745.2, 1e3) for s in (1.0, -1.0)]
EDGE_G = [0.0, 1e-320, 1e-12, 1e-8, 1.0, 1e6, 1e9]
EDGE_MV = [(0.0, 0.0), (0.3, 1e-3), (-0.3, 1e-3), (1e-9, 1e-20)]


KL_SHAPES = dict(head=dict(M0f=3, M1f=20, D0=2, D1=1), onoff=dict(M0f=3, M1f=20, M0g=11, M1g=2, D0=2, D1=1))      # M0 != M1: test_kron_kl_history
EDGE_SHAPES = dict(head=dict(M0f=20, M1f=28, D0=1, D1=1), onoff=dict(M0f=3, M1f=5, M0g=20, M1g=28, D0=1, D1=1))


def kron_edge_case(lik, t0, facts=None):
    """A (20, 28) grid, D = (1, 1): the 560 entries of its s block hold EDGE_X x EDGE_G x EDGE_MV (gradient signs alternate), one step's
    result repeated three times.  A head carries the grid itself; lik 'onoff' carries it as latent g behind a (3, 5) latent f, so the
    elements sit behind f's blocks in the element map and read the second latent's result block.  c['edge_block'] is the block."""
    shape = EDGE_SHAPES['onoff' if lik == 'onoff' else 'head']
    c = kron_case(shape, lik, 'bound', n_steps=3, t0=t0, seed=7, facts=facts)
    L = c['L']
    combos = [(xe, g, mv) for xe in EDGE_X for g in EDGE_G for mv in EDGE_MV]
    eb = 11 if lik == 'onoff' else 3
    assert len(combos) == L.sizes[eb] and L.kind(eb)[1] == 3
    sl = L.sl(eb)
    c['x'][sl] = [q[0] for q in combos]
    c['m'][sl] = [q[2][0] for q in combos]
    c['v'][sl] = [q[2][1] for q in combos]
    gs = np.array([q[1] * (-1.0 if j % 2 else 1.0) for j, q in enumerate(combos)])
    f = L.facts
    o = L.kind(eb)[0] * f['RES_SIZE'] + f['RES_GS']
    c['blocks'][:, o:o + gs.size] = gs
    c['edge'], c['edge_block'] = combos, eb
    return c


def _classes(L):
    """output classes of the parity log: block kinds -> name"""
    names = {0: 'Z', 1: 'Z', 2: 'u', 3: 's', 4: 'ell', 5: 'ell', 6: 'var', 7: 'var', 8: 'noise', 9: 'f_mu'}
    return [names[L.kind(b)[1]] for b in range(L.nblocks)]


def kron_accept(case, out):
    """The acceptance rule of tests/test_gpu_fit_update_stages.py on what zigp_test_kron_fit_update (or a stand-in) returned.  Every step is
    judged as a function of the inputs the device itself held before it (snapshot i -> snapshot i + 1).  Returns (failures, ratios):
    failures a list of strings (empty: accepted), ratios {output class: largest err / (eps S)} of the bound tier."""
    L, f, fails, ratios = case['L'], case['L'].facts, [], {}
    exact = case['tier'] == 'exact'
    n = len(case['blocks'])
    kw = dict(lr=case['lr'], positive=case['positive'], trainable=case['trainable'])
    hyp = [f['off_hyp'], f['off_hyp2']]
    KS = f['KH_SIZE']

    def judge(name, dev, a, b, S):
        if exact:
            bits_equal_msg(name, dev, a, fails)
            return
        ok, r = rule(dev, a, b, S)
        ratios[name] = max(ratios.get(name, 0.0), r)
        if not ok:
            fails.append('%s: outside 4 err_np + 16 eps S (largest err / (eps S) = %.3g)' % (name, r))

    def structure(tag, img, Hw):
        """the written block: KH_INV == 1 / KH_ELL on the device's own values, zero slots d >= D and KH_ZC"""
        for h in range(L.nlat):
            for q in range(2):
                R, D = Hw + L.rec(h, q), L.D[q]
                with np.errstate(all='ignore'):
                    bits_equal_msg('%s KH_INV == 1 / KH_ELL (%d, %d)' % (tag, h, q), img[R + f['KH_INV']:R + f['KH_INV'] + D],
                                   1.0 / img[R + f['KH_ELL']:R + f['KH_ELL'] + D], fails)
                for o in ('KH_INV', 'KH_ZC', 'KH_ELL'):
                    lo = 0 if o == 'KH_ZC' else D
                    bits_equal_msg('%s zero slots %s (%d, %d)' % (tag, o, h, q), img[R + f[o] + lo:R + f[o] + 8], np.zeros(8 - lo), fails)
        if not np.all(np.isfinite(img)):
            fails.append('%s: the image is not finite' % tag)

    # ---- snapshot 0: the state as given, the image of the launch with update = 0, hyperparameter block 1 still the memset's zeros
    for k in 'xmv':
        bits_equal_msg('snapshot 0 ' + k, out['snap_' + k][0], case[k], fails)
    z = np.zeros(f['n_img'])
    ia = kron_image(L, case['x'], case['positive'], z, np.float64)
    ib = ia if exact else kron_image(L, case['x'], case['positive'], z, np.longdouble)
    judge('image 0', out['snap_img'][0], ia, ib, np.abs(ib))
    bits_equal_msg('image 0, block 1', out['snap_img'][0][hyp[1]:hyp[1] + KS], np.zeros(KS), fails)
    structure('image 0', out['snap_img'][0], hyp[0])
    # ---- the steps
    failed = 0
    cls = _classes(L)
    for i in range(n):
        x0, m0, v0, g0 = out['snap_x'][i], out['snap_m'][i], out['snap_v'][i], out['snap_img'][i]
        x1, m1, v1, g1 = out['snap_x'][i + 1], out['snap_m'][i + 1], out['snap_v'][i + 1], out['snap_img'][i + 1]
        bad = kron_failed(L, case['blocks'][i])
        if failed or bad is not None:
            for k, a0, a1 in (('x', x0, x1), ('m', m0, m1), ('v', v0, v1), ('image', g0, g1)):
                bits_equal_msg('step %d (failed) leaves %s' % (i, k), a1, a0, fails)
            if not failed:
                failed = 1 + i
                if tuple(int(q) for q in out['fail'][:3]) != (1 + i, bad[0], bad[1]):
                    fails.append('fail record %r, expected %r' % (tuple(out['fail'][:3]), (1 + i, bad[0], bad[1])))
            continue
        ra = kron_step(L, x0, m0, v0, g0, case['blocks'][i], i, case['t0'] + i + 1, dt=np.float64, x_image=None if exact else x1, **kw)
        rb = ra if exact else kron_step(L, x0, m0, v0, g0, case['blocks'][i], i, case['t0'] + i + 1, dt=np.longdouble, x_image=x1, **kw)
        for b in range(L.nblocks):
            sl = L.sl(b)
            if case['trainable'] is not None and not case['trainable'][b]:
                for k, a0, a1 in (('x', x0, x1), ('m', m0, m1), ('v', v0, v1)):
                    bits_equal_msg('step %d untrainable block %d %s' % (i, b, k), a1[sl], a0[sl], fails)
                continue
            for k, a1 in (('x', x1), ('m', m1), ('v', v1)):
                judge('%s %s' % (k, cls[b]) if not exact else 'step %d block %d %s' % (i, b, k), a1[sl], ra[k][sl], rb[k][sl], rb['S_' + k][sl])
        judge('image' if not exact else 'step %d image' % i, g1, ra['img'], rb['img'], rb['S_img'])
        Hr, Hw = hyp[i & 1], hyp[1 - (i & 1)]
        bits_equal_msg('step %d: the block it read' % i, g1[Hr:Hr + KS], g0[Hr:Hr + KS], fails)
        structure('step %d' % i, g1, Hw)
        bits_equal_msg('step %d history' % i, out['hist'][i], np.array(ra['hist'], dtype=np.float64), fails)      # IEEE in either tier
        for k in ('x', 'm', 'v'):
            if not np.all(np.isfinite(out['snap_' + k][i + 1])):
                fails.append('step %d: %s is not finite' % (i, k))
    # ---- what the entry point returns
    done = failed - 1 if failed else n
    if int(out['steps_applied']) != done or int(out['rc']) != (-3 if failed else 0) or (not failed and int(out['fail'][0]) != 0):
        fails.append('rc %r, steps_applied %r, fail %r (expected %d steps)' % (out['rc'], out['steps_applied'], list(out['fail']), done))
    for k, col in (('elbo_data', 0), ('kl', 1)):
        bits_equal_msg('returned %s' % k, out[k][:done], out['hist'][:done, col], fails)
        if not np.all(np.isnan(out[k][done:])):
            fails.append('returned %s: entries from the failing step on must be NaN' % k)
    return fails, ratios


# ---- dense loop
DENSE_POSITIVE = (0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1)      # OnOffSVGP._pset: u_fs_sqrt, u_gs_sqrt (diagonal q(u)), ell, var, noise


def dense_case(mode, shape, ell_size, tier='exact', n_steps=3, t0=0, trainable=None, info=None, seed=0, facts=None, jitter=0.25, pivot_rtol=8.0):
    """A fixture of zigp_test_dense_fit_update: dict(L, x, m, v, lr, positive, trainable, t0, packed [n][n_packed], info [n][2], jitter,
    rtol_eps, tier).  The tiers as kron_case; the D entries of a d ell gradient have mixed magnitudes, so their sum depends on its order."""
    L = DenseLayout(mode, shape, ell_size, facts)
    rs = None if tier == 'exact' else np.random.RandomState(2000 + seed)
    x, positive = np.zeros(L.n_free), [0] * 11
    for b in range(11):
        i = np.arange(L.sizes[b], dtype=np.float64)
        if tier == 'exact':
            x[L.sl(b)] = ((i % 17 - 8) / 8.0 if b <= 1 else (i % 23 - 11) / 4.0 if b <= 3 else 1.0 + (i + b) % 5 if b <= 5 else
                          2.0 ** ((i + b) % 4 - 1) if b <= 7 else 4.0 ** (b % 3 - 1) if b <= 9 else 0.25)
        else:
            x[L.sl(b)] = rs.standard_normal(L.sizes[b]) * 2.0
            positive[b] = DENSE_POSITIVE[b] if not (L.tri and b in (4, 5)) else 0
            if L.tri and b in (4, 5):
                x[L.sl(b)] += np.where(x[L.sl(b)] == 0, 1.0, 0.0)
            elif b == 4:
                x[L.sl(b)][0] = -0.0           # the x == 0 branch of the softplus, either sign, in the image kernel
            elif b == 10:
                x[L.sl(b)] = 0.0
    e = np.arange(L.n_free, dtype=np.float64)
    if tier == 'exact':
        m, v = ((e * 7) % 13 - 6) / 1024.0, ((e * 5) % 11) / 2.0 ** 20
    else:
        m, v = rs.standard_normal(L.n_free) * 0.1, np.abs(rs.standard_normal(L.n_free)) * 1e-2
    packed = np.full((n_steps, L.n_packed), SENT)
    for i in range(n_steps):
        j = np.arange(L.n_packed - 16, dtype=np.float64)
        if tier == 'exact':
            packed[i, :5] = [-100.5 - i, 12.25 + i, 5.0 + 2 * i, 7.0 - i, 11.0 + i]
            packed[i, 16:] = np.where(j % 3 == 0, -1.0, 1.0) * (1.0 + j + 100000.0 * i) * 2.0 ** ((j * 5) % 9 * 6 - 24)
        else:
            packed[i, :5] = rs.standard_normal(5) * 50.0
            packed[i, 16:] = rs.standard_normal(j.size) * 10.0 ** rs.uniform(-2, 2, size=j.size)
    inf = np.zeros((n_steps, 2), dtype=np.int32)
    for i, st in (info or {}).items():
        inf[i] = st
    return dict(L=L, x=x, m=m, v=v, lr=[1e-3 * (1 + b) for b in range(11)], positive=positive, trainable=trainable or [1] * 11, t0=t0,
                packed=packed, info=inf, jitter=jitter, rtol_eps=pivot_rtol * EPS, tier=tier)


DENSE_CLASSES = ('Z', 'Z', 'u', 'u', 's', 's', 'ell', 'ell', 'var', 'var', 'noise')


def dense_accept(case, out):
    """kron_accept's twin for zigp_test_dense_fit_update: (failures, ratios)"""
    L, f, fails, ratios = case['L'], case['L'].facts, [], {}
    exact = case['tier'] == 'exact'
    n, D = len(case['packed']), L.D
    kw = dict(lr=case['lr'], positive=case['positive'], jitter=case['jitter'], rtol_eps=case['rtol_eps'])

    def judge(name, dev, a, b, S):
        if exact:
            bits_equal_msg(name, dev, a, fails)
            return
        ok, r = rule(dev, a, b, S)
        ratios[name] = max(ratios.get(name, 0.0), r)
        if not ok:
            fails.append('%s: outside 4 err_np + 16 eps S (largest err / (eps S) = %.3g)' % (name, r))

    def structure(tag, img, H, Lraw, x):
        """relations among the device's own values, bit for bit"""
        with np.errstate(all='ignore'):
            for h in range(2):
                M, R = L.M[h], h * f['DH_LAT']
                ell = img[f['img_ell'][h]:f['img_ell'][h] + D]
                Z = img[f['img_Z'][h]:f['img_Z'][h] + M * D].reshape(M, D)
                bits_equal_msg('%s Zs == Z (KUF_C (1 / ell)) %d' % (tag, h), img[f['img_Zs'][h]:f['img_Zs'][h] + M * D], Z * (KUF_C * (1.0 / ell)), fails)
                bits_equal_msg('%s DH_ELL %d' % (tag, h), H[R + f['DH_ELL']:R + f['DH_ELL'] + D], ell, fails)
                bits_equal_msg('%s DH_INV %d' % (tag, h), H[R + f['DH_INV']:R + f['DH_INV'] + D], 1.0 / ell, fails)
                bits_equal_msg('%s DH_SCALE %d' % (tag, h), H[R + f['DH_SCALE']:R + f['DH_SCALE'] + D], KUF_C * (1.0 / ell), fails)
                bits_equal_msg('%s DH_PIVTOL %d' % (tag, h), H[R + f['DH_PIVTOL']], case['rtol_eps'] * (H[R + f['DH_VAR']] + case['jitter']), fails)
                if L.es[h] == 1:
                    bits_equal_msg('%s scalar lengthscale broadcast %d' % (tag, h), ell, np.full(D, ell[0]), fails)
                Mp = f['Mp'][h]
                for k, w in (('img_Z', D), ('img_u', 1), ('img_s', 1), ('img_Zs', D)):
                    bits_equal_msg('%s padding of %s %d' % (tag, k, h), img[f[k][h] + M * w:f[k][h] + Mp * w], np.zeros((Mp - M) * w), fails)
                for o in ('DH_INV', 'DH_ELL', 'DH_SCALE'):
                    bits_equal_msg('%s zero slots %s %d' % (tag, o, h), H[R + f[o] + D:R + f[o] + 8], np.zeros(8 - D), fails)
                if L.tri:
                    A = np.zeros((M, M))
                    A[np.tril_indices(M)] = x[L.sl(4 + h)]
                    bits_equal_msg('%s Lraw %d' % (tag, h), Lraw[h], A, fails)
                    bits_equal_msg('%s diagonal in the s slot %d' % (tag, h), img[f['img_s'][h]:f['img_s'][h] + M], np.diag(A), fails)
        if not (np.all(np.isfinite(img)) and np.all(np.isfinite(H))):
            fails.append('%s: image or H not finite' % tag)

    def images(tag, i, x_in, img0, H0):
        x_img = out['snap_x'][i]
        ia = dense_image(L, x_in if exact else x_img, case['positive'], img0, H0, case['jitter'], case['rtol_eps'], np.float64)
        ib = ia if exact else dense_image(L, x_img, case['positive'], img0, H0, case['jitter'], case['rtol_eps'], np.longdouble)
        judge('image' if not exact else tag + ' image', out['snap_img'][i], ia[0], ib[0], np.abs(ib[0]))
        judge('H' if not exact else tag + ' H', out['snap_H'][i], ia[1], ib[1], np.abs(ib[1]))
        structure(tag, out['snap_img'][i], out['snap_H'][i], None if not L.tri else [q[i] for q in out['snap_Lraw']], x_img)

    for k in 'xmv':
        bits_equal_msg('snapshot 0 ' + k, out['snap_' + k][0], case[k], fails)
    images('snapshot 0', 0, case['x'], np.zeros(f['n_img']), np.zeros(f['DH_SIZE']))
    failed = 0
    for i in range(n):
        x0, m0, v0 = out['snap_x'][i], out['snap_m'][i], out['snap_v'][i]
        x1, m1, v1 = out['snap_x'][i + 1], out['snap_m'][i + 1], out['snap_v'][i + 1]
        inf = case['info'][i]
        bad = (0, int(inf[0])) if inf[0] != 0 else ((1, int(inf[1])) if inf[1] != 0 else None)
        if failed or bad is not None:
            for k, a0, a1 in (('x', x0, x1), ('m', m0, m1), ('v', v0, v1), ('image', out['snap_img'][i], out['snap_img'][i + 1]),
                              ('H', out['snap_H'][i], out['snap_H'][i + 1])):
                bits_equal_msg('step %d (failed) leaves %s' % (i, k), a1, a0, fails)
            if not failed:
                failed = 1 + i
                if tuple(int(q) for q in out['fail'][:3]) != (1 + i, bad[0], bad[1]):
                    fails.append('fail record %r, expected %r' % (tuple(out['fail'][:3]), (1 + i, bad[0], bad[1])))
            continue
        ra = dense_step(L, x0, m0, v0, out['snap_img'][i], out['snap_H'][i], case['packed'][i], inf, case['t0'] + i + 1, trainable=case['trainable'],
                        dt=np.float64, **kw)
        rb = ra if exact else dense_step(L, x0, m0, v0, out['snap_img'][i], out['snap_H'][i], case['packed'][i], inf, case['t0'] + i + 1,
                                         trainable=case['trainable'], dt=np.longdouble, **kw)
        for b in range(11):
            sl = L.sl(b)
            if not case['trainable'][b]:
                for k, a0, a1 in (('x', x0, x1), ('m', m0, m1), ('v', v0, v1)):
                    bits_equal_msg('step %d untrainable block %d %s' % (i, b, k), a1[sl], a0[sl], fails)
                continue
            for k, a1 in (('x', x1), ('m', m1), ('v', v1)):
                judge('%s %s' % (k, DENSE_CLASSES[b]) if not exact else 'step %d block %d %s' % (i, b, k), a1[sl], ra[k][sl], rb[k][sl], rb['S_' + k][sl])
        images('step %d' % i, i + 1, ra['x'], out['snap_img'][i], out['snap_H'][i])
        bits_equal_msg('step %d history' % i, out['hist'][i], case['packed'][i][:2], fails)
        for k in 'xmv':
            if not np.all(np.isfinite(out['snap_' + k][i + 1])):
                fails.append('step %d: %s is not finite' % (i, k))
    done = failed - 1 if failed else n
    if int(out['steps_applied']) != done or int(out['rc']) != (-3 if failed else 0) or (not failed and int(out['fail'][0]) != 0):
        fails.append('rc %r, steps_applied %r, fail %r (expected %d steps)' % (out['rc'], out['steps_applied'], list(out['fail']), done))
    for k, col in (('elbo_data', 0), ('kl', 1)):
        bits_equal_msg('returned %s' % k, out[k][:done], out['hist'][:done, col], fails)
        if not np.all(np.isnan(out[k][done:])):
            fails.append('returned %s: entries from the failing step on must be NaN' % k)
    return fails, ratios


# ---- the cases of tests/test_gpu_fit_update_stages.py (the mutation tier of tests/test_cpu_fit_update_ref.py runs on exactly these)
# head grids by the number of "big" elements M0 D0 + M1 D1 + 2 M0 M1: below 256, 255 / 256 / 257, two and three workgroups with block
# boundaries inside a workgroup; 112 rows on one factor with 1 on the other; D0 < D1 and the largest D the fused path takes (7: a factor
# dimension of 8 has 17 moment columns and goes to the GEMM panels -- both fit loops refuse it, and so does the hook)
HEAD_GRIDS = [((1, 84), (3, 1), 255), ((1, 85), (1, 1), 256), ((1, 85), (2, 1), 257), ((2, 50), (3, 1), 256), ((1, 1), (1, 1), 4),
              ((15, 17), (2, 1), 557), ((16, 16), (1, 7), 640), ((32, 32), (7, 7), 2496), ((16, 112), (7, 1), 3808), ((9, 50), (1, 7), 1259),
              ((1, 112), (7, 7), 1015), ((10, 12), (1, 1), 262)]
# on/off: equal grids, and pairs whose latents differ: `mix`, `under`, `Lrmix` of tests/test_gpu_kronf_stages.py and d21-mix, d21-mix2 of
# tests/kron_nd.py (L51 there is Lrmix)
ONOFF_GRIDS = [((1, 1), (1, 1), (1, 1)), ((16, 16), (16, 16), (2, 1)), ((32, 32), (10, 12), (2, 1)), ((10, 30), (30, 10), (2, 1)),
               ((16, 112), (9, 50), (5, 1)), ((1, 112), (16, 1), (1, 7)), ((5, 7), (7, 5), (7, 7)), ((20, 9), (9, 20), (1, 7)),
               ((6, 5), (20, 20), (2, 1)), ((1, 3), (8, 13), (1, 2)), ((1, 7), (11, 9), (1, 2)), ((1, 3), (6, 17), (1, 2))]      # the last three: 255, 256, 257


def _kron_cases():
    out = {}
    for j, (g, D, big) in enumerate(HEAD_GRIDS):
        for lik in ('gaussian', 'bernoulli'):
            tr = [1] * 10
            if lik == 'gaussian':
                tr[9] = 0                      # no f_mu
                if j % 2:
                    tr[4] = 0                  # a fixed lengthscale block
            else:
                tr[8] = 0                      # the classifier has no noise
                if j % 2:
                    tr[5] = tr[6] = 0
            out['%s-%dx%d-d%d%d' % (lik[:5], g[0], g[1], D[0], D[1])] = dict(lik=lik, shape=dict(M0f=g[0], M1f=g[1], D0=D[0], D1=D[1]),
                                                                           trainable=tr, ranks=float((1, 2, 0)[j % 3]), big=big, t0=(0, 37, 10 ** 6)[j % 3])
    for j, (gf, gg, D) in enumerate(ONOFF_GRIDS):
        out['onoff-%dx%d-%dx%d-d%d%d' % (gf + gg + D)] = dict(lik='onoff', shape=dict(M0f=gf[0], M1f=gf[1], M0g=gg[0], M1g=gg[1], D0=D[0], D1=D[1]),
                                                            trainable=None, ranks=float((1, 0, 2)[j % 3]), t0=(5, 0, 10 ** 6)[j % 3],
                                                            big=sum(m0 * D[0] + m1 * D[1] + 2 * m0 * m1 for m0, m1 in (gf, gg)))
    return out


KRON_CASES = _kron_cases()


def kron_fixture(name, tier, facts=None, info=None, n_steps=3):
    k = KRON_CASES[name]
    return kron_case(k['shape'], k['lik'], tier, n_steps=n_steps, t0=k['t0'], ranks=k['ranks'], trainable=k['trainable'], info=info,
                     seed=sorted(KRON_CASES).index(name), facts=facts)


# dense: M = (17, 5), (5, 17), (16, 16), (33, 1); D in {1, 3, 8}; ell_size 1 and D mixed between the latents; an untrainable block in most
# cases; and per mode three shapes whose n_free is 255 / 256 or 512 / 257 (modes 0 and 1 have no shape with n_free = 256 at these D)
DENSE_SHAPES = [((17, 5), 3, (1, 3), (7,)), ((5, 17), 8, (8, 1), (0, 8)), ((16, 16), 1, (1, 1), (5,)), ((33, 1), 8, (8, 8), ()),
                ((17, 5), 8, (1, 8), (10,))]
DENSE_BOUNDARY = {0: [((2, 48), 3, (1, 1), ()), ((43, 58), 3, (1, 3), (6,)), ((25, 59), 1, (1, 1), (3,))],
                  2: [((9, 17), 1, (1, 1), ()), ((4, 17), 3, (3, 3), (6,)), ((12, 15), 1, (1, 1), (2,))]}
DENSE_BOUNDARY[1] = DENSE_BOUNDARY[0]
DENSE_NFREE = {0: (255, 512, 257), 1: (255, 512, 257), 2: (255, 256, 257)}
DENSE_CASES = {'m%d-%dx%d-d%d-e%d%d' % (mode, M[0], M[1], D, es[0], es[1]): dict(mode=mode, shape=dict(Mf=M[0], Mg=M[1], D=D), ell_size=es,
                                                                              trainable=[0 if b in fixed else 1 for b in range(11)])
               for mode in (0, 1, 2) for (M, D, es, fixed) in DENSE_SHAPES + DENSE_BOUNDARY[mode]}


def dense_fixture(name, tier, facts=None, info=None, n_steps=3):
    k = DENSE_CASES[name]
    return dense_case(k['mode'], k['shape'], k['ell_size'], tier, n_steps=n_steps, t0=(0, 37, 10 ** 6)[sorted(DENSE_CASES).index(name) % 3],
                      trainable=k['trainable'], info=info, seed=sorted(DENSE_CASES).index(name), facts=facts)
