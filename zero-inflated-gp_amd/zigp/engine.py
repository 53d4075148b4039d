"""Host-side engine objects over the C-ABI (one context per GPU).

DenseEngine drives the dense (OnOffSVGP) path: data is made resident in HBM once (`set_data`), then every
`elbo` call is one ELBO value (+ gradient) = one optimiser step of the reference
(GPflow Model.optimize function evaluation / sess.run(train_op), scripts/onoff.py:379).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ZigpError, NotPositiveDefiniteError, as_f64, ptr

PARAM_KEYS = ('Zf', 'Zg', 'u_fm', 'u_gm', 'u_fs_sqrt', 'u_gs_sqrt', 'ell_f', 'ell_g', 'var_f', 'var_g', 'noise')


def _check(lib, ctx, rc):
    if rc == 0:
        return
    msg = lib.zigp_last_error(ctx)
    msg = msg.decode() if msg else 'unknown error'
    if rc == _lib.ZIGP_ENOTPD:
        raise NotPositiveDefiniteError(msg)
    if rc == _lib.ZIGP_EARG:
        raise ValueError(msg)
    raise ZigpError('libzigp error %d: %s' % (rc, msg))


def kernel_kinds(p, D=None):
    """(kind of f, kind of g) from p.get('kern_f', 'rbf') / p.get('kern_g', 'rbf') -- 'rbf', 'matern32' or 'matern52' (_lib.KERNELS).
    ValueError, before any device work, for an unknown name and for a Matern latent at D > 8."""
    kinds = []
    for tag in 'fg':
        name = p.get('kern_' + tag, 'rbf')
        if not isinstance(name, str) or name.lower() not in _lib.KERNELS:
            raise ValueError("kern_%s = %r: the dense path knows the kernels 'rbf', 'matern32' and 'matern52'" % (tag, name))
        kinds.append(_lib.KERNELS[name.lower()])
        if D is not None and kinds[-1] != _lib.KERN_RBF and D > _lib.MATERN_MAX_D:
            raise ValueError('kern_%s = %r and D = %d: the Matern kernels cover D in [1, %d] (the wide kernels are RBF only)'
                             % (tag, name, D, _lib.MATERN_MAX_D))
    return tuple(kinds)


def kron_kernel_kinds(p, tags=('f', 'g')):
    """{tag: (kind of factor 0, kind of factor 1)} of a Kronecker parameter dict: p.get('kern_f', 'rbf') / p.get('kern_g', 'rbf') is a
    name ('rbf', 'matern32', 'matern52': both factors) or a pair (kind0, kind1) of names.  ValueError, before any device work, for
    anything else."""
    out = {}
    for tag in tags:
        v = p.get('kern_' + tag, 'rbf')
        pair = (v, v) if isinstance(v, str) else tuple(v) if isinstance(v, (tuple, list)) else None
        if pair is None or len(pair) != 2 or not all(isinstance(n, str) and n.lower() in _lib.KERNELS for n in pair):
            raise ValueError("kern_%s = %r: a Kronecker latent takes 'rbf', 'matern32' or 'matern52', or a pair (kind0, kind1) of them, "
                             "one per factor" % (tag, v))
        out[tag] = (_lib.KERNELS[pair[0].lower()], _lib.KERNELS[pair[1].lower()])
    return out


def kron_matern_factor(kinds):
    """'<Kernel> kernel on factor <q> of latent <tag>' of the first Matern factor of kron_kernel_kinds' result, or None -- the naming
    of the library's own refusals (zigp_kron_fit_steps)"""
    names = {_lib.KERN_MATERN32: 'Matern32', _lib.KERN_MATERN52: 'Matern52'}
    for tag in ('f', 'g'):
        for q, k in enumerate(kinds.get(tag, ())):
            if k in names:
                return '%s kernel on factor %d of latent %s' % (names[k], q, tag)
    return None


class _Packed:
    """Keeps the numpy arrays behind a zigp_params struct alive."""

    def __init__(self, p):
        Zf, Zg = as_f64(p['Zf']), as_f64(p['Zg'])
        if Zf.ndim != 2 or Zg.ndim != 2 or Zf.shape[1] != Zg.shape[1]:
            raise ValueError('Zf and Zg must be (M,D) with equal D')
        D = Zf.shape[1]
        if not 1 <= D <= _lib.MAX_D:
            raise ValueError('D = %d: the dense path takes input dimensions 1 .. %d (ZIGP_MAX_D)' % (D, _lib.MAX_D))
        self.D, self.Mf, self.Mg = D, Zf.shape[0], Zg.shape[0]
        self.kinds = kernel_kinds(p, D)     # p['kern_f'] / p['kern_g']: the kernel family of each latent (zigp_set_kernel)

        def ell(v):
            v = as_f64(v).reshape(-1)
            if v.size == 1:
                v = np.full(D, float(v[0]))
            if v.size != D:
                raise ValueError('lengthscales must be scalar or have D entries')
            return np.ascontiguousarray(v)

        # p['q_diag'] = False: full-covariance q(u) on the whitened model (zigp_set_q_full); u_*s_sqrt is then the (M, M) or (M, M, 1)
        # factor, of which the library reads the lower triangle
        self.q_full = not p.get('q_diag', True)
        if self.q_full and not p.get('whiten', False):
            raise ValueError('q_diag=False needs whiten=True: the full-covariance q(u) exists for the whitened model only')

        def q_sqrt(k, M):
            a = as_f64(p[k])
            if not self.q_full:
                return a.reshape(-1)
            if a.shape not in ((M, M), (M, M, 1)):
                raise ValueError('%s must be (%d, %d) or (%d, %d, 1) with q_diag=False, not %s' % (k, M, M, M, M, a.shape))
            a = a.reshape(M, M)
            if not np.all(np.diagonal(a) != 0):
                raise ValueError('%s has a zero diagonal entry (q_diag=False)' % k)
            return a

        self.arr = dict(Zf=Zf, Zg=Zg, u_fm=as_f64(p['u_fm']).reshape(-1), u_gm=as_f64(p['u_gm']).reshape(-1),
                        u_fs_sqrt=q_sqrt('u_fs_sqrt', self.Mf), u_gs_sqrt=q_sqrt('u_gs_sqrt', self.Mg),
                        ell_f=ell(p['ell_f']), ell_g=ell(p['ell_g']))
        for k, M in (('u_fm', self.Mf), ('u_fs_sqrt', self.Mf), ('u_gm', self.Mg), ('u_gs_sqrt', self.Mg)):
            if self.arr[k].size != (M * M if self.q_full and k.endswith('s_sqrt') else M):
                raise ValueError('%s must have %d entries' % (k, M))
        s = _lib.zigp_params()
        s.Mf, s.Mg, s.D = self.Mf, self.Mg, D
        for k, a in self.arr.items():
            setattr(s, k, ptr(a))
        s.var_f, s.var_g, s.noise = float(np.squeeze(p['var_f'])), float(np.squeeze(p['var_g'])), float(np.squeeze(p['noise']))
        self.struct = s


HEAD_PARAM_KEYS = ('Zf', 'u_fm', 'u_fs_sqrt', 'ell_f', 'var_f', 'noise')     # what head_elbo reads of p, and the keys of its gradient


def head_placeholder(D, q_full=False):
    """The g fields of the placeholder latent a head call on the dense path runs beside latent f (include/zigp.h "heads on the dense
    path"): one inducing point at the origin, u = 0, s = 1 (q_full: the (1, 1) factor [1]), ell = 1 and var = 1 in every dimension, RBF.
    elbo / predict on dict(p, **head_placeholder(D)) enqueue the very launches head_elbo / head_predict do, point-wise stage apart."""
    return dict(Zg=np.zeros((1, int(D))), u_gm=np.zeros(1), u_gs_sqrt=np.ones((1, 1)) if q_full else np.ones(1), ell_g=np.ones(int(D)),
                var_g=1.0, kern_g='rbf')


def _scalar(v):
    """float of a Python number or a size-1 array (np.squeeze on a plain float costs 1.5 us)"""
    return float(v) if isinstance(v, (float, int)) else float(np.asarray(v).reshape(-1)[0])


class KronStepper:
    """see DenseEngine.kron_stepper"""
    _ARR = (('Z', 0), ('Z', 1), ('ell_', 0), ('ell_', 1))

    def __init__(self, engine, p):
        self.eng = engine
        s, keep, dims = engine._pack_kron(p)            # private copies below: the caller's arrays may be views that change or go away
        self.dims = dims
        self.kinds = kron_kernel_kinds(p)               # the factor kinds belong to the model shape: fixed here, set before every step
        self.par = {}
        self.s = _lib.zigp_kron_params()
        self.gs = _lib.zigp_kron_grads()
        sizes = []
        for tag in ('f', 'g'):
            Z0, Z1, l0, l1, um, us = keep[tag]
            self.par[tag] = [np.array(a, dtype=np.float64, order='C', copy=True) for a in (Z0, Z1, l0, l1, um, us)]
            sizes += [a.size for a in self.par[tag]]
        self.flat = np.zeros(sum(sizes))
        self.out = {}
        o = 0
        for tag in ('f', 'g'):
            Z0, Z1, l0, l1, um, us = self.par[tag]
            setattr(self.s, 'M0' + tag, Z0.shape[0]); setattr(self.s, 'M1' + tag, Z1.shape[0])
            for name, a in (('Z0', Z0), ('Z1', Z1), ('ell0', l0), ('ell1', l1)):
                setattr(self.s, name + tag, ptr(a))
            setattr(self.s, 'u_%sm' % tag, ptr(um)); setattr(self.s, 'u_%ss_sqrt' % tag, ptr(us))
            views = []
            for a in self.par[tag]:
                views.append(self.flat[o:o + a.size].reshape(a.shape)); o += a.size
            for name, v in zip(('Z0', 'Z1', 'ell0', 'ell1'), views[:4]):
                setattr(self.gs, name + tag, ptr(v))
            setattr(self.gs, 'u_%sm' % tag, ptr(views[4])); setattr(self.gs, 'u_%ss_sqrt' % tag, ptr(views[5]))
            self.out['Z' + tag] = [views[0], views[1]]
            self.out['ell_' + tag] = [views[2], views[3]]
            self.out['u_%sm' % tag] = views[4]
            self.out['u_%ss_sqrt' % tag] = views[5]
        self.s.D0, self.s.D1 = dims
        self._ed, self._kl, self._dmu = C.c_double(0), C.c_double(0), C.c_double(0)
        self._sref, self._gref = C.byref(self.s), C.byref(self.gs)
        self._edref, self._klref, self._dmuref = C.byref(self._ed), C.byref(self._kl), C.byref(self._dmu)

    def __call__(self, p, X=None, Y=None, rows=None, jitter=1e-5, scale=1.0, g_offset=0.0, include_kl=True, f_mu=None):
        s, copyto = self.s, np.copyto
        for tag in ('f', 'g'):
            b = self.par[tag]
            Z, ell, var = p['Z' + tag], p['ell_' + tag], p['var_' + tag]
            copyto(b[0], Z[0]); copyto(b[1], Z[1])
            copyto(b[2], np.reshape(ell[0], -1)); copyto(b[3], np.reshape(ell[1], -1))      # a scalar lengthscale broadcasts over the factor's columns
            copyto(b[4], np.reshape(p['u_%sm' % tag], -1)); copyto(b[5], np.reshape(p['u_%ss_sqrt' % tag], -1))
            setattr(s, 'var0' + tag, _scalar(var[0])); setattr(s, 'var1' + tag, _scalar(var[1]))
        s.noise = _scalar(p.get('noise', 1.0))
        fmu = 0.0 if f_mu is None else _scalar(f_mu)
        eng = self.eng
        eng._apply_kron_kinds(self.kinds)
        if rows is None:
            X = as_f64(X)
            Y = as_f64(Y).reshape(-1)
            if X.ndim != 2 or X.shape[1] != self.dims[0] + self.dims[1] or Y.size != X.shape[0]:
                raise ValueError('X must be (N,%d) and Y have N entries' % (self.dims[0] + self.dims[1]))
            rc = eng.lib.zigp_kron_elbo(eng.ctx, self._sref, ptr(X), ptr(Y), X.shape[0], float(jitter), float(scale), float(g_offset), fmu,
                                        1 if include_kl else 0, self._edref, self._klref, self._gref, self._dmuref)
        else:
            rc = eng.lib.zigp_kron_elbo_rows(eng.ctx, self._sref, int(rows[0]), int(rows[1]), float(jitter), float(scale), float(g_offset), fmu,
                                             1 if include_kl else 0, self._edref, self._klref, self._gref, self._dmuref)
        _check(eng.lib, eng.ctx, rc)
        gs, out = self.gs, self.out
        out['noise'] = gs.noise
        out['var_f'] = [gs.var0f, gs.var1f]
        out['var_g'] = [gs.var0g, gs.var1g]
        if f_mu is not None:
            out['f_mu'] = self._dmu.value
        else:
            out.pop('f_mu', None)
        return self._ed.value, self._kl.value, out


class DenseEngine:
    def __init__(self, device=0, pivot_rtol=None):
        """pivot_rtol: smallest accepted Cholesky pivot as a multiple of eps * (variance + jitter).  None keeps the library default
        (8: an exactly singular Kuu is reported whichever way its rounding-noise pivot falls); 0 is tf.cholesky's bare `pivot > 0` test
        (onofftf/main.py:200,268,355) -- what the reference look-alikes use: reference_engine() below."""
        self.lib = _lib.load()
        self.ctx = C.c_void_p()
        rc = self.lib.zigp_create(C.byref(self.ctx), int(device))
        if rc != 0:
            raise ZigpError('zigp_create failed (rc=%d): no usable HIP device %d' % (rc, device))
        self.device = int(device)
        self.N = 0
        self._full_N = 0
        self.D = 0
        self._keep = None
        if pivot_rtol is not None:
            self.set_pivot_rtol(pivot_rtol)

    def close(self):
        if self.ctx:
            self.lib.zigp_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_chunk(self, rows):
        """rows per pass (a multiple of 1024); None or 0: the library's automatic rule (see get_chunk_rows)"""
        _check(self.lib, self.ctx, self.lib.zigp_set_chunk(self.ctx, int(rows or 0)))

    def get_chunk(self, M):
        """rows per pass of the dense path at M inducing points per latent (the set_chunk value, else the library's rule)"""
        r = int(self.lib.zigp_get_chunk(self.ctx, int(M)))
        if r < 0:
            raise ValueError('zigp_get_chunk: bad M')
        return r

    def get_chunk_rows(self, M, span):
        """rows per pass the dense path uses for a row range of `span` rows at M inducing points per latent (equal passes; short ranges
        go through in one pass while the panels stay within 9 GB)"""
        r = int(self.lib.zigp_get_chunk_rows(self.ctx, int(M), int(span)))
        if r < 0:
            raise ValueError('zigp_get_chunk_rows: bad M or span')
        return r

    def set_pivot_rtol(self, rtol):
        """smallest accepted Cholesky pivot = rtol * eps * (variance + jitter); default 8, 0 = tf.cholesky's bare pivot > 0 test"""
        _check(self.lib, self.ctx, self.lib.zigp_set_pivot_rtol(self.ctx, float(rtol)))

    # ---- data-parallel exchange inside the library (RCCL; include/zigp.h 'data-parallel exchange') ----
    def comm_unique_id(self):
        """rank 0: the 128-byte id every rank hands to comm_init"""
        buf = (C.c_char * _lib.COMM_ID_BYTES)()
        rc = self.lib.zigp_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise ZigpError('zigp_comm_unique_id failed (rc=%d): librccl.so.1 not loadable?' % rc)
        return bytes(buf.raw)

    def comm_init(self, rank, nranks, unique_id):
        """collective; afterwards elbo() / kron_elbo() / kron_head_elbo() return sums over ranks (pass include_kl on rank 0 only)"""
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError('unique_id must have %d bytes' % _lib.COMM_ID_BYTES)
        buf = C.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        _check(self.lib, self.ctx, self.lib.zigp_comm_init(self.ctx, int(rank), int(nranks), C.cast(buf, C.c_void_p)))

    def comm_available(self):
        """True when RCCL can be bound in this process (zigp_comm_available): ranks agree on this before any of them enters comm_init"""
        v = C.c_int32(0)
        return self.lib.zigp_comm_available(C.byref(v)) == 0

    def comm_set_timeout(self, seconds):
        """how long comm_init waits for its peers before it gives up with a ZigpError (default 120 s)"""
        _check(self.lib, self.ctx, self.lib.zigp_comm_set_timeout(self.ctx, float(seconds)))

    def comm_destroy(self):
        _check(self.lib, self.ctx, self.lib.zigp_comm_destroy(self.ctx))

    def comm_allreduce(self, vec):
        """sum a small float64 host vector over the ranks of the library's communicator (returns a new array)"""
        v = np.array(vec, dtype=np.float64).reshape(-1)
        _check(self.lib, self.ctx, self.lib.zigp_comm_allreduce_host(self.ctx, ptr(v), v.size))
        return v

    def comm_info(self):
        r, n, k = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _check(self.lib, self.ctx, self.lib.zigp_comm_info(self.ctx, C.byref(r), C.byref(n), C.byref(k)))
        return dict(rank=r.value, nranks=n.value, allreduce_calls=k.value)

    def set_data(self, X, Y):
        X = as_f64(X)
        if X.ndim != 2:
            raise ValueError('X must be (N,D)')
        Y = as_f64(Y).reshape(-1)
        if Y.size != X.shape[0]:
            raise ValueError('Y must have N entries')
        _check(self.lib, self.ctx, self.lib.zigp_set_data(self.ctx, ptr(X), ptr(Y), X.shape[0], X.shape[1]))
        self.N, self.D = X.shape
        self._full_N = self.N

    def set_data_device(self, X_t, Y_t):
        """Adopt torch CUDA float64 tensors (no copy); they are kept alive by this object."""
        import torch
        N, D = X_t.shape
        if not (X_t.is_cuda and Y_t.is_cuda and X_t.device.index == self.device and Y_t.device.index == self.device):
            raise ValueError('set_data_device: tensors must live on cuda:%d, the engine\'s device' % self.device)
        if not (X_t.is_contiguous() and Y_t.is_contiguous() and X_t.dtype == torch.float64 and Y_t.dtype == torch.float64):
            raise ValueError('set_data_device: need contiguous float64 tensors')
        if Y_t.numel() != N:
            raise ValueError('Y must have N entries')
        # the engine's streams are non-blocking: nothing orders them after the torch stream that produced the tensors
        torch.cuda.current_stream(self.device).synchronize()
        self._keep = (X_t, Y_t)
        _check(self.lib, self.ctx, self.lib.zigp_set_data_device(self.ctx, C.c_void_p(X_t.data_ptr()), C.c_void_p(Y_t.data_ptr()), N, D))
        self.N, self.D = N, D
        self._full_N = N

    def select_rows(self, idx=None):
        """Minibatch by row indices (repeats allowed): the rows `idx` of the resident data set are gathered on the device and become
        the active data of the calls that follow (rows 0 .. len(idx)); None / empty: back to the whole resident set."""
        if idx is None or len(idx) == 0:
            _check(self.lib, self.ctx, self.lib.zigp_select_rows(self.ctx, None, 0))
            self.N = self._full_N
            return
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
        _check(self.lib, self.ctx, self.lib.zigp_select_rows(self.ctx, idx.ctypes.data, idx.size))
        self.N = int(idx.size)

    def set_whiten(self, on):
        """Whitened parametrisation of the dense path (zigp_set_whiten; the reference's `whiten` switch, onoffgpf/OnOffSVGP.py:88-91,
        133,137): u_*m / u_*s_sqrt are then the whitened mean and standard deviation, q(u) = N(L u_m, L diag(u_s_sqrt^2) L^T).  elbo,
        predict, predict_device and prior_kl set it themselves on every call from p.get('whiten', False) -- like the mean function -- so
        an engine shared between models does not carry the mode from one caller to the next."""
        _check(self.lib, self.ctx, self.lib.zigp_set_whiten(self.ctx, 1 if on else 0))

    def get_whiten(self):
        return bool(self.lib.zigp_get_whiten(self.ctx))

    def set_q_full(self, on):
        """Full-covariance q(u) of the whitened dense model (zigp_set_q_full; the reference's `q_diag = False`, onoffgpf/OnOffSVGP.py:
        59-71, 88-104): u_*s_sqrt are then (M, M) lower-triangular factors Lq, q(u) = N(L u_m, L Lq Lq^T L^T).  Set on every call from
        p.get('q_diag', True), like the whitening."""
        _check(self.lib, self.ctx, self.lib.zigp_set_q_full(self.ctx, 1 if on else 0))

    def get_q_full(self):
        return bool(self.lib.zigp_get_q_full(self.ctx))

    def set_kernel(self, latent, name):
        """Kernel family of a dense latent (zigp_set_kernel; the kernel object handed to the reference model, onoffgpf/OnOffSVGP.py:22):
        latent 'f' / 0 or 'g' / 1; name 'rbf', 'matern32' or 'matern52' (GPflow 0.4.0 kernels.RBF / Matern32 / Matern52).  elbo, predict,
        predict_device and prior_kl set both from p.get('kern_f', 'rbf') / p.get('kern_g', 'rbf') on every call, like the whitening."""
        if not isinstance(name, str) or name.lower() not in _lib.KERNELS:
            raise ValueError("kernel %r: the dense path knows 'rbf', 'matern32' and 'matern52'" % (name,))
        _check(self.lib, self.ctx, self.lib.zigp_set_kernel(self.ctx, {'f': 0, 'g': 1}.get(latent, latent), _lib.KERNELS[name.lower()]))

    def get_kernel(self, latent):
        k = self.lib.zigp_get_kernel(self.ctx, {'f': 0, 'g': 1}.get(latent, latent))
        if k < 0:
            raise ValueError('zigp_get_kernel: latent must be f / 0 or g / 1')
        return {v: n for n, v in _lib.KERNELS.items()}[k]

    def set_kron_kernel(self, latent, factor, name):
        """Kernel family of one factor of a Kronecker latent (zigp_set_kron_kernel): latent 'f' / 0 or 'g' / 1, factor 0 or 1, name 'rbf',
        'matern32' or 'matern52'.  Every kron_* call sets all four from p.get('kern_f', 'rbf') / p.get('kern_g', 'rbf') first, so a
        setting made here lasts until the next such call."""
        if not isinstance(name, str) or name.lower() not in _lib.KERNELS:
            raise ValueError("kernel %r: the Kronecker factors know 'rbf', 'matern32' and 'matern52'" % (name,))
        self._kron_kinds_set = None
        _check(self.lib, self.ctx, self.lib.zigp_set_kron_kernel(self.ctx, {'f': 0, 'g': 1}.get(latent, latent), int(factor),
                                                                  _lib.KERNELS[name.lower()]))

    def get_kron_kernel(self, latent, factor):
        k = self.lib.zigp_get_kron_kernel(self.ctx, {'f': 0, 'g': 1}.get(latent, latent), int(factor))
        if k < 0:
            raise ValueError('zigp_get_kron_kernel: latent must be f / 0 or g / 1, factor 0 or 1')
        return {v: n for n, v in _lib.KERNELS.items()}[k]

    _kron_kinds_set = None      # the four kinds as this engine last set them (None: unknown), so a training loop sets them once

    def _apply_kron_kinds(self, kinds):
        """All four factor kinds of the context from kron_kernel_kinds' result (a latent that is absent: RBF) -- before every kron_* call,
        so that a previous call's kinds never leak into this one."""
        want = kinds.get('f', (0, 0)) + kinds.get('g', (0, 0))
        if want == self._kron_kinds_set:
            return
        self._kron_kinds_set = None
        for i, k in enumerate(want):
            _check(self.lib, self.ctx, self.lib.zigp_set_kron_kernel(self.ctx, i >> 1, i & 1, int(k)))
        self._kron_kinds_set = want

    def _set_kron_kinds(self, p, tags=('f', 'g')):
        self._apply_kron_kinds(kron_kernel_kinds(p, tags))

    # what set_kron_matern_fused last set.  The fit loops refuse a Matern factor BEFORE the library is touched (an engine without a library
    # shows it: tests/test_cpu_kron_matern.py), so that refusal cannot ask the context; get_kron_matern_fused does.
    _kron_matern_fused = False

    def set_kron_matern_fused(self, on=True):
        """Opt in to the fused Kronecker kernels for Matern factors (zigp_set_kron_matern_fused; off by default): with it on, a kron_* call
        with a Matern factor on a grid the fused kernels cover runs their Matern instantiations instead of the GEMM panels, and
        kron_fit_steps / kron_head_fit_steps accept Matern factors.  set_kron_panels(True) still wins."""
        if on not in (True, False, 0, 1):
            raise ValueError('set_kron_matern_fused: on must be True or False')
        _check(self.lib, self.ctx, self.lib.zigp_set_kron_matern_fused(self.ctx, 1 if on else 0))
        self._kron_matern_fused = bool(on)

    def get_kron_matern_fused(self):
        return bool(self.lib.zigp_get_kron_matern_fused(self.ctx))

    def _kron_fit_kinds(self, who, shape, tags):
        """The device fit loops fit RBF factors unless set_kron_matern_fused is on: a Matern factor in shape then raises before the
        library is touched, with the naming of the library's own refusal.  Otherwise the context gets the kinds of shape (all RBF with
        the switch off)."""
        kinds = kron_kernel_kinds(shape, tags)
        bad = kron_matern_factor(kinds)
        if bad and not self._kron_matern_fused:
            raise ValueError('%s: a %s is set; the device loop fits RBF factors only: step the model with kron_%selbo(rows=...) and a host '
                             'optimiser' % (who, bad, 'head_' if tags == ('f',) else ''))
        self._apply_kron_kinds(kinds if bad else {})

    def _set_modes(self, p):
        kinds = kernel_kinds(p)          # an unknown name raises before anything is set
        self.set_whiten(p.get('whiten', False))
        self.set_q_full(not p.get('q_diag', True))
        for h in (0, 1):
            _check(self.lib, self.ctx, self.lib.zigp_set_kernel(self.ctx, h, kinds[h]))

    def elbo(self, p, jitter=1e-6, scale=1.0, g_offset=0.0, rows=None, include_kl=True, need_grad=True):
        """Returns (elbo_data, kl, grads or None); ELBO = elbo_data - kl.  p['whiten'] = True: the whitened parametrisation (set_whiten);
        with it, p['q_diag'] = False: full-covariance q(u) (set_q_full) -- u_*s_sqrt (M, M) or (M, M, 1), their gradients (M, M)."""
        pk = _Packed(p)
        self._set_modes(p)
        mean_D = self._set_mean_function(p, pk.D)
        r0, r1 = (0, self.N) if rows is None else rows
        ed, kl = C.c_double(0), C.c_double(0)
        gs, g = None, None
        if need_grad:
            g = dict(Zf=np.zeros((pk.Mf, pk.D)), Zg=np.zeros((pk.Mg, pk.D)), u_fm=np.zeros(pk.Mf), u_gm=np.zeros(pk.Mg),
                     u_fs_sqrt=np.zeros((pk.Mf, pk.Mf) if pk.q_full else pk.Mf), u_gs_sqrt=np.zeros((pk.Mg, pk.Mg) if pk.q_full else pk.Mg),
                     ell_f=np.zeros(pk.D), ell_g=np.zeros(pk.D))
            gs = _lib.zigp_grads()
            for k, a in g.items():
                setattr(gs, k, ptr(a))
        rc = self.lib.zigp_elbo(self.ctx, C.byref(pk.struct), float(jitter), float(scale), float(g_offset), int(r0), int(r1),
                                1 if include_kl else 0, C.byref(ed), C.byref(kl), C.byref(gs) if gs is not None else None)
        _check(self.lib, self.ctx, rc)
        if need_grad:
            g['var_f'], g['var_g'], g['noise'] = gs.var_f, gs.var_g, gs.noise
            if mean_D is not None:
                da, db = np.zeros(max(mean_D, 1)), C.c_double(0)
                _check(self.lib, self.ctx, self.lib.zigp_get_mean_function_grad(self.ctx, ptr(da), mean_D, C.byref(db)))
                g['mean_a'], g['mean_b'] = da[:mean_D], db.value
        return ed.value, kl.value, g

    def fit_steps(self, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6, scale=1.0,
                  beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        """n_steps Adam iterations of the dense on/off fit ON THE DEVICE (zigp_fit_steps; a minibatch step of OnOffSVGP, onoffgpf/
        OnOffSVGP.py:42-47,107-122, and its Adam update): one synchronisation for the whole call.
        shape: dict(Mf, Mg, D); x, m, v: float64 [n_free] free state and Adam moments, UPDATED IN PLACE, in the block order PARAM_KEYS
        (include/zigp.h); lr, positive, trainable: 11 per-block learning rates / Log1pe flags / trainable flags; ell_size = (f, g): 1 (one
        lengthscale for all columns) or D; t0: iterations done so far; rows: int64 [n_steps * batch] indices into the resident data set,
        step i uses rows[i * batch : (i + 1) * batch] -- None: every step uses the active rows (full-batch Adam).
        Returns (elbo_data[n_steps], kl[n_steps]) -- the history, each at the parameters before that step's update.
        shape['whiten'] = True or shape['q_diag'] = False raises ValueError: the device loop fits the diagonal unwhitened parametrisation only."""
        self._set_modes(shape)     # the library refuses the call while either mode is on (ZIGP_EARG; the message names q_diag / whitening)
        return self._fit_call(None, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows, batch, jitter, scale, beta1, beta2, eps,
                              include_kl)

    def fit_steps_mode(self, mode, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows=None, batch=0, jitter=1e-6, scale=1.0,
                       beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        """fit_steps for the parametrisation `mode` names (zigp_fit_steps_mode): _lib.FIT_DIAG (what fit_steps fits, bit for bit),
        _lib.FIT_WHITE (the whitened model, the same 11 blocks) or _lib.FIT_WHITE_FULL (full-covariance q(u): blocks 4 and 5 of x / m / v
        hold the M (M + 1) / 2 lower-triangle entries of the factors in row-major order, transforms.LowerTriangular's free vector, and
        positive[4], positive[5] must be False).  The mode belongs to the call: the engine's set_whiten / set_q_full settings are neither
        read nor changed, and shape's 'whiten' / 'q_diag' entries are ignored.  Arguments, return value, exceptions and what a
        NotPositiveDefiniteError carries (steps_applied, the elbo_data / kl prefix) are those of fit_steps."""
        return self._fit_call(int(mode), shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows, batch, jitter, scale, beta1, beta2,
                              eps, include_kl)

    def _fit_call(self, mode, shape, x, m, v, lr, positive, trainable, ell_size, t0, n_steps, rows, batch, jitter, scale, beta1, beta2, eps,
                  include_kl):
        """mode None: zigp_fit_steps; otherwise zigp_fit_steps_mode"""
        for tag, kind in zip('fg', kernel_kinds(shape)):      # the device loops fit RBF latents (the library refuses too: ZIGP_EARG)
            if kind != _lib.KERN_RBF:
                raise ValueError('kern_%s = %r: the device fit loops fit RBF latents only; a Matern model is fitted by elbo + a host '
                                 'optimiser (OnOffSVGP.optimize runs its host loop)' % (tag, shape['kern_' + tag]))
        for h in (0, 1):      # both RBF here; not left to whatever model used the engine before
            _check(self.lib, self.ctx, self.lib.zigp_set_kernel(self.ctx, h, _lib.KERN_RBF))
        s = _lib.zigp_params()
        s.Mf, s.Mg, s.D = int(shape['Mf']), int(shape['Mg']), int(shape['D'])
        o = _lib.zigp_fit_opts()
        for b in range(_lib.DENSE_FIT_BLOCKS):
            o.lr[b] = float(lr[b]); o.positive[b] = int(bool(positive[b])); o.trainable[b] = int(bool(trainable[b]))
        o.ell_size_f, o.ell_size_g = int(ell_size[0]), int(ell_size[1])
        o.beta1, o.beta2, o.eps = float(beta1), float(beta2), float(eps)
        for a in (x, m, v):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 1 and a.size == x.size):
                raise ValueError('x, m, v must be contiguous float64 vectors of one length')
        n = int(n_steps)
        rp = None
        if rows is not None:
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64)).reshape(-1)
            if int(batch) <= 0 or rows.size != n * int(batch):
                raise ValueError('rows must hold n_steps * batch indices')
            rp = rows.ctypes.data
        ed, kl = np.zeros(max(n, 0)), np.zeros(max(n, 0))
        tail = (C.byref(s), C.byref(o), ptr(x), ptr(m), ptr(v), x.size, int(t0), n, rp, int(batch), float(jitter), float(scale),
                1 if include_kl else 0, ptr(ed), ptr(kl))
        rc = self.lib.zigp_fit_steps(self.ctx, *tail) if mode is None else self.lib.zigp_fit_steps_mode(self.ctx, mode, *tail)
        try:
            _check(self.lib, self.ctx, rc)
        except ZigpError as e:
            # as kron_fit_steps: x / m / v hold the state after the updates that WERE applied; the count comes from the library
            done = max(0, min(n, int(self.lib.zigp_fit_steps_applied(self.ctx))))
            e.steps_applied = done
            e.elbo_data, e.kl = ed[:done].copy(), kl[:done].copy()
            raise
        return ed, kl

    def _set_mean_function(self, p, D):
        """p may carry the mean function of f, m(x) = mean_b + mean_a . x (OnOffSVGP.py:29,134): 'mean_b' alone is GPflow's
        Constant, 'mean_a' (+ 'mean_b') its Linear; neither is Zero.  Returns len(mean_a) when one is set, else None."""
        a, b = p.get('mean_a'), p.get('mean_b')
        if a is None and b is None:
            _check(self.lib, self.ctx, self.lib.zigp_set_mean_function(self.ctx, None, -1, 0.0))
            return None
        a = np.zeros(0) if a is None else as_f64(a).reshape(-1)
        if a.size not in (0, D):
            raise ValueError('mean_a must have D entries')
        _check(self.lib, self.ctx, self.lib.zigp_set_mean_function(self.ctx, ptr(a) if a.size else None, a.size,
                                                                    float(np.squeeze(0.0 if b is None else b))))
        return a.size

    # ---- what the predict-like calls share: predict, density, scores, sample paths ----
    def _prepare(self, p, pk=None):
        """the packed parameters of p (pk when the caller has packed them already), with the mean function and the modes set from p"""
        pk = _Packed(p) if pk is None else pk
        self._set_mean_function(p, pk.D)
        self._set_modes(p)
        return pk

    def _device_f64(self, t):
        """True for a contiguous float64 tensor on the engine's device"""
        import torch
        return t.is_cuda and t.device.index == self.device and t.dtype == torch.float64 and t.is_contiguous()

    @staticmethod
    def _host_xy(pk, Xnew, Ynew=None, with_y=False):
        """Xnew as a float64 (N, D) array and Ynew as N entries (None stays None); with_y: the refusal names Ynew too"""
        Xnew = as_f64(Xnew)
        Ynew = None if Ynew is None else as_f64(Ynew).reshape(-1)
        if Xnew.ndim != 2 or Xnew.shape[1] != pk.D or (Ynew is not None and Ynew.size != Xnew.shape[0]):
            raise ValueError('Xnew must be (N,%d)' % pk.D + (' and Ynew must have N entries' if with_y else ''))
        return Xnew, Ynew

    def _device_xy(self, who, pk, X_t, Y_t=None):
        """N of the device rows X_t (N, D) and Y_t (N entries, or None), refused under the method's name `who`"""
        if not (self._device_f64(X_t) and X_t.dim() == 2 and X_t.shape[1] == pk.D):
            raise ValueError('%s: X needs a contiguous float64 (N,%d) tensor on cuda:%d' % (who, pk.D, self.device))
        N = int(X_t.shape[0])
        if Y_t is not None and not (self._device_f64(Y_t) and Y_t.numel() == N):
            raise ValueError('%s: Y needs a contiguous float64 tensor of N entries on cuda:%d' % (who, self.device))
        return N

    def predict(self, p, Xnew, jitter=1e-6, g_offset=0.0):
        """(9,N) array in the order of OnOffSVGP.build_predict (onoffgpf/OnOffSVGP.py:152)."""
        pk = self._prepare(p)
        Xnew, _ = self._host_xy(pk, Xnew)
        out = np.zeros((9, Xnew.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_predict(self.ctx, C.byref(pk.struct), ptr(Xnew), Xnew.shape[0], float(jitter),
                                                          float(g_offset), ptr(out)))
        return out

    def predict_device(self, p, X_t, jitter=1e-6, g_offset=0.0, out=None):
        """predict on a torch CUDA float64 tensor (N,D) of the engine's device; returns (or fills `out` with) a (9,N) CUDA tensor in the
        order of OnOffSVGP.build_predict -- nothing but the parameters crosses PCIe."""
        import torch
        pk = self._prepare(p)
        if not (self._device_f64(X_t) and X_t.dim() == 2 and X_t.shape[1] == pk.D):
            raise ValueError('predict_device: need a contiguous float64 (N,%d) tensor on cuda:%d' % (pk.D, self.device))
        N = int(X_t.shape[0])
        if out is None:
            out = torch.empty((9, N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and tuple(out.shape) == (9, N)):
            raise ValueError('predict_device: out must be a contiguous float64 (9,N) tensor on the same device')
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        if N:
            _check(self.lib, self.ctx, self.lib.zigp_predict_device(self.ctx, C.byref(pk.struct), C.c_void_p(X_t.data_ptr()), N, float(jitter),
                                                                     float(g_offset), C.c_void_p(out.data_ptr())))
        return out

    # ---- heads on the dense path: latent f under a Gaussian or a Bernoulli likelihood (include/zigp.h "heads on the dense path") ----
    def _prepare_head(self, who, p, lik):
        """(packed parameters, ZIGP_LIK_*, len(mean_a) or None): p holds the f fields (HEAD_PARAM_KEYS; 'noise' may be left out for
        'bernoulli') plus 'whiten', 'q_diag', 'kern_f' and the mean function as in elbo; whatever g fields it carries are not read"""
        lik = self._head_lik(who, lik)
        if 'Zf' not in p:
            raise ValueError('%s: p needs Zf, u_fm, u_fs_sqrt, ell_f, var_f (and noise for the Gaussian head)' % who)
        D = as_f64(p['Zf']).shape[-1]
        q = dict(p, **head_placeholder(D, q_full=not p.get('q_diag', True)))
        if lik == _lib.LIK_BERNOULLI:
            q.setdefault('noise', 1.0)
        pk = _Packed(q)
        kinds = kernel_kinds(q)
        mean_D = self._set_mean_function(p, pk.D)
        self.set_whiten(p.get('whiten', False))
        self.set_q_full(not p.get('q_diag', True))
        _check(self.lib, self.ctx, self.lib.zigp_set_kernel(self.ctx, 0, kinds[0]))     # latent g's setting is not read by a head call
        return pk, lik, mean_D

    def head_elbo(self, p, lik, jitter=1e-6, scale=1.0, rows=None, include_kl=True, need_grad=True):
        """The SVGP bound of latent f under lik = 'gaussian' or 'bernoulli' on the resident data (zigp_head_elbo): returns
        (elbo_data, kl, grads or None), ELBO = elbo_data - kl, kl = KL_f.  grads has the keys HEAD_PARAM_KEYS (noise: 0 for 'bernoulli')
        and, with a mean function, mean_a / mean_b.  rows = (begin, end) of the active rows, as in elbo."""
        pk, lik, mean_D = self._prepare_head('head_elbo', p, lik)
        r0, r1 = (0, self.N) if rows is None else rows
        ed, kl = C.c_double(0), C.c_double(0)
        gs, g = None, None
        if need_grad:
            g = dict(Zf=np.zeros((pk.Mf, pk.D)), u_fm=np.zeros(pk.Mf), u_fs_sqrt=np.zeros((pk.Mf, pk.Mf) if pk.q_full else pk.Mf),
                     ell_f=np.zeros(pk.D))
            gs = _lib.zigp_grads()
            for k, a in g.items():
                setattr(gs, k, ptr(a))
        rc = self.lib.zigp_head_elbo(self.ctx, C.byref(pk.struct), lik, float(jitter), float(scale), int(r0), int(r1),
                                     1 if include_kl else 0, C.byref(ed), C.byref(kl), C.byref(gs) if gs is not None else None)
        _check(self.lib, self.ctx, rc)
        if need_grad:
            g['var_f'], g['noise'] = gs.var_f, gs.noise
            if mean_D is not None:
                da, db = np.zeros(max(mean_D, 1)), C.c_double(0)
                _check(self.lib, self.ctx, self.lib.zigp_get_mean_function_grad(self.ctx, ptr(da), mean_D, C.byref(db)))
                g['mean_a'], g['mean_b'] = da[:mean_D], db.value
        return ed.value, kl.value, g

    def head_predict(self, p, Xnew, lik, jitter=1e-6):
        """(4, N): fmean, fvar, pfmean, pfvar in the order of kron_head_predict (zigp_head_predict) -- 'gaussian': fmean, fvar + noise;
        'bernoulli': p = probit(fmean / sqrt(1 + fvar)) through the reference's clamp, p - p^2."""
        pk, lik, _ = self._prepare_head('head_predict', p, lik)
        Xnew, _ = self._host_xy(pk, Xnew)
        out = np.zeros((4, Xnew.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_head_predict(self.ctx, C.byref(pk.struct), lik, ptr(Xnew), Xnew.shape[0], float(jitter), ptr(out)))
        return out

    def head_predict_device(self, p, X_t, lik, jitter=1e-6, out=None):
        """head_predict on a torch CUDA float64 tensor (N, D) of the engine's device; returns (or fills `out` with) a (4, N) CUDA tensor."""
        import torch
        pk, lik, _ = self._prepare_head('head_predict_device', p, lik)
        N = self._device_xy('head_predict_device', pk, X_t)
        if out is None:
            out = torch.empty((4, N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and tuple(out.shape) == (4, N)):
            raise ValueError('head_predict_device: out must be a contiguous float64 (4,N) tensor on the same device')
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        if N:
            _check(self.lib, self.ctx, self.lib.zigp_head_predict_device(self.ctx, C.byref(pk.struct), lik, C.c_void_p(X_t.data_ptr()), N,
                                                                          float(jitter), C.c_void_p(out.data_ptr())))
        return out

    # ---- predictive density of held-out data (include/zigp.h "predictive density") ----
    DENSITY_LIK = {'onoff': _lib.LIK_ONOFF, 'gaussian': _lib.LIK_GAUSSIAN, 'bernoulli': _lib.LIK_BERNOULLI}

    @staticmethod
    def _rule(n_quad, rule):
        """(nodes, weights) as float64 arrays: `rule` when given, else Gauss-Hermite with n_quad nodes; the library checks the values"""
        if rule is None:
            from .quadrature import gauss_hermite
            rule = gauss_hermite(n_quad)
        x, w = as_f64(rule[0]).reshape(-1), as_f64(rule[1]).reshape(-1)
        if x.size != w.size:
            raise ValueError('rule: nodes and weights must have the same length')
        return x, w

    @staticmethod
    def _opt(a):
        """ptr(a), or None (a NULL pointer) for an array the call does not take"""
        return None if a is None else ptr(a)

    @staticmethod
    def _centre(centre, lik=None):
        """True for centre='mode', False for 'mean' (the rule centred on gm); the heads are closed form and have no rule to centre"""
        if centre not in ('mean', 'mode'):
            raise ValueError("centre must be 'mean' (the rule centred on gm) or 'mode' (centred on each row's mode), not %r" % (centre,))
        if centre == 'mode' and lik is not None and lik != _lib.LIK_ONOFF:
            raise ValueError("centre='mode' applies to the 'onoff' density only: the Gaussian and Bernoulli heads are closed form")
        return centre == 'mode'

    def density_rows(self, lik, fm, fv, gm, gv, y, noise, n_quad=64, rule=None, out=None, centre='mean', return_centre=False):
        """Log predictive density of y under rows of a predict call: returns ((3, N) array: logp, ymean, yvar; sum of logp).
        lik 'onoff' (rows 3-6 of predict / kron_predict; g integrated by `rule` = (nodes, weights) for N(0, 1), default Gauss-Hermite
        with n_quad nodes), 'gaussian' or 'bernoulli' (rows 0-1 of kron_head_predict, closed form; gm, gv and the rule are not read and
        may be None).  out: a float64 buffer of at least 3 N entries to fill instead of a new array.
        centre='mode' ('onoff' only) shifts and scales the rule, per row, to a mode of the integrand (zigp_density_rows_centred);
        return_centre=True appends the (2, N) array (zhat, tau) of that search to the result -- zeros and ones under centre='mean'."""
        lik = self.DENSITY_LIK[lik] if isinstance(lik, str) else int(lik)
        mode = self._centre(centre, lik)
        onoff = lik == _lib.LIK_ONOFF
        fm = as_f64(fm).reshape(-1)
        N = fm.size
        rows = [fm] + [None if a is None else as_f64(a).reshape(-1) for a in (fv, gm if onoff else None, gv if onoff else None, y)]
        if any(a is not None and a.size != N for a in rows):
            raise ValueError('density_rows: fm, fv, gm, gv and y must have the same length')
        x, w = self._rule(n_quad, rule) if onoff else (None, None)
        if out is None:
            out = np.zeros(3 * N)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.size >= 3 * N):
            raise ValueError('density_rows: out must be a C-contiguous float64 array of at least 3 N entries')
        total = np.zeros(1)
        centre2 = np.vstack([np.zeros(N), np.ones(N)]) if return_centre else None
        if mode and any(a is None for a in rows):
            raise ValueError("density_rows: centre='mode' needs fm, fv, gm, gv and y")
        # one call: the centred entry has no lik in front and takes the centre (or NULL) behind
        fn, head, tail = (self.lib.zigp_density_rows_centred, (), (self._opt(centre2),)) if mode else (self.lib.zigp_density_rows, (lik,), ())
        _check(self.lib, self.ctx, fn(self.ctx, *head, *[self._opt(a) for a in rows], N, float(noise), self._opt(x), self._opt(w), 0 if x is None else x.size,
                                      ptr(out), ptr(total), *tail))
        res = out.reshape(-1)[:3 * N].reshape(3, N), float(total[0])
        return res + (centre2,) if return_centre else res

    def predict_density(self, p, Xnew, Ynew, jitter=1e-6, g_offset=0.0, n_quad=64, rule=None, rows_out=True, centre='mean', return_centre=False):
        """Held-out log density of the dense OnOff model: predict at Xnew (N, D), then the density of Ynew (N) under its rows, on the device.
        Returns ((3, N) array: logp, ymean, yvar; sum of logp); rows_out=False asks for the sum alone (None in place of the array).
        centre and return_centre: as density_rows."""
        mode = self._centre(centre)
        pk = self._prepare(p)
        Xnew, Ynew = self._host_xy(pk, Xnew, as_f64(Ynew), True)
        x, w = self._rule(n_quad, rule)
        N = Xnew.shape[0]
        out = np.zeros((3, N)) if rows_out else None
        total = np.zeros(1)
        centre2 = np.vstack([np.zeros(N), np.ones(N)]) if return_centre else None
        fn, tail = (self.lib.zigp_predict_density_centred, (self._opt(centre2),)) if mode else (self.lib.zigp_predict_density, ())
        _check(self.lib, self.ctx, fn(self.ctx, C.byref(pk.struct), ptr(Xnew), ptr(Ynew), N, float(jitter), float(g_offset), ptr(x), ptr(w), x.size,
                                      self._opt(out), ptr(total), *tail))
        res = out, float(total[0])
        return res + (centre2,) if return_centre else res

    def predict_density_device(self, p, X_t, Y_t, jitter=1e-6, g_offset=0.0, n_quad=64, rule=None, out=None, centre='mean', return_centre=False):
        """predict_density on torch CUDA float64 tensors X_t (N, D) and Y_t (N) or (N, 1) of the engine's device; returns (a (3, N) CUDA
        tensor, or `out` filled; the sum as a float) -- nothing but the parameters, the rule and the sum crosses PCIe.
        centre and return_centre: as density_rows, the (2, N) centre a CUDA tensor."""
        import torch
        mode = self._centre(centre)
        pk = self._prepare(p)
        N = self._device_xy('predict_density_device', pk, X_t, Y_t)
        if out is None:
            out = torch.empty((3, N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and tuple(out.shape) == (3, N)):
            raise ValueError('predict_density_device: out must be a contiguous float64 (3,N) tensor on the same device')
        x, w = self._rule(n_quad, rule)
        total = np.zeros(1)
        centre2 = None
        if return_centre:
            centre2 = torch.cat([torch.zeros((1, N), dtype=torch.float64, device=X_t.device), torch.ones((1, N), dtype=torch.float64, device=X_t.device)])
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        fn, tail = self.lib.zigp_predict_density_device, ()
        if mode:
            fn, tail = self.lib.zigp_predict_density_centred_device, (None if centre2 is None else C.c_void_p(centre2.data_ptr()),)
        _check(self.lib, self.ctx, fn(self.ctx, C.byref(pk.struct), C.c_void_p(X_t.data_ptr()), C.c_void_p(Y_t.data_ptr()), N, float(jitter),
                                      float(g_offset), ptr(x), ptr(w), x.size, C.c_void_p(out.data_ptr()), ptr(total), *tail))
        res = out, float(total[0])
        return res + (centre2,) if return_centre else res

    # ---- predictive scores: CDF, quantiles and CRPS of y (include/zigp.h "predictive scores") ----
    @staticmethod
    def _levels(levels):
        """the quantile levels as a float64 array, or None for an empty set; the library checks the values"""
        lv = as_f64(levels).reshape(-1)
        if lv.size > _lib.SCORE_MAX_LEVELS:
            raise ValueError('levels: at most %d levels per call (ZIGP_SCORE_MAX_LEVELS), not %d' % (_lib.SCORE_MAX_LEVELS, lv.size))
        return lv if lv.size else None

    @staticmethod
    def _score_result(cdf2, quant, crps, total):
        return {'cdf': None if cdf2 is None else cdf2[0], 'sf': None if cdf2 is None else cdf2[1], 'quantiles': quant, 'crps': crps,
                'crps_sum': None if total is None else float(total[0])}

    @staticmethod
    def _score_outputs(new, N, lv, have_y, cdf, crps):
        """(cdf2, quant, crps, total) of a score call, None where the call does not ask for it; new(*shape): a zeroed array or tensor"""
        want = have_y and crps
        return (new(2, N) if have_y and cdf else None, None if lv is None else new(lv.size, N), new(N) if want else None,
                np.zeros(1) if want else None)

    def score_rows(self, lik, fm, fv, gm, gv, y, noise, n_quad=64, rule=None, levels=(), cdf=True, crps=True):
        """CDF pair, quantiles and CRPS of y under rows of a predict call, as a dict: 'cdf' and 'sf' (N) = F(y) and SF(y), each its own sum;
        'quantiles' (L, N), one row per level of `levels` in the caller's order; 'crps' (N) and 'crps_sum'.  A key is None where that
        output was not asked for: y=None leaves only the quantiles, levels=() leaves them out, cdf=False / crps=False drop those two.
        lik 'onoff' (rows 3-6 of predict / kron_predict; the mixture over `rule` = (nodes, weights) for N(0, 1), default Gauss-Hermite with
        n_quad nodes) or 'gaussian' (rows 0-1 of kron_head_predict, closed form; gm, gv and the rule are not read and may be None).
        'bernoulli' is refused: it has no density, and its CRPS is the Brier score (ymean - y)^2 of density_rows.  The rule is the fixed
        one only: a rule that moves with y (centre='mode') does not define one distribution per row."""
        lik = self.DENSITY_LIK[lik] if isinstance(lik, str) else int(lik)
        onoff = lik == _lib.LIK_ONOFF
        fm = as_f64(fm).reshape(-1)
        N = fm.size
        rows = [fm] + [None if a is None else as_f64(a).reshape(-1) for a in (fv, gm if onoff else None, gv if onoff else None, y)]
        if any(a is not None and a.size != N for a in rows):
            raise ValueError('score_rows: fm, fv, gm, gv and y must have the same length')
        x, w = self._rule(n_quad, rule) if onoff else (None, None)
        lv = self._levels(levels)
        cdf2, quant, out, total = self._score_outputs(lambda *shape: np.zeros(shape), N, lv, rows[4] is not None, cdf, crps)
        _check(self.lib, self.ctx, self.lib.zigp_score_rows(self.ctx, lik, *[self._opt(a) for a in rows], N, float(noise), self._opt(x), self._opt(w),
                                                            0 if x is None else x.size, self._opt(lv), 0 if lv is None else lv.size,
                                                            self._opt(cdf2), self._opt(quant), self._opt(out), self._opt(total)))
        return self._score_result(cdf2, quant, out, total)

    def predict_scores(self, p, Xnew, Ynew=None, jitter=1e-6, g_offset=0.0, n_quad=64, rule=None, levels=(), cdf=True, crps=True):
        """Scores of the dense OnOff model: predict at Xnew (N, D), then score_rows' dict for Ynew (N, or None) under its rows, on the device."""
        pk = self._prepare(p)
        Xnew, Ynew = self._host_xy(pk, Xnew, Ynew, True)
        x, w = self._rule(n_quad, rule)
        lv = self._levels(levels)
        N = Xnew.shape[0]
        cdf2, quant, out, total = self._score_outputs(lambda *shape: np.zeros(shape), N, lv, Ynew is not None, cdf, crps)
        _check(self.lib, self.ctx, self.lib.zigp_predict_scores(self.ctx, C.byref(pk.struct), ptr(Xnew), self._opt(Ynew), N, float(jitter), float(g_offset),
                                                                ptr(x), ptr(w), x.size, self._opt(lv), 0 if lv is None else lv.size,
                                                                self._opt(cdf2), self._opt(quant), self._opt(out), self._opt(total)))
        return self._score_result(cdf2, quant, out, total)

    def predict_scores_device(self, p, X_t, Y_t=None, jitter=1e-6, g_offset=0.0, n_quad=64, rule=None, levels=(), cdf=True, crps=True):
        """predict_scores on torch CUDA float64 tensors X_t (N, D) and Y_t (N) or (N, 1) (or None) of the engine's device; the dict's arrays
        are CUDA tensors, 'crps_sum' a float -- nothing but the parameters, the rule, the levels and the sum crosses PCIe."""
        import torch
        pk = self._prepare(p)
        N = self._device_xy('predict_scores_device', pk, X_t, Y_t)
        x, w = self._rule(n_quad, rule)
        lv = self._levels(levels)
        cdf2, quant, out, total = self._score_outputs(lambda *shape: torch.zeros(shape, dtype=torch.float64, device=X_t.device), N, lv,
                                                      Y_t is not None, cdf, crps)
        D = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        _check(self.lib, self.ctx, self.lib.zigp_predict_scores_device(self.ctx, C.byref(pk.struct), D(X_t), D(Y_t), N, float(jitter), float(g_offset),
                                                                       ptr(x), ptr(w), x.size, self._opt(lv), 0 if lv is None else lv.size,
                                                                       D(cdf2), D(quant), D(out), self._opt(total)))
        return self._score_result(cdf2, quant, out, total)

    # ---- sample paths: joint posterior draws at test inputs (include/zigp.h "sample paths") ----
    @staticmethod
    def _path_latents(lats, D, S):
        """The zigp_path_latent records of path_rows and the arrays behind them.  A latent is a dict: kind ('rbf' / 'matern32' /
        'matern52' or a ZIGP_KERN_* value), Z (M, D), ell, var, V (M, S), omega (R, D), phase (R), amp (R, S) and, optional, lin (D)
        and shift.  Sizes and shapes are checked here, before the library is touched."""
        from . import pathwise
        pathwise.check_sizes(D, S)
        if len(lats) not in (1, 2):
            raise ValueError('path_rows takes one or two latents, not %d' % len(lats))
        recs, keep = (_lib.zigp_path_latent * len(lats))(), []
        for h, q in enumerate(lats):
            Z = as_f64(q['Z'])
            if Z.ndim != 2 or Z.shape[1] != D or Z.shape[0] < 1:
                raise ValueError('latent %d: Z must be (M,%d) with M >= 1' % (h, D))
            M = Z.shape[0]
            ell = as_f64(q['ell']).reshape(-1)
            ell = np.full(D, float(ell[0])) if ell.size == 1 else np.ascontiguousarray(ell)
            if ell.size != D:
                raise ValueError('latent %d: ell must be scalar or have D entries' % h)
            phase = as_f64(q['phase']).reshape(-1)
            R = phase.size
            arr = dict(Z=Z, ell=ell, V=as_f64(q['V']), omega=as_f64(q['omega']).reshape(R, -1) if R else np.zeros((0, D)), phase=phase,
                       amp=as_f64(q['amp']).reshape(R, -1) if R else np.zeros((0, S)))
            for k, shape in (('V', (M, S)), ('omega', (R, D)), ('amp', (R, S))):
                if arr[k].shape != shape:
                    raise ValueError('latent %d: %s must be %s, not %s' % (h, k, shape, arr[k].shape))
            lin = q.get('lin')
            if lin is not None:
                lin = as_f64(lin).reshape(-1)
                if lin.size != D:
                    raise ValueError('latent %d: lin must have D entries' % h)
                arr['lin'] = lin
            r = recs[h]
            r.kind, r.M, r.R = pathwise._kind(q.get('kind', 'rbf')), M, R
            r.var, r.shift = float(np.squeeze(q['var'])), float(q.get('shift', 0.0))
            for k, a in arr.items():
                setattr(r, k, ptr(a) if a.size else None)
            keep.append(arr)
        return recs, keep

    def path_rows(self, lats, X, S):
        """The finite sum of zigp_path_rows: lats a list of one or two latent dicts (see _path_latents), X (N, D) host rows;
        returns (nlat, S, N)."""
        X = as_f64(X)
        if X.ndim != 2:
            raise ValueError('X must be (N, D)')
        N, D = X.shape
        recs, keep = self._path_latents(lats, D, int(S))
        out = np.zeros((len(lats), int(S), N))
        _check(self.lib, self.ctx, self.lib.zigp_path_rows(self.ctx, C.cast(recs, C.c_void_p), len(lats), D, int(S), ptr(X), N, ptr(out)))
        return out

    def path_rows_device(self, lats, X_t, S, out=None):
        """path_rows on a torch CUDA float64 tensor (N, D) of the engine's device; returns (or fills `out`, whose first nlat S N
        entries are the (nlat, S, N) result) a CUDA tensor."""
        import torch
        if not (self._device_f64(X_t) and X_t.dim() == 2):
            raise ValueError('path_rows_device: X needs a contiguous float64 (N, D) tensor on cuda:%d' % self.device)
        N, D = int(X_t.shape[0]), int(X_t.shape[1])
        recs, keep = self._path_latents(lats, D, int(S))
        if out is None:
            out = torch.empty((len(lats), int(S), N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and out.numel() >= len(lats) * int(S) * N):
            raise ValueError('path_rows_device: out must be a contiguous float64 tensor of at least nlat S N entries on the same device')
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        _check(self.lib, self.ctx, self.lib.zigp_path_rows_device(self.ctx, C.cast(recs, C.c_void_p), len(lats), D, int(S),
                                                                   C.c_void_p(X_t.data_ptr()), N, C.c_void_p(out.data_ptr())))
        return out

    def _path_draws(self, pk, kinds, n_samples, n_features, rng, draws):
        """(draws dict, the two zigp_path_draw records, the arrays behind them): new draws from rng unless `draws` is handed back"""
        from . import pathwise
        S = int(n_samples)
        pathwise.check_sizes(pk.D, S)
        if draws is None:
            if rng is None:
                rng = np.random.RandomState()
            elif isinstance(rng, (int, np.integer)):
                rng = np.random.RandomState(int(rng))
            draws = {tag: pathwise.draw(kinds[h], int(n_features), pk.D, M, S, rng) for h, (tag, M) in enumerate((('f', pk.Mf), ('g', pk.Mg)))}
        recs, keep = [], []
        for tag, M in (('f', pk.Mf), ('g', pk.Mg)):
            R, arr = pathwise.check_draw(draws[tag], tag, M, pk.D, S)
            r = _lib.zigp_path_draw()
            r.R = R
            for k, a in arr.items():
                setattr(r, k, ptr(a) if a.size else None)
            recs.append(r)
            keep.append(arr)
        return draws, recs, keep

    def sample_paths(self, p, Xnew, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, g_offset=0.0):
        """Joint posterior sample paths of the dense OnOff model at Xnew (N, D) by pathwise conditioning (zigp_sample_paths): returns
        dict(f, g, gf: (S, N) each; draws).  rng: a numpy RandomState / Generator or a seed.  draws: the `draws` of an earlier call --
        the same paths at other inputs or other hyperparameters (n_samples and the model's M must match them).  p is read as predict
        reads it (whiten, q_diag, kern_f / kern_g, mean_a / mean_b).  D <= 8, 1 <= n_samples <= 256."""
        pk = _Packed(p)
        Xnew, _ = self._host_xy(pk, Xnew)
        draws, recs, keep = self._path_draws(pk, pk.kinds, n_samples, n_features, rng, draws)
        self._prepare(p, pk)      # behind the draws' checks: a refused draw leaves the context's modes as they were
        S, N = int(n_samples), Xnew.shape[0]
        out = np.zeros((3, S, N))
        _check(self.lib, self.ctx, self.lib.zigp_sample_paths(self.ctx, C.byref(pk.struct), ptr(Xnew), N, float(jitter), float(g_offset),
                                                               C.addressof(recs[0]), C.addressof(recs[1]), S, ptr(out)))
        return dict(f=out[0], g=out[1], gf=out[2], draws=draws)

    def sample_paths_device(self, p, X_t, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, g_offset=0.0, out=None):
        """sample_paths on a torch CUDA float64 tensor (N, D) of the engine's device: f, g, gf are views of one (3, S, N) CUDA tensor
        (`out` when given) -- nothing but the parameters and the draws crosses PCIe."""
        import torch
        pk = _Packed(p)
        N = self._device_xy('sample_paths_device', pk, X_t)
        draws, recs, keep = self._path_draws(pk, pk.kinds, n_samples, n_features, rng, draws)
        self._prepare(p, pk)
        S = int(n_samples)
        if out is None:
            out = torch.empty((3, S, N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and tuple(out.shape) == (3, S, N)):
            raise ValueError('sample_paths_device: out must be a contiguous float64 (3,S,N) tensor on the same device')
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        if N:
            _check(self.lib, self.ctx, self.lib.zigp_sample_paths_device(self.ctx, C.byref(pk.struct), C.c_void_p(X_t.data_ptr()), N, float(jitter),
                                                                          float(g_offset), C.addressof(recs[0]), C.addressof(recs[1]), S,
                                                                          C.c_void_p(out.data_ptr())))
        return dict(f=out[0], g=out[1], gf=out[2], draws=draws)

    # ---- Kronecker sample paths (include/zigp_kronpaths.h) ----
    @staticmethod
    def _kron_path_latents(lats, dims, S):
        """The zigp_kron_path_latent records of kron_path_rows and the arrays behind them.  A latent is a dict: Z = [Z0 (M0, D0),
        Z1 (M1, D1)], ell = [ell0, ell1], var = [var0, var1], V (M0 M1, S) factor-0-major, omega (R, D0 + D1), phase (R), amp (R, S)
        and, optional, shift and kinds (a kernel name for both factors or a pair (kind0, kind1); default 'rbf').  Sizes and shapes are checked here, before the library is touched."""
        from . import pathwise
        D0, D1 = dims
        if len(lats) not in (1, 2):
            raise ValueError('kron_path_rows takes one or two latents, not %d' % len(lats))
        recs, keep = (_lib.zigp_kron_path_latent * len(lats))(), []
        for h, q in enumerate(lats):
            Z0, Z1 = as_f64(q['Z'][0]), as_f64(q['Z'][1])
            if Z0.ndim != 2 or Z1.ndim != 2 or Z0.shape[1] != D0 or Z1.shape[1] != D1:
                raise ValueError('latent %d: Z must be [(M0,%d), (M1,%d)]' % (h, D0, D1))
            M0, M1 = Z0.shape[0], Z1.shape[0]
            pathwise.check_kron_sizes(D0, D1, M0, M1, S)
            ells = []
            for k, Dq in ((0, D0), (1, D1)):
                e = as_f64(q['ell'][k]).reshape(-1)
                e = np.full(Dq, float(e[0])) if e.size == 1 else np.ascontiguousarray(e)
                if e.size != Dq:
                    raise ValueError('latent %d: ell[%d] must be scalar or have %d entries' % (h, k, Dq))
                ells.append(e)
            phase = as_f64(q['phase']).reshape(-1)
            R, D, M = phase.size, D0 + D1, M0 * M1
            arr = dict(Z0=Z0, Z1=Z1, ell0=ells[0], ell1=ells[1], V=as_f64(q['V']), omega=as_f64(q['omega']).reshape(R, -1) if R else np.zeros((0, D)),
                       phase=phase, amp=as_f64(q['amp']).reshape(R, -1) if R else np.zeros((0, S)))
            for k, shape in (('V', (M, S)), ('omega', (R, D)), ('amp', (R, S))):
                if arr[k].shape != shape:
                    raise ValueError('latent %d: %s must be %s, not %s' % (h, k, shape, arr[k].shape))
            r = recs[h]
            r.M0, r.M1, r.R = M0, M1, R
            k0, k1 = pathwise.kron_kinds(q.get('kinds', 'rbf'))      # the factor kinds of this latent's record: a name or a pair
            r.reserved = k0 + 4 * k1                                    # the record's fourth word carries the kinds (include/zigp_kronpaths.h)
            r.var0, r.var1, r.shift = _scalar(q['var'][0]), _scalar(q['var'][1]), float(q.get('shift', 0.0))
            for k, a in arr.items():
                setattr(r, k, ptr(a) if a.size else None)
            keep.append(arr)
        return recs, keep

    def kron_path_rows(self, lats, X, S, dims):
        """The finite sum of zigp_kron_path_rows: lats a list of one or two latent dicts (see _kron_path_latents), X (N, D0 + D1) host
        rows, dims = (D0, D1); returns (nlat, S, N)."""
        D0, D1 = int(dims[0]), int(dims[1])
        X = self._kron_rows(X, (D0, D1))
        recs, keep = self._kron_path_latents(lats, (D0, D1), int(S))
        N = X.shape[0]
        out = np.zeros((len(lats), int(S), N))
        _check(self.lib, self.ctx, self.lib.zigp_kron_path_rows(self.ctx, C.cast(recs, C.c_void_p), len(lats), D0, D1, int(S), ptr(X), N, ptr(out)))
        return out

    def kron_path_rows_device(self, lats, X_t, S, dims, out=None):
        """kron_path_rows on a torch CUDA float64 tensor (N, D0 + D1) of the engine's device; returns (or fills `out`, whose first
        nlat S N entries are the (nlat, S, N) result) a CUDA tensor."""
        import torch
        D0, D1 = int(dims[0]), int(dims[1])
        if not (self._device_f64(X_t) and X_t.dim() == 2 and int(X_t.shape[1]) == D0 + D1):
            raise ValueError('kron_path_rows_device: X needs a contiguous float64 (N, %d) tensor on cuda:%d' % (D0 + D1, self.device))
        N = int(X_t.shape[0])
        recs, keep = self._kron_path_latents(lats, (D0, D1), int(S))
        if out is None:
            out = torch.empty((len(lats), int(S), N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and out.numel() >= len(lats) * int(S) * N):
            raise ValueError('kron_path_rows_device: out must be a contiguous float64 tensor of at least nlat S N entries on the same device')
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        _check(self.lib, self.ctx, self.lib.zigp_kron_path_rows_device(self.ctx, C.cast(recs, C.c_void_p), len(lats), D0, D1, int(S),
                                                                        C.c_void_p(X_t.data_ptr()), N, C.c_void_p(out.data_ptr())))
        return out

    @staticmethod
    def _kron_path_draws(s, dims, tags, n_samples, n_features, rng, draws, kinds=None):
        """(draws dict, the zigp_path_draw records by tag, the arrays behind them) for the packed Kronecker parameters s; kinds: the
        factor kinds by tag (kron_kernel_kinds), which decide the spectral law of each factor's frequencies"""
        from . import pathwise
        S, D = int(n_samples), dims[0] + dims[1]
        grids = {t: (int(getattr(s, 'M0' + t)), int(getattr(s, 'M1' + t))) for t in tags}
        for t in tags:
            pathwise.check_kron_sizes(dims[0], dims[1], grids[t][0], grids[t][1], S)
        if draws is None:
            if rng is None:
                rng = np.random.RandomState()
            elif isinstance(rng, (int, np.integer)):
                rng = np.random.RandomState(int(rng))
            kinds = kinds or {}
            draws = {t: pathwise.kron_draw(kinds.get(t, (0, 0)), int(n_features), dims[0], dims[1], grids[t][0], grids[t][1], S, rng) for t in tags}
        recs, keep = {}, []
        for t in tags:
            R, arr = pathwise.check_draw(draws[t], t, grids[t][0] * grids[t][1], D, S)
            r = _lib.zigp_path_draw()
            r.R = R
            for k, a in arr.items():
                setattr(r, k, ptr(a) if a.size else None)
            recs[t] = r
            keep.append(arr)
        return draws, recs, keep

    def _kron_paths_out(self, who, X_t, planes, S, out):
        import torch
        N = int(X_t.shape[0])
        if out is None:
            out = torch.empty((planes, S, N), dtype=torch.float64, device=X_t.device)
        elif not (self._device_f64(out) and tuple(out.shape) == (planes, S, N)):
            raise ValueError('%s: out must be a contiguous float64 (%d,S,N) tensor on the same device' % (who, planes))
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        return out

    def _kron_device_rows(self, who, X_t, dims):
        if not (self._device_f64(X_t) and X_t.dim() == 2 and int(X_t.shape[1]) == dims[0] + dims[1]):
            raise ValueError('%s: Xnew needs a contiguous float64 (N, %d) tensor on cuda:%d' % (who, dims[0] + dims[1], self.device))
        return int(X_t.shape[0])

    def kron_sample_paths(self, p, Xnew, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, g_offset=0.0, f_mu=None):
        """Joint posterior sample paths of the Kronecker OnOff model at Xnew (N, D0 + D1) by pathwise conditioning
        (zigp_kron_sample_paths): returns dict(f, g, gf: (S, N) each; draws).  p as kron_predict reads it; rng, draws as sample_paths
        (a draw has omega0 (R, D0 + D1) and eps (M0 M1, S)).  D0 + D1 <= 8, grids of at most 128 x 128, 1 <= n_samples <= 256."""
        s, keep, dims = self._pack_kron(p)
        self._set_kron_kinds(p)
        Xnew = self._kron_rows(Xnew, dims, 'Xnew')
        draws, recs, keepd = self._kron_path_draws(s, dims, ('f', 'g'), n_samples, n_features, rng, draws, kron_kernel_kinds(p, ('f', 'g')))
        S, N = int(n_samples), Xnew.shape[0]
        out = np.zeros((3, S, N))
        _check(self.lib, self.ctx, self.lib.zigp_kron_sample_paths(self.ctx, C.byref(s), ptr(Xnew), N, float(jitter), float(g_offset),
                                                                    0.0 if f_mu is None else _scalar(f_mu), C.addressof(recs['f']),
                                                                    C.addressof(recs['g']), S, ptr(out)))
        return dict(f=out[0], g=out[1], gf=out[2], draws=draws)

    def kron_sample_paths_device(self, p, X_t, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, g_offset=0.0, f_mu=None,
                                 out=None):
        """kron_sample_paths on a torch CUDA float64 tensor (N, D0 + D1) of the engine's device: f, g, gf are views of one (3, S, N)
        CUDA tensor (`out` when given)."""
        s, keep, dims = self._pack_kron(p)
        self._set_kron_kinds(p)
        N = self._kron_device_rows('kron_sample_paths_device', X_t, dims)
        draws, recs, keepd = self._kron_path_draws(s, dims, ('f', 'g'), n_samples, n_features, rng, draws, kron_kernel_kinds(p, ('f', 'g')))
        S = int(n_samples)
        out = self._kron_paths_out('kron_sample_paths_device', X_t, 3, S, out)
        if N:
            _check(self.lib, self.ctx, self.lib.zigp_kron_sample_paths_device(self.ctx, C.byref(s), C.c_void_p(X_t.data_ptr()), N, float(jitter),
                                                                               float(g_offset), 0.0 if f_mu is None else _scalar(f_mu),
                                                                               C.addressof(recs['f']), C.addressof(recs['g']), S,
                                                                               C.c_void_p(out.data_ptr())))
        return dict(f=out[0], g=out[1], gf=out[2], draws=draws)

    def _head_lik(self, who, lik):
        if lik not in self.LIK:
            raise ValueError("%s: lik must be 'gaussian' or 'bernoulli', not %r (the on/off paths are kron_sample_paths)" % (who, lik))
        return self.LIK[lik]

    def kron_head_sample_paths(self, p, Xnew, lik, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, f_mu=0.0):
        """Sample paths of a single-latent head (zigp_kron_head_sample_paths): dict(f (S, N), draws) for 'gaussian', dict(f, p, draws)
        for 'bernoulli' (p = the probit link of f with the reference's 1e-3 clamp).  p holds the f fields only; f already carries f_mu."""
        code = self._head_lik('kron_head_sample_paths', lik)
        s, keep, dims = self._pack_kron(p, tags=('f',))
        self._set_kron_kinds(p, ('f',))
        Xnew = self._kron_rows(Xnew, dims, 'Xnew')
        draws, recs, keepd = self._kron_path_draws(s, dims, ('f',), n_samples, n_features, rng, draws, kron_kernel_kinds(p, ('f',)))
        S, N, planes = int(n_samples), Xnew.shape[0], 2 if lik == 'bernoulli' else 1
        out = np.zeros((planes, S, N))
        _check(self.lib, self.ctx, self.lib.zigp_kron_head_sample_paths(self.ctx, C.byref(s), code, ptr(Xnew), N, float(jitter), _scalar(f_mu),
                                                                         C.addressof(recs['f']), S, ptr(out)))
        res = dict(f=out[0], draws=draws)
        if planes == 2:
            res['p'] = out[1]
        return res

    def kron_head_sample_paths_device(self, p, X_t, lik, n_samples=16, n_features=1024, rng=None, draws=None, jitter=1e-6, f_mu=0.0, out=None):
        """kron_head_sample_paths on a torch CUDA float64 tensor of the engine's device: views of one (1 or 2, S, N) CUDA tensor."""
        code = self._head_lik('kron_head_sample_paths_device', lik)
        s, keep, dims = self._pack_kron(p, tags=('f',))
        self._set_kron_kinds(p, ('f',))
        N = self._kron_device_rows('kron_head_sample_paths_device', X_t, dims)
        draws, recs, keepd = self._kron_path_draws(s, dims, ('f',), n_samples, n_features, rng, draws, kron_kernel_kinds(p, ('f',)))
        S, planes = int(n_samples), 2 if lik == 'bernoulli' else 1
        out = self._kron_paths_out('kron_head_sample_paths_device', X_t, planes, S, out)
        if N:
            _check(self.lib, self.ctx, self.lib.zigp_kron_head_sample_paths_device(self.ctx, C.byref(s), code, C.c_void_p(X_t.data_ptr()), N,
                                                                                    float(jitter), _scalar(f_mu), C.addressof(recs['f']), S,
                                                                                    C.c_void_p(out.data_ptr())))
        res = dict(f=out[0], draws=draws)
        if planes == 2:
            res['p'] = out[1]
        return res

    # ---- sample-path scores: totals, energy and variogram scores of an ensemble (include/zigp_ensemble.h) ----
    ENS_KEYS = ('total', 'total_obs', 'crps_total', 'energy', 'variogram', 'dist')

    @staticmethod
    def _ens_outputs(new, S, G, energy, totals, variogram, return_dist):
        """The six outputs of an ensemble call in the order of ENS_KEYS, None where the call does not ask; new(*shape): an array or tensor"""
        return [new(S, G) if totals else None, new(G) if totals else None, new(G) if totals else None, new(G) if energy else None,
                new(G) if variogram is not None else None, new(G, S + 1, S + 1) if return_dist else None]

    def ensemble_scores(self, E, y, groups=None, weights=None, energy=True, totals=True, variogram=None, fair=False, return_dist=False):
        """Scores of an ensemble E (S members, N rows) against the observation y (N) per group of rows (zigp_ensemble_scores), as a dict:
        'total' (S, G) and 'total_obs' (G), the weighted group sums; 'crps_total' (G), the ensemble CRPS of the totals; 'energy' (G), the
        energy score over the group's rows; 'variogram' (G), the variogram score of order p = variogram (0.5, 1 or 2); 'dist'
        (G, S + 1, S + 1), the matrix of weighted distances between members, member S = y; 'offsets' (G + 1) and 'labels' (the distinct
        labels in group order, or None).  A key is None where that output was not asked for (totals=False drops the first three).
        groups: None (one group), G + 1 boundaries from 0 to N, or N integer labels -- labels that are not non-decreasing cost one stable
        sort of the columns (np.take), and the groups come back in ascending label order.  weights: N row weights >= 0 (cell areas), default
        1.  fair=True: c = 1 / (S (S - 1)) in place of 1 / S^2.  E may be a row-strided view (rows of stride >= N doubles)."""
        from . import ensemble as ens
        E = np.asarray(E, dtype=np.float64)
        if E.ndim != 2:
            raise ValueError('E must be (S, N)')
        S, N = E.shape
        y = as_f64(y).reshape(-1)
        if y.size != N:
            raise ValueError('y must have N = %d entries' % N)
        w = None if weights is None else as_f64(weights).reshape(-1)
        if w is not None and w.size != N:
            raise ValueError('weights must have N = %d entries' % N)
        off, order, labels = ens.plan_groups(groups, N)
        opts = ens.check_args(S, N, off, w, variogram, fair)
        if order is not None:
            E, y, w = np.take(E, order, axis=1), np.take(y, order), None if w is None else np.take(w, order)
        if S == 1 or not (E.strides[1] == 8 and E.strides[0] % 8 == 0 and E.strides[0] >= 8 * N):
            E = np.ascontiguousarray(E)
        ld = N if S == 1 else E.strides[0] // 8
        G = off.size - 1
        outs = self._ens_outputs(lambda *shape: np.zeros(shape), S, G, energy, totals, variogram, return_dist)
        if any(o is not None for o in outs):
            _check(self.lib, self.ctx, self.lib.zigp_ensemble_scores(self.ctx, E.ctypes.data, ld, S, N, ptr(y), self._opt(w),
                                                                      off.ctypes.data_as(C.POINTER(C.c_int64)), G, C.byref(opts),
                                                                      *[self._opt(o) for o in outs]))
        return dict(zip(self.ENS_KEYS, outs), offsets=off, labels=labels)

    def ensemble_scores_device(self, E_t, y_t, groups=None, weights=None, energy=True, totals=True, variogram=None, fair=False,
                               return_dist=False):
        """ensemble_scores on torch CUDA float64 tensors of the engine's device: E_t (S, N) with unit column stride and a row stride of
        at least N -- a plane of a (3, S, N) paths block, or a row-strided view of one, is read where it is; y_t (N) or (N, 1); weights a
        tensor of N entries (or None; not checked for sign).  The dict's outputs are CUDA tensors: nothing but the boundaries crosses PCIe.
        Unsorted labels cost one index_select of the columns."""
        import torch
        from . import ensemble as ens
        ok = lambda t: t.is_cuda and t.device.index == self.device and t.dtype == torch.float64     # noqa: E731
        if not (ok(E_t) and E_t.dim() == 2 and (E_t.shape[1] == 0 or E_t.stride(1) == 1) and (E_t.shape[0] == 1 or E_t.stride(0) >= E_t.shape[1])):
            raise ValueError('ensemble_scores_device: E needs a float64 (S, N) tensor on cuda:%d with unit column stride and a row stride >= N'
                             % self.device)
        S, N = int(E_t.shape[0]), int(E_t.shape[1])
        if not (ok(y_t) and y_t.numel() == N and y_t.is_contiguous()):
            raise ValueError('ensemble_scores_device: y needs a contiguous float64 tensor of N entries on cuda:%d' % self.device)
        if weights is not None and not (ok(weights) and weights.numel() == N and weights.is_contiguous()):
            raise ValueError('ensemble_scores_device: weights needs a contiguous float64 tensor of N entries on cuda:%d' % self.device)
        off, order, labels = ens.plan_groups(groups, N)
        opts = ens.check_args(S, N, off, None, variogram, fair)
        y_t = y_t.reshape(-1)
        w_t = None if weights is None else weights.reshape(-1)
        if order is not None:
            idx = torch.as_tensor(order, device=E_t.device)
            E_t, y_t = E_t.index_select(1, idx), y_t.index_select(0, idx)
            w_t = None if w_t is None else w_t.index_select(0, idx)
        ld = N if S == 1 else int(E_t.stride(0))
        G = off.size - 1
        outs = self._ens_outputs(lambda *shape: torch.zeros(shape, dtype=torch.float64, device=E_t.device), S, G, energy, totals, variogram,
                                 return_dist)
        D = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        if any(o is not None for o in outs):
            _check(self.lib, self.ctx, self.lib.zigp_ensemble_scores_device(self.ctx, D(E_t), ld, S, N, D(y_t), D(w_t),
                                                                             off.ctypes.data_as(C.POINTER(C.c_int64)), G, C.byref(opts),
                                                                             *[D(o) for o in outs]))
        return dict(zip(self.ENS_KEYS, outs), offsets=off, labels=labels)

    def _score_paths(self, who, paths, noise, Y_t, member, noise_eps, score_args):
        """ensemble_scores_device of one plane of a paths dict against Y_t; with noise_eps (S, N) the members get observation noise"""
        from . import ensemble as ens
        E_t = paths[ens.member_plane(member)]
        if noise_eps is not None:
            if not (self._device_f64(noise_eps) and tuple(noise_eps.shape) == tuple(E_t.shape)):
                raise ValueError('%s: noise_eps needs a contiguous float64 (S, N) tensor of standard normals on cuda:%d' % (who, self.device))
            E_t = E_t + float(np.sqrt(noise)) * noise_eps
        res = self.ensemble_scores_device(E_t, Y_t, **score_args)
        res['draws'] = paths['draws']
        return res

    def path_scores_device(self, p, X_t, Y_t, groups=None, n_samples=16, member='gf', noise_eps=None, weights=None, energy=True, totals=True,
                           variogram=None, fair=False, return_dist=False, n_features=1024, rng=None, draws=None, jitter=1e-6, g_offset=0.0):
        """Scores of the dense OnOff model's joint sample paths at X_t (N, D) against Y_t (N): sample_paths_device, then
        ensemble_scores_device of the plane `member` ('f', 'g' or 'gf') where it lies -- only parameters, draws and scores cross PCIe.
        Without noise_eps the members are the NOISE-FREE paths (the latent product gf, not draws of y); with noise_eps, a CUDA (S, N)
        tensor of standard normals the caller drew, they are gf + sqrt(noise) noise_eps.  Returns ensemble_scores_device's dict plus
        'draws' (hand them back to score the same paths again)."""
        from . import ensemble as ens
        ens.member_plane(member)
        pk = _Packed(p)
        N = self._device_xy('path_scores_device', pk, X_t, Y_t)
        ens.check_args(int(n_samples), max(N, 1), ens.plan_groups(groups, N)[0], None, variogram, fair)
        paths = self.sample_paths_device(p, X_t, n_samples=n_samples, n_features=n_features, rng=rng, draws=draws, jitter=jitter, g_offset=g_offset)
        return self._score_paths('path_scores_device', paths, float(np.squeeze(p['noise'])), Y_t, member, noise_eps,
                                 dict(groups=groups, weights=weights, energy=energy, totals=totals, variogram=variogram, fair=fair,
                                      return_dist=return_dist))

    def kron_path_scores_device(self, p, X_t, Y_t, groups=None, n_samples=16, member='gf', noise_eps=None, weights=None, energy=True,
                                totals=True, variogram=None, fair=False, return_dist=False, n_features=1024, rng=None, draws=None, jitter=1e-6,
                                g_offset=0.0, f_mu=None):
        """path_scores_device for the Kronecker OnOff model: kron_sample_paths_device, then ensemble_scores_device of the plane `member`.
        The members are noise-free unless noise_eps is given (p['noise'] is then the observation variance)."""
        from . import ensemble as ens
        ens.member_plane(member)
        N = int(X_t.shape[0])
        ens.check_args(int(n_samples), max(N, 1), ens.plan_groups(groups, N)[0], None, variogram, fair)
        paths = self.kron_sample_paths_device(p, X_t, n_samples=n_samples, n_features=n_features, rng=rng, draws=draws, jitter=jitter,
                                              g_offset=g_offset, f_mu=f_mu)
        return self._score_paths('kron_path_scores_device', paths, float(np.squeeze(p['noise'])) if noise_eps is not None else 0.0, Y_t, member,
                                 noise_eps, dict(groups=groups, weights=weights, energy=energy, totals=totals, variogram=variogram, fair=fair,
                                                 return_dist=return_dist))

    # ---- inducing inputs by k-means on the device (include/zigp.h "inducing inputs"; zigp.inducing) ----
    @staticmethod
    def _kmeans_args(N, ld, M, init, seed, max_iter, cols, rows_of):
        """(col0, D, C, outputs) of a k-means call, every refusal raised before the library is touched.  init None: the rows
        zigp.inducing.sample_rows(N, M, seed), fetched by rows_of(idx) -> (M, ld)."""
        from . import inducing
        M, max_iter = int(M), int(max_iter)
        col0, D = inducing.check_cols(cols, ld)
        inducing.check_sizes(N, D, M, max_iter)
        if init is None:
            Cm = np.array(rows_of(inducing.sample_rows(N, M, seed))[:, col0:col0 + D], dtype=np.float64, order='C')
        else:
            Cm = inducing.check_init(init, M, D)
        return col0, D, Cm, dict(labels=np.zeros(N, dtype=np.int32), counts=np.zeros(M, dtype=np.int64), history=np.zeros((max_iter, 2)))

    @staticmethod
    def _kmeans_result(Cm, out, n_iter, return_info):
        if not return_info:
            return Cm
        h = out['history'][:n_iter]
        return Cm, dict(labels=out['labels'], counts=out['counts'], inertia=h[:, 0].copy(), changed=h[:, 1].astype(np.int64), n_iter=n_iter,
                        n_empty=int(np.count_nonzero(out['counts'] == 0)))

    def kmeans(self, X, M, init=None, seed=None, max_iter=100, cols=None, return_info=False):
        """Lloyd iterations on the device from a start the caller chooses (zigp_kmeans; the definition is zigp.inducing.kmeans_np).
        X (N, ld) host rows, of which cols = (col0, D) are used (None: all); init None: the rows sample_rows(N, M, seed), else an
        (M, D) array.  Returns the (M, D) centroids, with return_info also dict(labels, counts, inertia, changed, n_iter, n_empty)."""
        X = as_f64(X)
        if X.ndim != 2:
            raise ValueError('X must be (N, ld)')
        N, ld = X.shape
        col0, D, Cm, out = self._kmeans_args(N, ld, M, init, seed, max_iter, cols, lambda idx: X[idx])
        n = C.c_int32(0)
        _check(self.lib, self.ctx, self.lib.zigp_kmeans(self.ctx, ptr(X), N, ld, col0, D, int(M), ptr(Cm), int(max_iter), out['labels'].ctypes.data,
                                                        out['counts'].ctypes.data, ptr(out['history']), C.byref(n)))
        return self._kmeans_result(Cm, out, n.value, return_info)

    def kmeans_device(self, X_t, M, init=None, seed=None, max_iter=100, cols=None, return_info=False):
        """kmeans on a torch CUDA float64 tensor (N, ld) of the engine's device (zigp_kmeans_device): the rows stay where they are, the
        centroids and the info come back as host arrays."""
        import torch
        if not (self._device_f64(X_t) and X_t.dim() == 2):
            raise ValueError('kmeans_device: X needs a contiguous float64 (N, ld) tensor on cuda:%d' % self.device)
        N, ld = int(X_t.shape[0]), int(X_t.shape[1])
        col0, D, Cm, out = self._kmeans_args(N, ld, M, init, seed, max_iter, cols,
                                             lambda idx: X_t[torch.as_tensor(idx, device=X_t.device)].cpu().numpy())
        torch.cuda.current_stream(self.device).synchronize()      # the engine's streams are not ordered after torch's
        n = C.c_int32(0)
        _check(self.lib, self.ctx, self.lib.zigp_kmeans_device(self.ctx, C.c_void_p(X_t.data_ptr()), N, ld, col0, D, int(M), ptr(Cm), int(max_iter),
                                                               out['labels'].ctypes.data, out['counts'].ctypes.data, ptr(out['history']), C.byref(n)))
        return self._kmeans_result(Cm, out, n.value, return_info)

    def kmeans_resident(self, M, init=None, max_iter=100, cols=None, return_info=False):
        """kmeans on the WHOLE resident set of set_data / set_data_device (zigp_kmeans_resident): a selection made by select_rows is
        ignored and left as it was.  init is an (M, D) start: the rows are on the device, so the caller picks it (e.g.
        X[sample_rows(N, M, seed)] before set_data)."""
        if self._full_N < 1:
            raise ValueError('kmeans_resident: no resident data (call set_data first)')
        if init is None:
            raise ValueError('kmeans_resident: init must be an (M, D) array (the rows are on the device: nothing to sample from here)')
        N, ld = int(self._full_N), int(self.D)
        col0, D, Cm, out = self._kmeans_args(N, ld, M, init, None, max_iter, cols, None)
        n = C.c_int32(0)
        _check(self.lib, self.ctx, self.lib.zigp_kmeans_resident(self.ctx, col0, D, int(M), ptr(Cm), int(max_iter), out['labels'].ctypes.data,
                                                                 out['counts'].ctypes.data, ptr(out['history']), C.byref(n)))
        return self._kmeans_result(Cm, out, n.value, return_info)

    def prior_kl(self, p, jitter=1e-6):
        pk = _Packed(p)
        self._set_modes(p)
        out = np.zeros(2)
        _check(self.lib, self.ctx, self.lib.zigp_prior_kl(self.ctx, C.byref(pk.struct), float(jitter), ptr(out)))
        return out

    def rbf_K(self, X1, X2, ell, var):
        X1 = as_f64(X1)
        D = X1.shape[1]
        X2a = X1 if X2 is None else as_f64(X2)
        ell = as_f64(ell).reshape(-1)
        if ell.size == 1:
            ell = np.full(D, float(ell[0]))
        out = np.zeros((X1.shape[0], X2a.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_rbf_K(self.ctx, ptr(X1), X1.shape[0], None if X2 is None else ptr(X2a), X2a.shape[0], D,
                                                        ptr(ell), float(np.squeeze(var)), ptr(out)))
        return out

    def kern_K(self, kind, X1, X2, ell, var):
        """K(X1, X2) of the kernel `kind` ('rbf', 'matern32', 'matern52'), no jitter (zigp_kern_K; gpflow kernels.Stationary.K);
        X2 None: K(X1, X1), whose diagonal is the formula at r = 1e-6 for the Matern kinds."""
        if not isinstance(kind, str) or kind.lower() not in _lib.KERNELS:
            raise ValueError("kernel %r: the dense path knows 'rbf', 'matern32' and 'matern52'" % (kind,))
        X1 = as_f64(X1)
        D = X1.shape[1]
        X2a = X1 if X2 is None else as_f64(X2)
        ell = as_f64(ell).reshape(-1)
        if ell.size == 1:
            ell = np.full(D, float(ell[0]))
        out = np.zeros((X1.shape[0], X2a.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_kern_K(self.ctx, _lib.KERNELS[kind.lower()], ptr(X1), X1.shape[0], None if X2 is None else ptr(X2a),
                                                         X2a.shape[0], D, ptr(ell), float(np.squeeze(var)), ptr(out)))
        return out

    # ---- Kronecker (space x time) variant -------------------------------------------------------
    @staticmethod
    def _pack_kron(p, tags=('f', 'g')):
        """p: Zf/Zg = [Z0 (M0,D0), Z1 (M1,D1)], ell_f/ell_g = [l0, l1], var_f/var_g = [v0, v1], u_* (M0*M1), noise."""
        keep = {}
        s = _lib.zigp_kron_params()

        def ell(v, D):
            v = as_f64(v).reshape(-1)
            if v.size == 1:
                v = np.full(D, float(v[0]))
            if v.size != D:
                raise ValueError('lengthscales must be scalar or match the factor dimension')
            return np.ascontiguousarray(v)

        dims = None
        for tag in tags:
            Z0, Z1 = as_f64(p['Z' + tag][0]), as_f64(p['Z' + tag][1])
            if Z0.ndim != 2 or Z1.ndim != 2:
                raise ValueError('factor inducing inputs must be 2-D')
            if dims is None:
                dims = (Z0.shape[1], Z1.shape[1])
            elif dims != (Z0.shape[1], Z1.shape[1]):
                raise ValueError('f and g factors must act on the same input columns')
            M0, M1 = Z0.shape[0], Z1.shape[0]
            l0, l1 = ell(p['ell_' + tag][0], dims[0]), ell(p['ell_' + tag][1], dims[1])
            um = as_f64(p['u_%sm' % tag]).reshape(-1)
            us = as_f64(p['u_%ss_sqrt' % tag]).reshape(-1)
            if um.size != M0 * M1 or us.size != M0 * M1:
                raise ValueError('u_%sm / u_%ss_sqrt must have M0*M1 entries' % (tag, tag))
            keep[tag] = (Z0, Z1, l0, l1, um, us)
            setattr(s, 'M0' + tag, M0); setattr(s, 'M1' + tag, M1)
            setattr(s, 'Z0' + tag, ptr(Z0)); setattr(s, 'Z1' + tag, ptr(Z1))
            setattr(s, 'ell0' + tag, ptr(l0)); setattr(s, 'ell1' + tag, ptr(l1))
            setattr(s, 'var0' + tag, _scalar(p['var_' + tag][0])); setattr(s, 'var1' + tag, _scalar(p['var_' + tag][1]))
            setattr(s, 'u_%sm' % tag, ptr(um)); setattr(s, 'u_%ss_sqrt' % tag, ptr(us))
        s.D0, s.D1 = dims
        s.noise = _scalar(p.get('noise', 1.0))
        return s, keep, dims

    @staticmethod
    def _kron_rows(X, dims, name='X'):
        """the rows of a Kronecker call as float64 (N, D0 + D1)"""
        X = as_f64(X)
        if X.ndim != 2 or X.shape[1] != dims[0] + dims[1]:
            raise ValueError('%s must be (N,%d)' % (name, dims[0] + dims[1]))
        return X

    @classmethod
    def _kron_xy(cls, X, Y, rows, dims):
        """(X, Y) of an explicit host minibatch, checked; (None, None) with rows=(lo, hi) of the resident data set -- not both"""
        if rows is None:
            X = cls._kron_rows(X, dims)
            Y = as_f64(Y).reshape(-1)
            if Y.size != X.shape[0]:
                raise ValueError('Y must have N entries')
            return X, Y
        if X is not None or Y is not None:
            raise ValueError('pass either (X, Y) or rows=(lo, hi), not both')
        return None, None

    def _kron_fit_call(self, fn, lead, x, m, v, t0, row_begin, batch, jitter, scale, Xw, Yw, include_kl):
        """The part kron_fit_steps and kron_head_fit_steps share: fn is the library's entry point, lead its arguments between the
        context and the free state (the shape and options structs, the head's likelihood)."""
        for a in (x, m, v):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 1 and a.size == x.size):
                raise ValueError('x, m, v must be contiguous float64 vectors of one length')
        rb = np.ascontiguousarray(np.asarray(row_begin, dtype=np.int64))
        n = rb.size
        xw = yw = None
        if Xw is not None:
            xw, yw = as_f64(Xw), as_f64(Yw).reshape(-1)
            if xw.ndim != 2 or xw.shape[0] % int(batch) or yw.size != xw.shape[0]:
                raise ValueError('Xw must hold whole batches of `batch` rows, Yw one value per row')
            if rb.min() < -(xw.shape[0] // int(batch)):
                raise ValueError('row_begin refers to a host batch beyond Xw')
        elif n and rb.min() < 0:
            raise ValueError('negative row_begin needs Xw, Yw')
        ed, kl = np.zeros(n), np.zeros(n)
        rc = fn(self.ctx, *lead, ptr(x), ptr(m), ptr(v), x.size, int(t0), n, rb.ctypes.data, int(batch),
                ptr(xw) if xw is not None else None, ptr(yw) if yw is not None else None, float(jitter), float(scale),
                1 if include_kl else 0, ptr(ed), ptr(kl))
        try:
            _check(self.lib, self.ctx, rc)
        except ZigpError as e:
            # include/zigp.h: after a failure x / m / v hold the state before the failing step and the history from that step on is NaN --
            # the caller learns how many updates WERE applied (its iteration count and Adam's bias correction depend on it) and gets the
            # history of those steps
            # (the count comes from the library -- zigp_kron_fit_steps_applied, one counter for both loops; the first non-finite history
            # entry is NOT it: an applied step can itself have a non-finite ELBO at extreme parameters)
            done = max(0, min(n, int(self.lib.zigp_kron_fit_steps_applied(self.ctx))))
            e.steps_applied = done
            e.elbo_data, e.kl = ed[:done].copy(), kl[:done].copy()
            raise
        return ed, kl

    def kron_elbo(self, p, X=None, Y=None, jitter=1e-5, scale=1.0, g_offset=0.0, include_kl=True, need_grad=True, rows=None, f_mu=None):
        """One Kronecker ELBO (step); returns (elbo_data, kl, grads or None).  Either an explicit host minibatch (X, Y), as
        scripts/onoff.py:377-381 feeds it, or rows=(lo, hi) of the resident data set (set_data / set_data_device).
        f_mu: the optional constant added to fmean (scripts/onoff.py:161,168-169); when given, grads['f_mu'] is its gradient."""
        s, keep, dims = self._pack_kron(p)
        self._set_kron_kinds(p)
        X, Y = self._kron_xy(X, Y, rows, dims)
        ed, kl, dmu = C.c_double(0), C.c_double(0), C.c_double(0)
        fmu = 0.0 if f_mu is None else _scalar(f_mu)
        g, gs = None, None
        if need_grad:
            g = {}
            gs = _lib.zigp_kron_grads()
            # one allocation for the twelve gradient arrays (views into it): np.zeros_like twelve times is 6 us of a 190 us call
            sizes = [a.size for tag in ('f', 'g') for a in keep[tag]]
            flat = np.zeros(sum(sizes))
            o = 0
            for tag in ('f', 'g'):
                Z0, Z1, l0, l1, um, us = keep[tag]
                arrs = {}
                for name, a in (('Z0', Z0), ('Z1', Z1), ('ell0', l0), ('ell1', l1), ('um', um), ('us', us)):
                    arrs[name] = flat[o:o + a.size].reshape(a.shape); o += a.size
                g[tag] = arrs
                setattr(gs, 'Z0' + tag, ptr(arrs['Z0'])); setattr(gs, 'Z1' + tag, ptr(arrs['Z1']))
                setattr(gs, 'ell0' + tag, ptr(arrs['ell0'])); setattr(gs, 'ell1' + tag, ptr(arrs['ell1']))
                setattr(gs, 'u_%sm' % tag, ptr(arrs['um'])); setattr(gs, 'u_%ss_sqrt' % tag, ptr(arrs['us']))
        gref = C.byref(gs) if gs is not None else None
        if rows is None:
            rc = self.lib.zigp_kron_elbo(self.ctx, C.byref(s), ptr(X), ptr(Y), X.shape[0], float(jitter), float(scale), float(g_offset), fmu,
                                         1 if include_kl else 0, C.byref(ed), C.byref(kl), gref, C.byref(dmu))
        else:
            rc = self.lib.zigp_kron_elbo_rows(self.ctx, C.byref(s), int(rows[0]), int(rows[1]), float(jitter), float(scale), float(g_offset), fmu,
                                              1 if include_kl else 0, C.byref(ed), C.byref(kl), gref, C.byref(dmu))
        _check(self.lib, self.ctx, rc)
        out = None
        if need_grad:
            out = dict(noise=gs.noise)
            if f_mu is not None:
                out['f_mu'] = dmu.value
            for tag in ('f', 'g'):
                a = g[tag]
                out['Z' + tag] = [a['Z0'], a['Z1']]
                out['ell_' + tag] = [a['ell0'], a['ell1']]
                out['var_' + tag] = [getattr(gs, 'var0' + tag), getattr(gs, 'var1' + tag)]
                out['u_%sm' % tag] = a['um']
                out['u_%ss_sqrt' % tag] = a['us']
        return ed.value, kl.value, out

    def kron_fit_steps(self, shape, x, m, v, lr, positive, t0, row_begin, batch, jitter=1e-5, scale=1.0, Xw=None, Yw=None,
                       beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        """n = len(row_begin) Adam steps of the Kronecker on/off fit ON THE DEVICE (zigp_kron_fit_steps; the loop body of
        scripts/onoff.py:375-381): one synchronisation for the whole call.
        shape: dict(M0f, M1f, M0g, M1g, D0, D1); x, m, v: float64 [n_free] free state and Adam moments, UPDATED IN PLACE, in the block
        order of include/zigp.h (per latent Z0, Z1, u, s, ell0, ell1, var0, var1; then the noise variance); lr, positive: 17 per-block
        learning rates / Log1pe flags; t0: iterations done so far; row_begin[i] >= 0: rows of the resident data set, -(1 + k): batch k of
        the host arrays (Xw, Yw).  Returns (elbo_data[n], kl[n]) -- the history, each at the parameters before that step's update."""
        self._kron_fit_kinds('kron_fit_steps', shape, ('f', 'g'))
        s = _lib.zigp_kron_params()
        for k in ('M0f', 'M1f', 'M0g', 'M1g', 'D0', 'D1'):
            setattr(s, k, int(shape[k]))
        o = _lib.zigp_kron_fit_opts()
        for b in range(_lib.FIT_BLOCKS):
            o.lr[b] = float(lr[b]); o.positive[b] = int(bool(positive[b]))
        o.beta1, o.beta2, o.eps = float(beta1), float(beta2), float(eps)
        return self._kron_fit_call(self.lib.zigp_kron_fit_steps, (C.byref(s), C.byref(o)), x, m, v, t0, row_begin, batch, jitter, scale, Xw, Yw,
                                   include_kl)

    def kron_stepper(self, p):
        """A prepared Kronecker step for a FIXED model shape (the training loop: scripts/onoff.py:375-431 calls sess.run on one graph 50 000
        times): parameter buffers, the ctypes structs and the gradient arrays are set up once; a call copies the new parameter values in
        and returns views of its own gradient buffer (valid until the next call).  Same entry points, same numbers as kron_elbo."""
        return KronStepper(self, p)

    def kron_predict(self, p, Xnew, jitter=1e-6, g_offset=0.0, f_mu=None):
        """(9,N) in the order of build_predict (scripts/onoff.py:184); onofftf/onoffpred.py uses jitter 1e-6, g_offset -1."""
        s, keep, dims = self._pack_kron(p)
        self._set_kron_kinds(p)
        Xnew = self._kron_rows(Xnew, dims, 'Xnew')
        out = np.zeros((9, Xnew.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_kron_predict(self.ctx, C.byref(s), ptr(Xnew), Xnew.shape[0], float(jitter),
                                                               float(g_offset), 0.0 if f_mu is None else _scalar(f_mu), ptr(out)))
        return out

    LIK = {'gaussian': _lib.LIK_GAUSSIAN, 'bernoulli': _lib.LIK_BERNOULLI}

    def kron_head_elbo(self, p, X=None, Y=None, lik=None, jitter=1e-5, scale=1.0, f_mu=0.0, include_kl=True, need_grad=True, rows=None):
        """Single-latent Kronecker SVGP bound with a 'gaussian' (scripts/svgp.py, hurdle.py) or 'bernoulli'
        (scripts/classifier.py) head.  p holds the f fields only (Zf, ell_f, var_f, u_fm, u_fs_sqrt[, noise]).  Either an explicit host
        minibatch (X, Y) or rows=(lo, hi) of the resident data set (set_data / set_data_device; zigp_kron_head_elbo_rows).
        Returns (elbo_data, kl, grads or None); grads has the f keys, 'noise' and 'f_mu'."""
        s, keep, dims = self._pack_kron(p, tags=('f',))
        self._set_kron_kinds(p, ('f',))
        X, Y = self._kron_xy(X, Y, rows, dims)
        ed, kl, dmu = C.c_double(0), C.c_double(0), C.c_double(0)
        gs, a = None, None
        if need_grad:
            gs = _lib.zigp_kron_grads()
            Z0, Z1, l0, l1, um, us = keep['f']
            a = dict(Z0=np.zeros_like(Z0), Z1=np.zeros_like(Z1), ell0=np.zeros_like(l0), ell1=np.zeros_like(l1),
                     um=np.zeros_like(um), us=np.zeros_like(us))
            gs.Z0f, gs.Z1f, gs.ell0f, gs.ell1f = ptr(a['Z0']), ptr(a['Z1']), ptr(a['ell0']), ptr(a['ell1'])
            gs.u_fm, gs.u_fs_sqrt = ptr(a['um']), ptr(a['us'])
        gref = C.byref(gs) if gs is not None else None
        if rows is None:
            rc = self.lib.zigp_kron_head_elbo(self.ctx, C.byref(s), self.LIK[lik], ptr(X), ptr(Y), X.shape[0], float(jitter), float(scale),
                                              float(f_mu), 1 if include_kl else 0, C.byref(ed), C.byref(kl), gref, C.byref(dmu))
        else:
            rc = self.lib.zigp_kron_head_elbo_rows(self.ctx, C.byref(s), self.LIK[lik], int(rows[0]), int(rows[1]), float(jitter), float(scale),
                                                   float(f_mu), 1 if include_kl else 0, C.byref(ed), C.byref(kl), gref, C.byref(dmu))
        _check(self.lib, self.ctx, rc)
        out = None
        if need_grad:
            out = dict(noise=gs.noise, f_mu=dmu.value, Zf=[a['Z0'], a['Z1']], ell_f=[a['ell0'], a['ell1']], var_f=[gs.var0f, gs.var1f],
                       u_fm=a['um'], u_fs_sqrt=a['us'])
        return ed.value, kl.value, out

    def kron_head_fit_steps(self, shape, lik, x, m, v, lr, positive, trainable, t0, row_begin, batch, jitter=1e-5, scale=1.0, Xw=None, Yw=None,
                            beta1=0.9, beta2=0.999, eps=1e-8, include_kl=True):
        """n = len(row_begin) Adam steps of a single-latent head fit ON THE DEVICE (zigp_kron_head_fit_steps; the loop bodies of
        scripts/svgp.py:289-330 and classifier.py:276-316): one synchronisation for the whole call.  The single-latent twin of
        kron_fit_steps -- shape: dict(M0f, M1f, D0, D1); lik: 'gaussian' or 'bernoulli'; x, m, v: float64 [n_free], UPDATED IN PLACE, in
        the block order Z0, Z1, u, s, ell0, ell1, var0, var1, noise, f_mu; lr, positive, trainable: 10 per-block learning rates / Log1pe
        flags / 0 for a block that is not updated (an absent f_mu: free value 0; the classifier's noise).  row_begin, Xw, Yw and the
        return value (elbo_data[n], kl[n]) as kron_fit_steps; so are the exceptions, and what NotPositiveDefiniteError carries."""
        if lik not in self.LIK:
            raise ValueError("kron_head_fit_steps: lik must be 'gaussian' or 'bernoulli', not %r (the on/off fit is kron_fit_steps)" % (lik,))
        self._kron_fit_kinds('kron_head_fit_steps', shape, ('f',))
        s = _lib.zigp_kron_params()
        for k in ('M0f', 'M1f', 'D0', 'D1'):
            setattr(s, k, int(shape[k]))
        o = _lib.zigp_kron_head_fit_opts()
        for b in range(_lib.HEAD_FIT_BLOCKS):
            o.lr[b] = float(lr[b]); o.positive[b] = int(bool(positive[b])); o.trainable[b] = int(bool(trainable[b]))
        o.beta1, o.beta2, o.eps = float(beta1), float(beta2), float(eps)
        return self._kron_fit_call(self.lib.zigp_kron_head_fit_steps, (C.byref(s), self.LIK[lik], C.byref(o)), x, m, v, t0, row_begin, batch,
                                   jitter, scale, Xw, Yw, include_kl)

    def kron_head_predict(self, p, Xnew, lik, jitter=1e-6, f_mu=0.0):
        """(4,N): fmean, fvar, pfmean, pfvar (onofftf/svgppred.py:180-186, onofftf/svcppred.py 'pfmean'/'pfvar')."""
        s, keep, dims = self._pack_kron(p, tags=('f',))
        self._set_kron_kinds(p, ('f',))
        Xnew = self._kron_rows(Xnew, dims, 'Xnew')
        out = np.zeros((4, Xnew.shape[0]))
        _check(self.lib, self.ctx, self.lib.zigp_kron_head_predict(self.ctx, C.byref(s), self.LIK[lik], ptr(Xnew), Xnew.shape[0],
                                                                    float(jitter), float(f_mu), ptr(out)))
        return out

    # ---- measurement ----
    def set_overlap(self, on=True):
        """stream overlap inside elbo(): True/1 (the library's DEFAULT since round 3) runs the side kernels of a chunk (kgrad, the next
        chunk's Kuf panels) on a second stream under its rank-N updates; False/0 keeps every launch on one stream -- set this for
        per-kernel timing with an external tracer (rocprofv3), where overlapped kernels stretch each other.  Results are bit-identical
        either way."""
        _check(self.lib, self.ctx, self.lib.zigp_set_overlap(self.ctx, int(on)))

    def set_kron_panels(self, on=True):
        """diagnostic: route the Kronecker entry points through the GEMM-panel path also for grids the fused kernels cover"""
        _check(self.lib, self.ctx, self.lib.zigp_set_kron_panels(self.ctx, 1 if on else 0))

    def set_kron_range_tiles(self, tiles=1024):
        """diagnostic: rows per range (in 16-point tiles) of the larger-grid Kronecker gradient step; results do not depend on it"""
        _check(self.lib, self.ctx, self.lib.zigp_set_kron_range_tiles(self.ctx, int(tiles)))

    def profile_enable(self, on=True):
        _check(self.lib, self.ctx, self.lib.zigp_profile_enable(self.ctx, 1 if on else 0))

    def clock_stamp(self):
        """{XCC id: (shader-clock counter, 100 MHz counter)} taken in stream order now (zigp_clock_stamp); see clock_mhz"""
        out = np.zeros(24, dtype=np.int64)
        _check(self.lib, self.ctx, self.lib.zigp_clock_stamp(self.ctx, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return {int(out[3 * i]): (int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(8)}

    @staticmethod
    def clock_mhz(a, b):
        """sustained shader clock (MHz) between two clock_stamp() results: median over the XCDs both stamps saw; None if the counters
        do not behave as a core-clock / constant-clock pair on this device"""
        vals = []
        for x in a:
            # a region shorter than 20 ms of the constant 100 MHz counter says nothing about a SUSTAINED clock (a 4 ms region once read 3.8 GHz
            # on a chip that tops out at 2.4: the two counters are sampled by a one-wave kernel a few microseconds apart)
            if x in b and b[x][1] - a[x][1] >= 2000000:
                vals.append((b[x][0] - a[x][0]) / ((b[x][1] - a[x][1]) / 1e8) / 1e6)
        if not vals:
            return None
        v = float(np.median(vals))
        return v if 300.0 < v < 3000.0 else None

    def profile_sampling(self, every=8):
        """every=1 times every launch of the chunk loop (exact sums); n > 1 samples every n-th full-size chunk"""
        _check(self.lib, self.ctx, self.lib.zigp_profile_sampling(self.ctx, int(every)))

    def profile_reset(self):
        _check(self.lib, self.ctx, self.lib.zigp_profile_reset(self.ctx))

    def profile_get(self):
        ms = np.zeros(_lib.NCLASS)
        n = np.zeros(_lib.NCLASS, dtype=np.int64)
        fl = np.zeros(_lib.NCLASS)
        tot = np.zeros(_lib.NCLASS, dtype=np.int64)
        _check(self.lib, self.ctx, self.lib.zigp_profile_get(self.ctx, ptr(ms), n.ctypes.data_as(C.POINTER(C.c_int64)), ptr(fl)))
        _check(self.lib, self.ctx, self.lib.zigp_profile_totals(self.ctx, tot.ctypes.data_as(C.POINTER(C.c_int64))))
        # ms / launches / flops: the TIMED (sampled) launches; total_launches: all of them; est_total_ms = avg * total
        return {name: dict(ms=float(ms[i]), launches=int(n[i]), flops=float(fl[i]), total_launches=int(tot[i]),
                           est_total_ms=float(ms[i]) / max(int(n[i]), 1) * int(tot[i]))
                for i, name in enumerate(_lib.PROF_CLASSES)}

    # ---- diagnostics ----
    def test_gemm(self, A, B, transA=False, transB=False):
        A, B = as_f64(A), as_f64(B)
        m, k = (A.shape[1], A.shape[0]) if transA else A.shape
        n = B.shape[0] if transB else B.shape[1]
        out = np.zeros((m, n))
        _check(self.lib, self.ctx, self.lib.zigp_test_gemm(self.ctx, int(transA), int(transB), m, n, k, ptr(A), ptr(B), ptr(out)))
        return out

    def test_kuf(self, X, Z, ell, var):
        """K (M,N) = kern.K(Z, X) as the chunk loop's k_kuf_build writes a Kuf panel (hand-written exponential)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        N, D = X.shape
        M = Z.shape[0]
        ell = as_f64(np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)))
        out = np.zeros((M, N))
        _check(self.lib, self.ctx, self.lib.zigp_test_kuf(self.ctx, N, M, D, ptr(X), ptr(Z), ptr(ell), float(var), ptr(out)))
        return out

    def test_kuf_kind(self, kind, X, Z, ell, var, grad=True):
        """(K, K') as a call with kernel `kind` on the latent builds its Kuf panel (zigp_test_kuf_kind): both (Mp16, N) with Mp16 = M
        rounded up to 16, the padded rows included (zeros); K' = -dk / d(r2 / 2) is the derivative panel of a gradient step (None with
        grad=False, where the launch is the value-only one)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        N, D = X.shape
        M = Z.shape[0]
        Mp16 = (M + 15) // 16 * 16
        ell = as_f64(np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)))
        K = np.zeros((Mp16, N))
        Kd = np.zeros((Mp16, N)) if grad else None
        _check(self.lib, self.ctx, self.lib.zigp_test_kuf_kind(self.ctx, _lib.KERNELS[kind], N, M, D, ptr(X), ptr(Z), ptr(ell), float(var), ptr(K),
                                                                None if Kd is None else ptr(Kd)))
        return K, Kd

    def test_kgrad_kind(self, kind, Jp, K, Kd, alpha, gm, gv, X, Z, n0=0, krow=None):
        """test_kgrad for a kernel kind (zigp_test_kgrad_kind): the moment columns are taken with F Kd, columns 0 and 1 + 2D with K."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        M, D = Z.shape
        K = as_f64(K)
        Nc = K.shape[1]
        K, Kd, Jp = as_f64(K, (M, Nc)), as_f64(Kd, (M, Nc)), as_f64(Jp, (M, Nc))
        alpha, gm, gv = as_f64(alpha, (M,)), as_f64(gm, (Nc,)), as_f64(gv, (Nc,))
        out = np.zeros((_lib.KG_SPLIT, M, 2 + 2 * D)) if krow is None else np.array(as_f64(krow, (_lib.KG_SPLIT, M, 2 + 2 * D)), copy=True)
        _check(self.lib, self.ctx, self.lib.zigp_test_kgrad_kind(self.ctx, _lib.KERNELS[kind], M, D, Nc, X.shape[0], int(n0), ptr(Jp), ptr(K), ptr(Kd),
                                                                  ptr(alpha), ptr(gm), ptr(gv), ptr(X), ptr(Z), ptr(out)))
        return out

    def test_potrf_trtri(self, A, split_k=False):
        A = as_f64(A)
        n = A.shape[0]
        L, W = np.zeros((n, n)), np.zeros((n, n))
        _check(self.lib, self.ctx, self.lib.zigp_test_potrf_trtri(self.ctx, n, ptr(A), ptr(L), ptr(W), int(bool(split_k))))
        return L, W

    def test_potrf_stages(self, A, split_k=False, snapshots=True):
        """The blocked Cholesky + inverse of ONE (n,n) matrix through potrf_trtri_jobs itself, tapped (zigp_test_potrf_stages).  Returns
        dict(L, W, T: the whole padded [Mp][Mp] images; T holds _lib.STAGE_SENTINEL where no launch wrote), Mp, nb, info (0 or the 1-based
        failing pivot), launches: a list of dict(kind in _lib.PSL_KINDS, idx (block column j / doubling distance b), tiles, S (split-K slices;
        0: one workgroup per tile), npan, snap: the [Mp][Mp] images copied right behind the launch -- diag: (L, W); panel, trail: (L,);
        tri1: (T,); tri2: (W,) -- or () without snapshots).  A failed factorisation raises NotPositiveDefiniteError with this dict as
        its `.stages` attribute (zigp_last_info holds the pivot)."""
        A = as_f64(A)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError('test_potrf_stages: A must be square')
        n = A.shape[0]
        Mp = max(1, (n + 127) // 128) * 128
        nb = Mp // 128
        launches = nb + 2 * (nb - 1) + 2 * max(0, (nb - 1).bit_length())
        out = dict(L=np.zeros((Mp, Mp)), W=np.zeros((Mp, Mp)), T=np.zeros((Mp, Mp)))
        snap = np.zeros((launches + nb, Mp, Mp)) if snapshots else None
        facts = np.zeros(_lib.PSF_REC + _lib.PSF_PER * launches, dtype=np.int64)
        a = _lib.zigp_stage_potrf(n=n, split_k=int(bool(split_k)), A=ptr(A), L=ptr(out['L']), W=ptr(out['W']), T=ptr(out['T']),
                                  snap=None if snap is None else ptr(snap), snap_cap=0 if snap is None else snap.shape[0],
                                  facts=facts.ctypes.data_as(C.POINTER(C.c_int64)), facts_cap=facts.size)
        rc = self.lib.zigp_test_potrf_stages(self.ctx, C.byref(a))
        if rc not in (0, _lib.ZIGP_ENOTPD):
            _check(self.lib, self.ctx, rc)
        out.update(Mp=int(facts[0]), nb=int(facts[1]), info=int(facts[4]), launches=[])
        for k in range(int(facts[2])):
            kind, idx, tiles, S, npan, first = (int(v) for v in facts[_lib.PSF_REC + _lib.PSF_PER * k:_lib.PSF_REC + _lib.PSF_PER * (k + 1)])
            imgs = () if first < 0 else tuple(snap[first + i] for i in range(2 if kind == 0 else 1))
            out['launches'].append(dict(kind=_lib.PSL_KINDS[kind], idx=idx, tiles=tiles, S=S, npan=npan, snap=imgs))
        if rc != 0:
            try:
                _check(self.lib, self.ctx, rc)
            except NotPositiveDefiniteError as e:
                e.stages = out
                raise
        return out

    # ---- stage diagnostics (include/zigp_diag.h): one chunk's stage through the chunk loop's own functions ----
    def test_chunk_forward(self, lat_f, lat_g, Nc, need_grad, only=None, whiten=False):
        """Forward products of one chunk.  lat_*: dict(M=..., W=(M,M) lower, v=(M), s2=(M), K=(M,Nc), Rt=(M,M) in gradient mode); the latent
        that does not run (only = 0 / 1) needs M alone.  Returns ([out_f, out_g], facts): out = dict(A1, Jp or None, part [3][Mp/32][Nc]
        with rows nothing wrote at _lib.STAGE_SENTINEL) or None, facts = dict(paired, tail_f, tail_g, Mp, np, np1, np2).
        whiten: the launches of a whitened call (zigp_test_chunk_forward_white): v / s2 are the weights of the mean / variance sums (planes 0
        and 2), Rt the factor image D W of J' = Rt^T A; without need_grad no A panel is stored (A1 is None)."""
        Nc = int(Nc)
        arr = (_lib.zigp_stage_latent * 2)()
        keep, outs = [], []
        for h, q in enumerate((lat_f, lat_g)):
            M = int(q['M'])
            arr[h].M = M
            if only is not None and only != h:
                outs.append(None)
                continue
            Mp = (M + 127) // 128 * 128
            ins = dict(W=as_f64(q['W'], (M, M)), v=as_f64(q['v'], (M,)), s2=as_f64(q['s2'], (M,)), K=as_f64(q['K'], (M, Nc)))
            if need_grad:
                ins['Rt'] = as_f64(q['Rt'], (M, M))
            out = dict(A1=np.zeros((M, Nc)) if need_grad or not whiten else None, Jp=np.zeros((M, Nc)) if need_grad else None,
                       part=np.zeros((3, Mp // 32, Nc)))
            for k, a in list(ins.items()) + [(k, a) for k, a in out.items() if a is not None]:
                setattr(arr[h], k, ptr(a))
            keep.append(ins)
            outs.append(out)
        facts = (C.c_int64 * 12)()
        fn = self.lib.zigp_test_chunk_forward_white if whiten else self.lib.zigp_test_chunk_forward
        _check(self.lib, self.ctx, fn(self.ctx, Nc, int(bool(need_grad)), -1 if only is None else int(only), arr, facts))
        f = list(facts)
        return outs, dict(paired=f[0], tail_f=f[1], tail_g=f[2], Mp=(f[3], f[4]), np=(f[5], f[6]), np1=(f[7], f[9]), np2=(f[8], f[10]))

    def test_latents_forward(self, p, jitter=1e-6, need_grad=True):
        """What the M x M forward of the context's parametrisation leaves (p['whiten'] as in elbo; a full-covariance p is refused):
        [dict for f, g] with the keys of _lib.FWD_OUTS -- W, L, Kuu, Wt, kl always; unwhitened: v, alpha, dkinv and with need_grad Rt, P, Qt,
        Wp = W diag(s^2); whitened: wh (3, M) = (s^2 - 1, u, 1) and with need_grad alpha = W^T u, Wp = D W.  Anything else is None."""
        self._set_modes(p)
        pk = _Packed(p)
        white = bool(p.get('whiten', False))
        made = {'W', 'L', 'Kuu', 'Wt', 'kl'} | ({'wh'} if white else {'v', 'alpha', 'dkinv'})
        if need_grad:
            made |= {'alpha', 'Wp'} if white else {'Rt', 'P', 'Qt', 'Wp'}
        outs, arrs = [], []
        for M in (pk.Mf, pk.Mg):
            shape = dict(v=(M,), alpha=(M,), dkinv=(M,), kl=(1,), wh=(3, M))
            o = {k: np.zeros(shape.get(k, (M, M))) if k in made else None for k in _lib.FWD_OUTS}
            outs.append(o)
            arrs.append((_lib.dp * len(_lib.FWD_OUTS))(*[None if o[k] is None else ptr(o[k]) for k in _lib.FWD_OUTS]))
        _check(self.lib, self.ctx, self.lib.zigp_test_latents_forward(self.ctx, C.byref(pk.struct), float(jitter), int(bool(need_grad)), arrs[0], arrs[1]))
        for o in outs:
            o['kl'] = float(o['kl'][0])
        return outs

    def test_dense_pack(self, lat_f, lat_g, pw, D, mode='diag', need_grad=True, include_kl=True, mean_on=False):
        """The call's result vector from the stages' accumulators (zigp_test_dense_pack).  lat_*: dict(krow [4][M][2+2D], du (M), dsq (M), s (M)
        -- mode 'white_full': dLq (M,M) instead of dsq and s --, kl_vec1 (M), kl_vec2 (M), ell (D), var, kl); pw [blocks][PW_ACC].
        Returns dict(data, kl, var_f, var_g, noise, mean_b, mean_a (8), f = dict(dZ, du, ds, dell), g = ..., packed)."""
        pw = as_f64(pw)
        a = _lib.zigp_stage_pack()
        a.D, a.mode, a.need_grad, a.include_kl, a.mean_on, a.pw_blocks = int(D), _lib.MXM_MODES.index(mode), int(bool(need_grad)), int(bool(include_kl)), int(bool(mean_on)), pw.shape[0]
        a.pw = ptr(pw)
        full = mode == 'white_full'
        keep, n, Ms = [], 16, []
        for h, q in enumerate((lat_f, lat_g)):
            M = int(np.asarray(q['kl_vec1']).size)
            Ms.append(M)
            a.lat[h].M, a.lat[h].var, a.lat[h].kl = M, float(q.get('var', 1.0)), float(q.get('kl', 0.0))
            shapes = dict(krow=(_lib.KG_SPLIT, M, 2 + 2 * D), du=(M,), dsq=(M,), s=(M,), dLq=(M, M), kl_vec1=(M,), kl_vec2=(M,), ell=(D,))
            for k, shape in shapes.items():
                if q.get(k) is not None:
                    x = as_f64(q[k], shape)
                    keep.append(x)
                    setattr(a.lat[h], k, ptr(x))
            if need_grad:
                n += M * D + M + (M * M if full else M) + D
        out = np.zeros(n)
        a.out, a.n_out = ptr(out), n
        _check(self.lib, self.ctx, self.lib.zigp_test_dense_pack(self.ctx, C.byref(a)))
        res = dict(data=out[0], kl=out[1], var_f=out[2], var_g=out[3], noise=out[4], mean_b=out[5], mean_a=out[6:14].copy(), packed=out)
        if need_grad:
            off = 16
            for tag, M in zip('fg', Ms):
                ns = M * M if full else M
                res[tag] = dict(dZ=out[off:off + M * D].reshape(M, D), du=out[off + M * D:off + M * D + M],
                                ds=out[off + M * D + M:off + M * D + M + ns].reshape((M, M) if full else (M,)),
                                dell=out[off + M * D + M + ns:off + M * D + M + ns + D])
                off += M * D + M + ns + D
        return res

    def test_pointwise(self, mode, part_f, part_g, np1, np2, X, Y, n0, row_end, var_f, var_g, noise, g_offset=0.0, scale=1.0,
                       mean=None, repeat=1, acc=None, whiten=False, head=None):
        """The point-wise stage of one chunk.  mode 'value' / 'grad' / 'predict'; part_* [3][np][Nc]; np1 / np2 = (f, g) rows to add of planes
        0, 1 / of plane 2; mean = None or (a (D), b); whiten: the launch of a whitened call (mean = plane 0, var = var_* + plane 2 in every mode).  Returns dict(gm_f, gv_f, gm_g, gv_g (grad), acc [Nc/64][PW_ACC], out9 (predict)).
        head = 'gaussian' / 'bernoulli': the head's kernel instead (zigp_test_pointwise_head) -- part_g may be None, np1 / np2 are the f
        counts (or pairs whose second entry is ignored), out9 is the head's (4, row_end) block."""
        part_f = as_f64(part_f)
        if head is not None:
            lik = self._head_lik('test_pointwise', head)
            part_g = np.zeros((3, 1, part_f.shape[2])) if part_g is None else part_g
            np1, np2 = [(int(v), 0) if np.isscalar(v) else v for v in (np1, np2)]
        part_g = as_f64(part_g)
        X = as_f64(X)
        if X.ndim == 1: X = X[:, None]
        Nc = part_f.shape[2]
        s = _lib.zigp_stage_pointwise()
        s.mode = {'value': 0, 'grad': 1, 'predict': 2}[mode]
        s.repeat = int(repeat)
        s.np_f, s.np_g = part_f.shape[1], part_g.shape[1]
        s.np1_f, s.np1_g = int(np1[0]), int(np1[1])
        s.np2_f, s.np2_g = int(np2[0]), int(np2[1])
        s.D, s.mean_on = X.shape[1], 0 if mean is None else 1
        if mean is not None:
            a = np.zeros(8)
            a[:X.shape[1]] = np.asarray(mean[0], dtype=np.float64).reshape(-1)
            s.mean_a = (C.c_double * 8)(*a)
            s.mean_b = float(mean[1])
        Yc = None if Y is None else as_f64(Y).reshape(-1)
        s.part_f, s.part_g, s.X, s.Y = ptr(part_f), ptr(part_g), ptr(X), None if Yc is None else ptr(Yc)
        s.Nrows, s.n0, s.row_end, s.Nc = X.shape[0], int(n0), int(row_end), Nc
        s.var_f, s.var_g, s.noise, s.g_offset, s.scale = float(var_f), float(var_g), float(noise), float(g_offset), float(scale)
        out = dict(acc=np.zeros((Nc // _lib.PW_PTS, _lib.PW_ACC)) if acc is None else np.array(as_f64(acc), copy=True))
        s.acc = ptr(out['acc'])
        if mode == 'grad':
            for k in ('gm_f', 'gv_f', 'gm_g', 'gv_g'):
                out[k] = np.zeros(Nc)
                setattr(s, k, ptr(out[k]))
        if mode == 'predict':
            out['out9'] = np.zeros((4 if head is not None else 9, int(row_end)))
            s.out9 = ptr(out['out9'])
        if head is not None:
            _check(self.lib, self.ctx, self.lib.zigp_test_pointwise_head(self.ctx, lik, 1 if whiten else 0, C.byref(s)))
            return out
        fn = self.lib.zigp_test_pointwise_white if whiten else self.lib.zigp_test_pointwise
        _check(self.lib, self.ctx, fn(self.ctx, C.byref(s)))
        return out

    # ---- Kronecker stage diagnostics (include/zigp_diag.h): one launch of a point-wise or per-point panel kernel ----
    def test_kron_pointwise(self, lik, mode, part_f, part_g=None, Y=None, N=None, var_f=(1.0, 1.0), var_g=(1.0, 1.0), noise=1.0, g_offset=0.0,
                            f_offset=0.0, scale=1.0, dev_hyp=False, sentinel_out=True, ld_out=None):
        """The point-wise launch of a Kronecker call (zigp_test_kron_pointwise).  lik 'onoff' / 'gaussian' / 'bernoulli'; mode 'value' / 'grad' /
        'predict'; part_* [4][Nc] = q0, q1, mean, st (Nc a multiple of 256; part_g: OnOff only); N valid points (default: len(Y)); var_* =
        (var0, var1) of the latent's two factors.  dev_hyp: Knn, the noise and (heads) f_offset are read from the device hyperparameter block.
        Returns, for 'value' / 'grad', dict(gm_f, gv_f, dq0_f, dq1_f, gm_g, gv_g, dq0_g, dq1_g [Nc] each, acc [Nc/256][5]) -- with
        sentinel_out a buffer the launch did not write holds _lib.STAGE_SENTINEL --, for 'predict' dict(out [9 or 4][ld_out]), ld_out >= N
        (default N, as the real calls)."""
        part_f = as_f64(part_f)
        Nc = part_f.shape[1]
        part_f = as_f64(part_f, (4, Nc))
        s = _lib.zigp_stage_kron_pointwise()
        s.lik = {'onoff': _lib.LIK_ONOFF, 'gaussian': _lib.LIK_GAUSSIAN, 'bernoulli': _lib.LIK_BERNOULLI}[lik]
        s.mode = {'value': 0, 'grad': 1, 'predict': 2}[mode]
        s.dev_hyp, s.sentinel_out = int(bool(dev_hyp)), int(bool(sentinel_out))
        Yc = None if Y is None else as_f64(Y).reshape(-1)
        N = int(Yc.size if N is None else N)
        s.N, s.Nc = N, Nc
        s.part_f = ptr(part_f)
        if part_g is not None:
            part_g = as_f64(part_g, (4, Nc))
            s.part_g = ptr(part_g)
        s.Y = None if Yc is None else ptr(Yc)
        s.var0f, s.var1f, s.var0g, s.var1g = float(var_f[0]), float(var_f[1]), float(var_g[0]), float(var_g[1])
        s.noise, s.g_offset, s.f_offset, s.scale = float(noise), float(g_offset), float(f_offset), float(scale)
        out = {}
        if mode == 'predict':
            ld = N if ld_out is None else int(ld_out)
            s.ld_out = ld
            out['out'] = np.zeros((9 if lik == 'onoff' else 4, ld))
            s.out = ptr(out['out'])
        else:
            for k in ('gm_f', 'gv_f', 'dq0_f', 'dq1_f', 'gm_g', 'gv_g', 'dq0_g', 'dq1_g'):
                out[k] = np.zeros(Nc)
                setattr(s, k, ptr(out[k]))
            out['acc'] = np.zeros((Nc // _lib.KPW_THREADS, _lib.KPW_ACC))
            s.acc = ptr(out['acc'])
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_pointwise(self.ctx, C.byref(s)))
        return out

    def test_kron_fused_step(self, p, X, Y, lik='onoff', jitter=1e-5, scale=1.0, g_offset=0.0, f_mu=0.0, include_kl=True, inject=None, taps=True):
        """One value-and-gradient step of the fused Kronecker path with its device buffers snapshot around the launches
        (zigp_test_kron_fused_step, include/zigp_diag.h, where every layout is written down).  p, X, Y as kron_elbo (lik 'onoff') or
        kron_head_elbo ('gaussian' / 'bernoulli': the f fields only).  inject: None, or one entry per latent, each None or [4][N] = gm, gv,
        dq0, dq1 copied over the point-wise kernel's cotangents before the backward launch.  taps=False: no snapshot at all.
        Returns dict(elbo_data, kl, grads (as kron_elbo / kron_head_elbo), facts {name: int}, lat [per latent: dict(K, P, PF, dvec, Zs, zc --
        lists over the two factors --, U, S2, T0, T1, Al, AlF, S2F, AlTF, S2TF, part, cot, work; of the finish stage, trimmed to what the kernels
        write: klv (5), gu, gs (M0, M1), krow [2] (M_p, 2 + 2 D_p); a step with a Matern factor: krow_first [2] and, small grids, Kd [2] (32, 128),
        work2, krow2 [2]; larger grids: G [2] -- (16 + Mq0, Mq0): G of factor 0 then the low words of Q2, and (Mq1, Mq1): P Q2 of factor 1; and
        each of klv, gu, gs, krow, krow_first, krow2, G once more as '<name>_cap': the whole region at its capacity size, where an element no kernel
        wrote holds _lib.STAGE_SENTINEL)])."""
        two = lik == 'onoff'
        tags = ('f', 'g') if two else ('f',)
        sp, keep, dims = self._pack_kron(p, tags=tags)
        X = as_f64(X)
        if X.ndim != 2 or X.shape[1] != dims[0] + dims[1]:
            raise ValueError('X must be (N,%d)' % (dims[0] + dims[1]))
        Y = as_f64(Y).reshape(-1)
        N = X.shape[0]
        if Y.size != N:
            raise ValueError('Y must have N entries')
        s = _lib.zigp_stage_kron_fused()
        s.lik = self.LIK[lik] if not two else _lib.LIK_ONOFF
        s.include_kl = 1 if include_kl else 0
        s.p = C.pointer(sp)
        s.X, s.Y, s.N = ptr(X), ptr(Y), N
        s.jitter, s.scale, s.g_offset, s.f_mu = float(jitter), float(scale), float(g_offset), float(f_mu)
        Ms = [(keep[t][0].shape[0], keep[t][1].shape[0]) for t in tags]
        small = all(m0 <= 32 and m1 <= 32 for m0, m1 in Ms)
        R0, R1 = (32, 32) if small else (16, 112)                     # capacity rows (kf_plan)
        # the step follows the factor kinds of the CONTEXT: with a Matern factor it runs the Matern additions of the finish stage
        matern = any(self.get_kron_kernel(0 if not two else h, q) != 'rbf' for h in range(len(tags)) for q in range(2))
        ldw = max(R0, R1)
        Npad = max(1024, -(-N // 1024) * 1024)
        lat, hold = [], []
        for h, (M0, M1) in enumerate(Ms):
            Mq = (-(-M0 // 16) * 16, -(-M1 // 16) * 16)
            d = {}
            if taps:
                d = dict(K=[np.zeros((128, 128)) for q in range(2)], P=[np.zeros((Mq[q], Mq[q])) for q in range(2)],
                         PF=[np.zeros(Mq[q] * Mq[q]) for q in range(2)], dvec=[np.zeros(Mq[q] + 1) for q in range(2)],
                         Zs=[np.zeros((Mq[q], dims[q])) for q in range(2)], zc=[np.zeros(dims[q]) for q in range(2)],
                         part=np.zeros((4, Npad)), cot=np.zeros((4, Npad)), work=np.zeros(3 * R0 * ldw + R1 * ldw + 16 * (R0 + R1)))
                for k in ('U', 'S2', 'T0', 'T1', 'Al'):
                    d[k] = np.zeros(Mq)
                for k in ('AlF', 'S2F', 'AlTF', 'S2TF'):
                    d[k] = np.zeros(Mq[0] * Mq[1])
                t = s.lat[h]
                for q in range(2):
                    for k in ('K', 'P', 'PF', 'dvec', 'Zs', 'zc'):
                        setattr(t.fac[q], k, ptr(d[k][q]))
                for k in ('U', 'S2', 'T0', 'T1', 'Al', 'AlF', 'S2F', 'AlTF', 'S2TF', 'part', 'cot', 'work'):
                    setattr(t, k, ptr(d[k]))
                # ---- the finish stage: regions at their capacity sizes (W = 2 + 2 * 8 doubles per capacity row of a krow region)
                Rc, Wc, W = (R0, R1), 18, (2 + 2 * dims[0], 2 + 2 * dims[1])
                raw = dict(klv=np.zeros(8), gu=np.zeros(R0 * R1), gs=np.zeros(R0 * R1), krow=[np.zeros(Rc[q] * Wc) for q in range(2)])
                if matern:
                    raw['krow_first'] = [np.zeros(Rc[q] * Wc) for q in range(2)]
                    if small:
                        raw.update(Kd=[np.zeros((32, 128)) for q in range(2)], work2=np.zeros(d['work'].size), krow2=[np.zeros(32 * Wc) for q in range(2)])
                if not small:
                    raw['G'] = [np.zeros((ldw, ldw)) for q in range(2)]
                for k, v in raw.items():
                    if isinstance(v, list):
                        setattr(t, k, (_lib.dp * 2)(ptr(v[0]), ptr(v[1])))
                    else:
                        setattr(t, k, ptr(v))
                hold.append(raw)
                # every region whole under '<name>_cap' -- what the kernels do not write comes back as _lib.STAGE_SENTINEL (include/zigp_diag.h) --
                # and, under the plain name, the part the kernels write (a view of it)
                for k, v in raw.items():
                    if k not in ('Kd', 'work2'):
                        d[k + '_cap'] = v
                Mh = (M0, M1)
                d['klv'] = raw['klv'][:5]
                d['gu'], d['gs'] = raw['gu'][:M0 * M1].reshape(M0, M1), raw['gs'][:M0 * M1].reshape(M0, M1)
                for k in ('krow', 'krow_first', 'krow2'):
                    if k in raw:
                        d[k] = [raw[k][q][:Mh[q] * W[q]].reshape(Mh[q], W[q]) for q in range(2)]
                if 'Kd' in raw:
                    d['Kd'], d['work2'] = raw['Kd'], raw['work2']
                if 'G' in raw:      # factor 0: G rows, then the low words of Q2 (rows 16 ..); factor 1: P Q2
                    d['G'] = [raw['G'][0][:16 + Mq[0], :Mq[0]], raw['G'][1][:Mq[1], :Mq[1]]]
            if inject is not None and inject[h] is not None:
                inj = as_f64(inject[h], (4, N))
                hold.append(inj)
                s.lat[h].inject = ptr(inj)
            lat.append(d)
        facts = (C.c_int64 * len(_lib.KFF_FACTS))()
        s.facts = C.cast(facts, C.POINTER(C.c_int64))
        sc = np.zeros(3)
        s.elbo_data, s.kl, s.d_f_mu = sc.ctypes.data, sc.ctypes.data + 8, sc.ctypes.data + 16
        gs = _lib.zigp_kron_grads()
        g = {}
        for tag in tags:
            Z0, Z1, l0, l1, um, us = keep[tag]
            a = dict(Z0=np.zeros_like(Z0), Z1=np.zeros_like(Z1), ell0=np.zeros_like(l0), ell1=np.zeros_like(l1), um=np.zeros_like(um), us=np.zeros_like(us))
            g[tag] = a
            setattr(gs, 'Z0' + tag, ptr(a['Z0'])); setattr(gs, 'Z1' + tag, ptr(a['Z1']))
            setattr(gs, 'ell0' + tag, ptr(a['ell0'])); setattr(gs, 'ell1' + tag, ptr(a['ell1']))
            setattr(gs, 'u_%sm' % tag, ptr(a['um'])); setattr(gs, 'u_%ss_sqrt' % tag, ptr(a['us']))
        s.grads = C.pointer(gs)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_fused_step(self.ctx, C.byref(s)))
        out = dict(noise=gs.noise, f_mu=sc[2])
        for tag in tags:
            a = g[tag]
            out['Z' + tag] = [a['Z0'], a['Z1']]
            out['ell_' + tag] = [a['ell0'], a['ell1']]
            out['var_' + tag] = [getattr(gs, 'var0' + tag), getattr(gs, 'var1' + tag)]
            out['u_%sm' % tag] = a['um']
            out['u_%ss_sqrt' % tag] = a['us']
        return dict(elbo_data=float(sc[0]), kl=float(sc[1]), grads=out, facts={k: int(facts[i]) for i, k in enumerate(_lib.KFF_FACTS)}, lat=lat)

    def test_kron_panel_step(self, p, X, Y, lik='onoff', jitter=1e-5, scale=1.0, g_offset=0.0, f_mu=0.0, include_kl=True, inject=None, taps=True,
                             planes_of='dAl'):
        """One value-and-gradient step of the GEMM-panel Kronecker path with its device buffers snapshot behind the launches
        (zigp_test_kron_panel_step, include/zigp_diag.h, where every tap is written down).  Arguments as test_kron_fused_step; planes_of: the
        split-K reduction whose raw planes are taken ('dP0', 'dP1', 'dAl', 'dS2').  Refused for a step an ordinary call runs on the fused
        kernels (set_kron_panels forces the panels).
        Returns dict(elbo_data, kl, grads, facts {Nc, nk, lat: [per latent {Mq0, Mq1, nb0, nb1, S_dP0, S_dP1, S_dAl, S_dS2}]}, lat [per latent:
        dict(K, L, W, P, krow_n, dP_red, dP_acc, Q, dP_comb, T, PdPP, G, krow -- lists over the two factors, (Mq, Mq) or (Mq, 2 + 2 D); Q only
        with include_kl --, U, S2, T0, Al, dAl, dS2, T1_a, dU, T1_b (Mq0, Mq1), vec (Mq0 + Mq1), klv (5, with include_kl), part, cot (4, Nc),
        planes (S, nba 128, nbb 128), gu, gs (M0, M1))])."""
        two = lik == 'onoff'
        tags = ('f', 'g') if two else ('f',)
        sp, keep, dims = self._pack_kron(p, tags=tags)
        X = as_f64(X)
        if X.ndim != 2 or X.shape[1] != dims[0] + dims[1]:
            raise ValueError('X must be (N,%d)' % (dims[0] + dims[1]))
        Y = as_f64(Y).reshape(-1)
        N = X.shape[0]
        if Y.size != N:
            raise ValueError('Y must have N entries')
        s = _lib.zigp_stage_kron_panels()
        s.lik = self.LIK[lik] if not two else _lib.LIK_ONOFF
        s.include_kl = 1 if include_kl else 0
        s.p = C.pointer(sp)
        s.X, s.Y, s.N = ptr(X), ptr(Y), N
        s.jitter, s.scale, s.g_offset, s.f_mu = float(jitter), float(scale), float(g_offset), float(f_mu)
        Nc = max(1024, -(-N // 1024) * 1024)
        nk = Nc // 16
        which = _lib.KP_REDUCTIONS.index(planes_of)
        lat, hold = [], []
        for h, tag in enumerate(tags):
            M = (keep[tag][0].shape[0], keep[tag][1].shape[0])
            Mq = tuple(-(-m // 128) * 128 for m in M)
            t = s.lat[h]
            t.planes_of = which
            d = {}
            if taps:
                for k in _lib.KPT_FACTOR:
                    if k == 'Q' and not include_kl:
                        continue
                    d[k] = [np.zeros((Mq[q], 2 + 2 * dims[q]) if k.startswith('krow') else (Mq[q], Mq[q])) for q in range(2)]
                    for q in range(2):
                        setattr(t.f[q], k, ptr(d[k][q]))
                for k in ('U', 'S2', 'T0', 'Al', 'dAl', 'dS2', 'T1_a', 'dU', 'T1_b'):
                    d[k] = np.zeros(Mq)
                ba, bb = {'dP0': (Mq[0], Mq[0]), 'dP1': (Mq[1], Mq[1])}.get(planes_of, Mq)
                S = max(1, min(nk, 512 // max(1, (ba // 128) * (bb // 128))))      # nred's rule; the step's own S comes back in facts
                d.update(vec=np.zeros(Mq[0] + Mq[1]), part=np.zeros((4, Nc)), cot=np.zeros((4, Nc)), planes=np.zeros((S, ba, bb)),
                         gu=np.zeros(M), gs=np.zeros(M))
                if include_kl:
                    d['klv'] = np.zeros(5)
                for k, v in d.items():
                    if not isinstance(v, list):
                        setattr(t, k, ptr(v))
            if inject is not None and inject[h] is not None:
                inj = as_f64(inject[h], (4, N))
                hold.append(inj)
                t.inject = ptr(inj)
            lat.append(d)
        facts = (C.c_int64 * _lib.KPF_COUNT)()
        s.facts = C.cast(facts, C.POINTER(C.c_int64))
        sc = np.zeros(3)
        s.elbo_data, s.kl, s.d_f_mu = sc.ctypes.data, sc.ctypes.data + 8, sc.ctypes.data + 16
        gs = _lib.zigp_kron_grads()
        g = {}
        for tag in tags:
            Z0, Z1, l0, l1, um, us = keep[tag]
            a = dict(Z0=np.zeros_like(Z0), Z1=np.zeros_like(Z1), ell0=np.zeros_like(l0), ell1=np.zeros_like(l1), um=np.zeros_like(um), us=np.zeros_like(us))
            g[tag] = a
            setattr(gs, 'Z0' + tag, ptr(a['Z0'])); setattr(gs, 'Z1' + tag, ptr(a['Z1']))
            setattr(gs, 'ell0' + tag, ptr(a['ell0'])); setattr(gs, 'ell1' + tag, ptr(a['ell1']))
            setattr(gs, 'u_%sm' % tag, ptr(a['um'])); setattr(gs, 'u_%ss_sqrt' % tag, ptr(a['us']))
        s.grads = C.pointer(gs)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_panel_step(self.ctx, C.byref(s)))
        out = dict(noise=gs.noise, f_mu=sc[2])
        for tag in tags:
            a = g[tag]
            out['Z' + tag] = [a['Z0'], a['Z1']]
            out['ell_' + tag] = [a['ell0'], a['ell1']]
            out['var_' + tag] = [getattr(gs, 'var0' + tag), getattr(gs, 'var1' + tag)]
            out['u_%sm' % tag] = a['um']
            out['u_%ss_sqrt' % tag] = a['us']
        nl = len(_lib.KPF_LAT_FACTS)
        fd = dict(Nc=int(facts[0]), nk=int(facts[1]),
                  lat=[{k: int(facts[2 + h * nl + i]) for i, k in enumerate(_lib.KPF_LAT_FACTS)} for h in range(len(tags))])
        if taps:
            for h, d in enumerate(lat):
                if fd['lat'][h]['S_' + planes_of] != d['planes'].shape[0]:
                    raise RuntimeError('test_kron_panel_step: the step split %s into %d slices, the binding sized its planes for %d'
                                       % (planes_of, fd['lat'][h]['S_' + planes_of], d['planes'].shape[0]))
        return dict(elbo_data=float(sc[0]), kl=float(sc[1]), grads=out, facts=fd, lat=lat)

    def test_path_weights(self, p, draws, n_samples, jitter=1e-6):
        """The weight stage of sample_paths -- a draw of q(u) into the weight table the path kernel reads -- through the product's own
        host function, with the device buffers snapshot behind every launch (zigp_test_path_weights, include/zigp_diag.h, where every
        tap is written down).  p and draws as sample_paths reads them.  Returns dict(facts {mode, Sp, nst, ntile, Mp, M4, R4, F}, lat
        [f, g: dict(Kuu, W (Mp, Mp), u, s (Mp), E, rhs, V (Mp, Sp), FT (Sp, Mp), tab (ntile, F, 16); unwhitened: t, V0, KV, res, t2, cor;
        whitened: G; full covariance: Lq, H)]).  A work matrix element no launch wrote holds _lib.STAGE_SENTINEL."""
        pk = _Packed(p)
        S = int(n_samples)
        draws, recs, keep = self._path_draws(pk, pk.kinds, S, 0, None, draws)
        self._prepare(p, pk)
        mode = 0 if not p.get('whiten', False) else 1 if p.get('q_diag', True) else 2
        Sp, nt = -(-S // 128) * 128, -(-S // 16)
        nst = 4 if nt >= 4 else 2 if nt >= 2 else 1
        ntile = -(-nt // nst) * nst
        s = _lib.zigp_stage_path_weights()
        s.p, s.jitter, s.S = C.pointer(pk.struct), float(jitter), S
        s.draw_f, s.draw_g = C.pointer(recs[0]), C.pointer(recs[1])
        lat = []
        for h, (M, tag) in enumerate(((pk.Mf, 'f'), (pk.Mg, 'g'))):
            Mp, R = -(-M // 128) * 128, int(draws[tag]['R'])
            F = -(-M // 4) * 4 + -(-R // 4) * 4
            names = ['Kuu', 'W', 'u', 's', 'E', 'FT', 'rhs', 'V', 'tab'] + (['t', 'V0', 'KV', 'res', 't2', 'cor'] if mode == 0 else ['G']) + (
                ['Lq', 'H'] if mode == 2 else [])
            d = {}
            for k in names:
                shape = (Mp, Mp) if k in ('Kuu', 'W', 'Lq') else (Mp,) if k in ('u', 's') else (Sp, Mp) if k == 'FT' else (ntile, F, 16) if k == 'tab' else (Mp, Sp)
                d[k] = np.full(shape, np.nan)
                setattr(s.lat[h], k, ptr(d[k]))
            lat.append(d)
        facts = (C.c_int64 * _lib.PWF_COUNT)()
        s.facts = C.cast(facts, C.POINTER(C.c_int64))
        _check(self.lib, self.ctx, self.lib.zigp_test_path_weights(self.ctx, C.byref(s)))
        fd = _lib.unpack_facts(_lib.PWF_FACTS, facts)
        want = dict(mode=mode, Sp=Sp, nst=nst, ntile=ntile, Mp=[d['Kuu'].shape[0] for d in lat], F=[d['tab'].shape[1] for d in lat])
        for k, v in want.items():
            if fd[k] != v:
                raise RuntimeError('test_path_weights: the stage ran with %s = %r, the binding sized its taps for %r' % (k, fd[k], v))
        return dict(facts=fd, lat=lat)

    def test_kron_path_weights(self, p, draws, n_samples, lik='onoff', jitter=1e-6):
        """The weight stage of kron_sample_paths (lik 'onoff') or kron_head_sample_paths ('gaussian', 'bernoulli': the f fields alone)
        through the product's own host function, with the device buffers snapshot behind every launch (zigp_test_kron_path_weights,
        include/zigp_diag.h).  Returns dict(facts {nst, ntile, Mq0, Mq1, M1p, R4, F}, lat [per latent: dict(K, W: lists over the two factors,
        (Mq, Mq); E (M, S); U, Sq (M); FZ, rhs, A1, B1, A2, V (S, M0, M1); tab (ntile, F, 16))])."""
        two = lik == 'onoff'
        tags = ('f', 'g') if two else ('f',)
        code = _lib.LIK_ONOFF if two else self._head_lik('test_kron_path_weights', lik)
        sp, keep, dims = self._pack_kron(p, tags=tags)
        self._set_kron_kinds(p, tags)
        S = int(n_samples)
        draws, recs, keepd = self._kron_path_draws(sp, dims, tags, S, 0, None, draws, kron_kernel_kinds(p, tags))
        nt = -(-S // 16)
        nst = 4 if nt >= 4 else 2 if nt >= 2 else 1
        ntile = -(-nt // nst) * nst
        s = _lib.zigp_stage_kron_path_weights()
        s.p, s.lik, s.S, s.jitter = C.pointer(sp), code, S, float(jitter)
        s.draw_f = C.pointer(recs['f'])
        if two:
            s.draw_g = C.pointer(recs['g'])
        lat = []
        for h, tag in enumerate(tags):
            M0, M1 = int(getattr(sp, 'M0' + tag)), int(getattr(sp, 'M1' + tag))
            Mq, R = (-(-M0 // 128) * 128, -(-M1 // 128) * 128), int(draws[tag]['R'])
            F = M0 * (-(-M1 // 4) * 4) + -(-R // 4) * 4
            d = dict(K=[np.full((m, m), np.nan) for m in Mq], W=[np.full((m, m), np.nan) for m in Mq], E=np.full((M0 * M1, S), np.nan),
                     U=np.full(M0 * M1, np.nan), Sq=np.full(M0 * M1, np.nan), tab=np.full((ntile, F, 16), np.nan))
            for k in ('FZ', 'rhs', 'A1', 'B1', 'A2', 'V'):
                d[k] = np.full((S, M0, M1), np.nan)
            for k, v in d.items():
                if isinstance(v, list):
                    for q in range(2):
                        getattr(s.lat[h], k)[q] = ptr(v[q])
                else:
                    setattr(s.lat[h], k, ptr(v))
            lat.append(d)
        facts = (C.c_int64 * _lib.KWF_COUNT)()
        s.facts = C.cast(facts, C.POINTER(C.c_int64))
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_path_weights(self.ctx, C.byref(s)))
        fd = _lib.unpack_facts(_lib.KWF_FACTS, facts)
        for h, d in enumerate(lat):
            got = (fd['nst'], fd['ntile'], fd['Mq0'][h], fd['Mq1'][h], fd['F'][h])
            want = (nst, ntile, d['K'][0].shape[0], d['K'][1].shape[0], d['tab'].shape[1])
            if got != want:
                raise RuntimeError('test_kron_path_weights: the stage ran with (nst, ntile, Mq0, Mq1, F) = %r, the binding sized its taps for %r' % (got, want))
        return dict(facts=fd, lat=lat)

    @staticmethod
    def kron_fit_sizes(shape, lik='onoff'):
        """block sizes of the free vector of kron_fit_steps (lik 'onoff': 17 blocks) or kron_head_fit_steps (10 blocks)"""
        D0, D1 = int(shape['D0']), int(shape['D1'])
        out = []
        for t in (('f', 'g') if lik == 'onoff' else ('f',)):
            M0, M1 = int(shape['M0' + t]), int(shape['M1' + t])
            out += [M0 * D0, M1 * D1, M0 * M1, M0 * M1, D0, D1, 1, 1]
        return out + ([1] if lik == 'onoff' else [1, 1])

    def _kron_fit_update_struct(self, shape, lik):
        two = lik == 'onoff'
        if not two and lik not in self.LIK:
            raise ValueError("lik must be 'onoff', 'gaussian' or 'bernoulli'")
        sp = _lib.zigp_kron_params()
        for k in (('M0f', 'M1f', 'M0g', 'M1g', 'D0', 'D1') if two else ('M0f', 'M1f', 'D0', 'D1')):
            setattr(sp, k, int(shape[k]))
        s = _lib.zigp_stage_kron_fit_update()
        s.lik = _lib.LIK_ONOFF if two else self.LIK[lik]
        s.shape = C.pointer(sp)
        facts = np.zeros(_lib.KFU_COUNT, dtype=np.int64)
        s.facts = facts.ctypes.data
        return s, sp, facts

    def test_kron_fit_update_facts(self, shape, lik='onoff'):
        """The layout a fit call of this shape uses (zigp_test_kron_fit_update with res = NULL): offsets of the result block, the grid and the
        element map of the update launches, the parameter image (_lib.KFU_FACTS)."""
        s, sp, facts = self._kron_fit_update_struct(shape, lik)
        nb = _lib.FIT_BLOCKS if lik == 'onoff' else _lib.HEAD_FIT_BLOCKS
        nf = sum(self.kron_fit_sizes(shape, lik))
        z, lr, pos = np.zeros(nf), np.ones(nb), np.zeros(nb, dtype=np.int32)
        s.n_steps, s.lr, s.positive, s.beta1, s.beta2, s.eps, s.n_free = 1, ptr(lr), pos.ctypes.data, 0.9, 0.999, 1e-8, nf
        s.x, s.m, s.v = ptr(z), ptr(z), ptr(z)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_fit_update(self.ctx, C.byref(s)))
        return _lib.unpack_facts(_lib.KFU_FACTS, facts)

    @staticmethod
    def kron_result_block(facts, shape, lik, lats, pws, info=()):
        """One raw result block [n_res] from compact arrays: lats = per latent dict(klv (5), krow [2] (M_q, 2 + 2 D_q), gu, gs (M0 M1)), pws (8),
        info = the Cholesky status of factor job j (missing: 0).  Every other double -- and the second int of every status slot, and the slots
        of jobs the model does not have -- holds _lib.STAGE_SENTINEL's bytes."""
        blk = np.full(facts['n_res'], _lib.STAGE_SENTINEL)
        for h, L in enumerate(lats):
            o = h * facts['RES_SIZE']
            blk[o + facts['RES_KLV']:o + facts['RES_KLV'] + 5] = as_f64(L['klv']).reshape(5)
            for q, key in enumerate(('RES_KROW0', 'RES_KROW1')):
                kr = as_f64(L['krow'][q]).reshape(-1)
                blk[o + facts[key]:o + facts[key] + kr.size] = kr
            for key, a in (('RES_GU', L['gu']), ('RES_GS', L['gs'])):
                a = as_f64(a).reshape(-1)
                blk[o + facts[key]:o + facts[key] + a.size] = a
        blk[facts['RES_PWS']:facts['RES_PWS'] + 8] = as_f64(pws).reshape(8)
        ints = blk[facts['RES_INFO']:facts['RES_INFO'] + 8].view(np.int32)
        for j in range(2 * len(lats)):
            ints[2 * j] = int(info[j]) if j < len(info) else 0
        return blk

    def test_kron_fit_update(self, shape, lik, x, m, v, lr, positive, trainable, t0, res, beta1=0.9, beta2=0.999, eps=1e-8):
        """The update kernel of kron_fit_steps (lik 'onoff') / kron_head_fit_steps through the host loop itself, step i replaced by the raw
        result block res[i] (zigp_test_kron_fit_update, include/zigp_diag.h; kron_result_block builds one).  x, m, v are updated in place as by
        the fit calls.  An injected Cholesky failure does NOT raise: returns dict(rc, error, steps_applied, snap_x, snap_m, snap_v
        [1 + n][n_free], snap_img [1 + n][n_img], hist [n][2], fail [4], elbo_data [n], kl [n], facts)."""
        s, sp, facts = self._kron_fit_update_struct(shape, lik)
        nb = _lib.FIT_BLOCKS if lik == 'onoff' else _lib.HEAD_FIT_BLOCKS
        for a in (x, m, v):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 1 and a.size == x.size):
                raise ValueError('x, m, v must be contiguous float64 vectors of one length')
        f0 = self.test_kron_fit_update_facts(shape, lik)
        res = as_f64(res)
        if res.ndim != 2 or res.shape[1] != f0['n_res']:
            raise ValueError('res must be [n_steps][n_res = %d]' % f0['n_res'])
        n, nf, n_img = res.shape[0], x.size, f0['n_img']
        lr_a = as_f64(lr).reshape(nb)
        pos = np.ascontiguousarray(np.asarray(positive, dtype=bool).reshape(nb), dtype=np.int32)
        tr = None if trainable is None else np.ascontiguousarray(np.asarray(trainable, dtype=bool).reshape(nb), dtype=np.int32)
        out = dict(snap_x=np.zeros((1 + n, nf)), snap_m=np.zeros((1 + n, nf)), snap_v=np.zeros((1 + n, nf)), snap_img=np.zeros((1 + n, n_img)),
                   hist=np.zeros((n, 2)), fail=np.zeros(4, dtype=np.int32), elbo_data=np.zeros(n), kl=np.zeros(n))
        applied = np.zeros(1, dtype=np.int64)
        s.n_steps, s.lr, s.positive, s.trainable = n, ptr(lr_a), pos.ctypes.data, None if tr is None else tr.ctypes.data
        s.beta1, s.beta2, s.eps, s.t0, s.n_free = float(beta1), float(beta2), float(eps), int(t0), nf
        s.x, s.m, s.v, s.res, s.n_res, s.n_img = ptr(x), ptr(m), ptr(v), ptr(res), f0['n_res'], n_img
        for k, a in out.items():
            setattr(s, k, a.ctypes.data)
        s.steps_applied = applied.ctypes.data
        rc = self.lib.zigp_test_kron_fit_update(self.ctx, C.byref(s))
        msg = ''
        if rc != 0:
            e = self.lib.zigp_last_error(self.ctx)
            msg = e.decode() if e else ''
            if rc != _lib.ZIGP_ENOTPD:
                _check(self.lib, self.ctx, rc)
        out.update(rc=rc, error=msg, steps_applied=int(applied[0]), facts=_lib.unpack_facts(_lib.KFU_FACTS, facts))
        return out

    @staticmethod
    def dense_fit_sizes(mode, shape, ell_size):
        """block sizes of the free vector of fit_steps / fit_steps_mode"""
        Mf, Mg, D = int(shape['Mf']), int(shape['Mg']), int(shape['D'])
        ns = [M * (M + 1) // 2 if mode == _lib.FIT_WHITE_FULL else M for M in (Mf, Mg)]
        return [Mf * D, Mg * D, Mf, Mg, ns[0], ns[1], int(ell_size[0]), int(ell_size[1]), 1, 1, 1]

    def test_dense_fit_update(self, mode, shape, x, m, v, lr, positive, trainable, ell_size, t0, packed, info=None, jitter=1e-6,
                              beta1=0.9, beta2=0.999, eps=1e-8):
        """The image and update kernels of fit_steps / fit_steps_mode through the host loop itself, step i's gradient step replaced by the
        packed vector packed[i] (layout of test_dense_pack's output) and the Cholesky status info[i] = (f, g) (zigp_test_dense_fit_update,
        include/zigp_diag.h).  A data set must be resident (set_data).  packed=None: the layout query, returns the facts dict
        (_lib.DFU_FACTS).  Otherwise x, m, v are updated in place and an injected failure does NOT raise: returns dict(rc, error,
        steps_applied, snap_x, snap_m, snap_v [1 + n][n_free], snap_img [1 + n][n_img], snap_H [1 + n][DH_SIZE], snap_Lraw [2] ([1 + n][M, M],
        full mode), hist, fail, elbo_data, kl, facts)."""
        mode = int(mode)
        s = _lib.zigp_stage_dense_fit_update()
        sp = _lib.zigp_params()
        sp.Mf, sp.Mg, sp.D = int(shape['Mf']), int(shape['Mg']), int(shape['D'])
        o = _lib.zigp_fit_opts()
        for b in range(_lib.DENSE_FIT_BLOCKS):
            o.lr[b] = float(lr[b]); o.positive[b] = int(bool(positive[b])); o.trainable[b] = int(bool(trainable[b]))
        o.ell_size_f, o.ell_size_g = int(ell_size[0]), int(ell_size[1])
        o.beta1, o.beta2, o.eps = float(beta1), float(beta2), float(eps)
        for a in (x, m, v):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 1 and a.size == x.size):
                raise ValueError('x, m, v must be contiguous float64 vectors of one length')
        facts = np.zeros(_lib.DFU_COUNT, dtype=np.int64)
        s.mode, s.shape, s.opts, s.t0, s.n_free, s.jitter = mode, C.pointer(sp), C.pointer(o), int(t0), x.size, float(jitter)
        s.x, s.m, s.v, s.facts = ptr(x), ptr(m), ptr(v), facts.ctypes.data
        if packed is None:
            s.n_steps = 1
            _check(self.lib, self.ctx, self.lib.zigp_test_dense_fit_update(self.ctx, C.byref(s)))
            return _lib.unpack_facts(_lib.DFU_FACTS, facts)
        f0 = self.test_dense_fit_update(mode, shape, x, m, v, lr, positive, trainable, ell_size, t0, None, jitter=jitter, beta1=beta1, beta2=beta2,
                                        eps=eps)
        packed = as_f64(packed)
        if packed.ndim != 2 or packed.shape[1] != f0['n_packed']:
            raise ValueError('packed must be [n_steps][n_packed = %d]' % f0['n_packed'])
        n, nf = packed.shape[0], x.size
        info_a = np.zeros((n, 2), dtype=np.int32) if info is None else np.ascontiguousarray(np.asarray(info, dtype=np.int32).reshape(n, 2))
        Ms = (sp.Mf, sp.Mg)
        full = mode == _lib.FIT_WHITE_FULL
        out = dict(snap_x=np.zeros((1 + n, nf)), snap_m=np.zeros((1 + n, nf)), snap_v=np.zeros((1 + n, nf)), snap_img=np.zeros((1 + n, f0['n_img'])),
                   snap_H=np.zeros((1 + n, f0['DH_SIZE'])), hist=np.zeros((n, 2)), fail=np.zeros(4, dtype=np.int32), elbo_data=np.zeros(n), kl=np.zeros(n))
        lraw = [np.zeros((1 + n, M, M)) for M in Ms] if full else None
        applied = np.zeros(1, dtype=np.int64)
        s.n_steps, s.packed, s.info, s.n_packed, s.n_img = n, ptr(packed), info_a.ctypes.data, f0['n_packed'], f0['n_img']
        for k, a in out.items():
            setattr(s, k, a.ctypes.data)
        if full:
            s.snap_Lraw = (_lib.dp * 2)(ptr(lraw[0]), ptr(lraw[1]))
        s.steps_applied = applied.ctypes.data
        rc = self.lib.zigp_test_dense_fit_update(self.ctx, C.byref(s))
        msg = ''
        if rc != 0:
            e = self.lib.zigp_last_error(self.ctx)
            msg = e.decode() if e else ''
            if rc != _lib.ZIGP_ENOTPD:
                _check(self.lib, self.ctx, rc)
        out.update(rc=rc, error=msg, steps_applied=int(applied[0]), facts=_lib.unpack_facts(_lib.DFU_FACTS, facts), snap_Lraw=lraw)
        return out

    def test_kron_panel_kbuild(self, X, col0, Z, ell, var, Nc):
        """k_kron_kbuild (zigp_test_kron_kbuild): the WHOLE padded factor panel (Mq, Nc), Mq = M rounded up to 128, from the columns
        col0 : col0 + D of X (N, ldx) and Z (M, D)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        (N, ldx), (M, D) = X.shape, Z.shape
        ell = as_f64(np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)))
        out = np.zeros(((M + 127) // 128 * 128, int(Nc)))
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_kbuild(self.ctx, N, int(Nc), ldx, int(col0), M, D, ptr(X), ptr(Z), ptr(ell), float(var), ptr(out)))
        return out

    def test_kron_panel_kbuild_kind(self, kind, X, col0, Z, ell, var, Nc, grad=True):
        """The factor panel of the kind 'rbf' / 'matern32' / 'matern52' (zigp_test_kron_kbuild_kind): (K, K') -- K' None with grad=False --
        as test_kron_panel_kbuild returns K: the whole padded (Mq, Nc) panels."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        (N, ldx), (M, D) = X.shape, Z.shape
        ell = as_f64(np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)))
        Mq = (M + 127) // 128 * 128
        K, Kd = np.zeros((Mq, int(Nc))), (np.zeros((Mq, int(Nc))) if grad else None)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_kbuild_kind(self.ctx, _lib.KERNELS[kind], N, int(Nc), ldx, int(col0), M, D, ptr(X), ptr(Z),
                                                                       ptr(ell), float(var), ptr(K), ptr(Kd) if grad else None))
        return K, Kd

    def test_kron_panel_kgrad_kind(self, kind, B, A, PdA, K, Kd, gm, dq, X, col0, Z, krow=None):
        """The factor cotangent of the kind (zigp_test_kron_kgrad_kind): test_kron_panel_kgrad with the derivative panel Kd (M, Nc)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        (N, ldx), (M, D) = X.shape, Z.shape
        K = as_f64(K)
        Nc = K.shape[1]
        B, A, PdA, K, Kd = (as_f64(x, (M, Nc)) for x in (B, A, PdA, K, Kd))
        gm, dq = as_f64(gm, (Nc,)), as_f64(dq, (Nc,))
        out = np.zeros((M, 2 + 2 * D)) if krow is None else np.array(as_f64(krow, (M, 2 + 2 * D)), copy=True)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_kgrad_kind(self.ctx, _lib.KERNELS[kind], M, D, N, Nc, ldx, int(col0), ptr(B), ptr(A),
                                                                      ptr(PdA), ptr(K), ptr(Kd), ptr(gm), ptr(dq), ptr(X), ptr(Z), ptr(out)))
        return out

    def test_kron_panel_colsum(self, K0, A0, K1, A1, B1, A0sq, C1):
        """k_kron_colsum (zigp_test_kron_colsum): part [4][Nc] = column sums of K0.A0, K1.A1, K0.B1, A0sq.C1."""
        K0, K1 = as_f64(K0), as_f64(K1)
        (M0, Nc), M1 = K0.shape, K1.shape[0]
        a = [as_f64(x, (m, Nc)) for x, m in ((K0, M0), (A0, M0), (K1, M1), (A1, M1), (B1, M0), (A0sq, M0), (C1, M0))]
        out = np.zeros((4, Nc))
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_colsum(self.ctx, M0, M1, Nc, *[ptr(x) for x in a], ptr(out)))
        return out

    def test_kron_panel_da(self, A, Cx, K, gv, dq):
        """k_kron_da (zigp_test_kron_da): (dA, E) = (2 A gv C, dq K + dA), (M, Nc) each."""
        A = as_f64(A)
        M, Nc = A.shape
        Cx, K, gv, dq = as_f64(Cx, (M, Nc)), as_f64(K, (M, Nc)), as_f64(gv, (Nc,)), as_f64(dq, (Nc,))
        dA, E = np.zeros((M, Nc)), np.zeros((M, Nc))
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_da(self.ctx, M, Nc, ptr(A), ptr(Cx), ptr(K), ptr(gv), ptr(dq), ptr(dA), ptr(E)))
        return dA, E

    def test_kron_panel_kgrad(self, B, A, PdA, K, gm, dq, X, col0, Z, krow=None):
        """k_kron_kgrad (zigp_test_kron_kgrad): krow (M, 2 + 2D) with the sums over the N = len(X) valid columns added onto `krow` (zeros if
        None); the factor's inputs are the columns col0 : col0 + D of X (N, ldx)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        (N, ldx), (M, D) = X.shape, Z.shape
        K = as_f64(K)
        Nc = K.shape[1]
        B, A, PdA, K = (as_f64(x, (M, Nc)) for x in (B, A, PdA, K))
        gm, dq = as_f64(gm, (Nc,)), as_f64(dq, (Nc,))
        out = np.zeros((M, 2 + 2 * D)) if krow is None else np.array(as_f64(krow, (M, 2 + 2 * D)), copy=True)
        _check(self.lib, self.ctx, self.lib.zigp_test_kron_kgrad(self.ctx, M, D, N, Nc, ldx, int(col0), ptr(B), ptr(A), ptr(PdA), ptr(K), ptr(gm), ptr(dq),
                                                                  ptr(X), ptr(Z), ptr(out)))
        return out

    def test_q_full_forward(self, W, Lq, u):
        """Forward M x M stage of a full-covariance call for one latent (zigp_test_q_full_forward): returns (T - I, R^T = (T - I) W, KL)
        for T = tril(Lq) tril(Lq)^T."""
        W, Lq, u = as_f64(W), as_f64(Lq), as_f64(u).reshape(-1)
        M = W.shape[0]
        TmI, Rt, kl = np.zeros((M, M)), np.zeros((M, M)), np.zeros(1)
        _check(self.lib, self.ctx, self.lib.zigp_test_q_full_forward(self.ctx, M, ptr(W), ptr(Lq), ptr(u), ptr(TmI), ptr(Rt), ptr(kl)))
        return TmI, Rt, float(kl[0])

    def test_q_full_dlq(self, C1, Lq, include_kl=True):
        """dLq = tril(2 C1 Lq) - [include_kl] (tril(Lq) - diag(1 / Lq_ii)) as the reverse M x M stage forms it (zigp_test_q_full_dlq)."""
        C1, Lq = as_f64(C1), as_f64(Lq)
        M = C1.shape[0]
        out = np.zeros((M, M))
        _check(self.lib, self.ctx, self.lib.zigp_test_q_full_dlq(self.ctx, M, ptr(C1), ptr(Lq), 1 if include_kl else 0, ptr(out)))
        return out

    def test_kgrad(self, Jp, K, alpha, gm, gv, X, Z, n0=0, ell=None, centre=None, exact=None, krow=None):
        """Kuf cotangent reductions of one chunk: the KG_SPLIT slabs [4][M][2+2D] (added onto `krow` if given)."""
        X, Z = as_f64(X), as_f64(Z)
        if X.ndim == 1: X = X[:, None]
        if Z.ndim == 1: Z = Z[:, None]
        M, D = Z.shape
        K, Jp = as_f64(K), as_f64(Jp)
        Nc = K.shape[1]
        alpha, gm, gv = as_f64(alpha, (M,)), as_f64(gm, (Nc,)), as_f64(gv, (Nc,))
        ell = None if ell is None else as_f64(np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)))
        centre = None if centre is None else as_f64(centre, (D,))
        out = np.zeros((_lib.KG_SPLIT, M, 2 + 2 * D)) if krow is None else np.array(as_f64(krow, (_lib.KG_SPLIT, M, 2 + 2 * D)), copy=True)
        _check(self.lib, self.ctx, self.lib.zigp_test_kgrad(
            self.ctx, M, D, Nc, X.shape[0], int(n0), ptr(as_f64(Jp, (M, Nc))), ptr(as_f64(K, (M, Nc))), ptr(alpha), ptr(gm), ptr(gv), ptr(X), ptr(Z),
            None if ell is None else ptr(ell), None if centre is None else ptr(centre), -1 if exact is None else int(bool(exact)), ptr(out)))
        return out

    def test_rank_update(self, chunks):
        """C1 = sum_i A1_i diag(gv_i) A1_i^T over chunks [(A1 (M,Nc_i), gv (Nc_i)), ...].  Returns (C1 (M,M), (So, Sd))."""
        A = [as_f64(a) for a, _ in chunks]
        g = [as_f64(v, (a.shape[1],)) for a, (_, v) in zip(A, chunks)]
        M, n = A[0].shape[0], len(A)
        Nc = (C.c_int64 * n)(*[a.shape[1] for a in A])
        pa, pg = (_lib.dp * n)(*[ptr(a) for a in A]), (_lib.dp * n)(*[ptr(v) for v in g])
        out, plan = np.zeros((M, M)), (C.c_int64 * 2)()
        _check(self.lib, self.ctx, self.lib.zigp_test_rank_update(self.ctx, M, n, Nc, pa, pg, ptr(out), plan))
        return out, (plan[0], plan[1])

    def test_mxm_backward(self, W, L, Kuu, Z, s, alpha, C1=None, Kgm=None, v=None, u=None, P=None, mode='diag', with_data=True, with_kl=True,
                          jitter=1e-6, krow=None, pad=0.0, taps=True):
        """The M x M reverse stage of one latent through latent_mxm_backward[_white] (zigp_test_mxm_backward).  mode 'diag' (unwhitened),
        'white' or 'white_full' (then s is Lq, (M,M)).  krow: the WHOLE device buffer [KG_SPLIT][Mp][2+2D], padded rows included (the sum of
        column 1 + 2D over the slabs is K gm), or None: zeros with Kgm (M) in slab 0.  P = None: the stage forms W^T W itself.  pad: what
        the padding of Z, Kuu, s and C1 holds on the device.  Returns dict(a1gm, du, dsq, G, dLq (white_full), krow (whole buffer),
        taps = {name: (M,M)} of the taps this mode passes (_lib.MXM_TAPS))."""
        W, L, Kuu, Z = as_f64(W), as_f64(L), as_f64(Kuu), as_f64(Z)
        if Z.ndim == 1: Z = Z[:, None]
        M, D = Z.shape
        Mp, Wd = (M + 127) // 128 * 128, 2 + 2 * D
        full = mode == 'white_full'
        a = _lib.zigp_stage_mxm()
        a.M, a.D, a.mode, a.with_data, a.with_kl = M, D, _lib.MXM_MODES.index(mode), int(bool(with_data)), int(bool(with_kl))
        a.jitter, a.pad = float(jitter), float(pad)
        ins = dict(W=as_f64(W, (M, M)), L=as_f64(L, (M, M)), Kuu=as_f64(Kuu, (M, M)), Z=Z, s=as_f64(s, (M, M) if full else (M,)),
                   alpha=as_f64(alpha, (M,)))
        for k, x, shape in (('u', u, (M,)), ('v', v, (M,)), ('P', P, (M, M)), ('C1', C1, (M, M))):
            if x is not None:
                ins[k] = as_f64(x, shape)
        if krow is None:
            krow = np.zeros((_lib.KG_SPLIT, Mp, Wd))
            if Kgm is not None:
                krow[0, :M, 1 + 2 * D] = as_f64(Kgm, (M,))
        out = dict(krow=np.array(as_f64(krow, (_lib.KG_SPLIT, Mp, Wd)), copy=True), a1gm=np.zeros(M), du=np.zeros(M), dsq=np.zeros(M),
                   G=np.zeros((M, M)))
        if full:
            out['dLq'] = np.zeros((M, M))
        for k, x in list(ins.items()) + list(out.items()):
            setattr(a, k, ptr(x))
        if mode == 'diag':
            names = [t for t in _lib.MXM_TAPS if (with_data or t in ('P', 'PSP')) and (with_kl or t not in ('P', 'PSP')) and (t != 'P' or P is None)]
        else:
            names = [t for t in ('C1', 'R', 'dL', 'Q', 'QW', 'S') + (('Y',) if full else ()) if with_data]
        tp = {t: np.zeros((M, M)) for t in names} if taps else {}
        for t, x in tp.items():
            a.tap[_lib.MXM_TAPS.index(t)] = ptr(x)
        _check(self.lib, self.ctx, self.lib.zigp_test_mxm_backward(self.ctx, C.byref(a)))
        out['taps'] = tp
        return out


def reference_engine(device=0):
    """The engine of the reference look-alikes (onoffgpf.OnOffSVGP, onofftf.onoff / predict_onoff, the likelihood heads): results identical
    to the reference on the same inputs includes WHERE it fails -- tf.cholesky raises on a non-positive pivot only (onofftf/main.py:200,
    268,355), so these run with zigp_set_pivot_rtol(ctx, 0).  The stricter default of the bare engine (8 eps (variance + jitter)) stays
    one call away: engine.set_pivot_rtol(8)."""
    return DenseEngine(device, pivot_rtol=0.0)
