"""Host side of the heads' device fit loop (zigp_kron_head_fit_steps): the C-ABI symbols, onofftf.heads.HeadDeviceFit against a stand-in
engine whose kron_head_fit_steps is the CPU oracle (torch autograd) plus NumPy Adam, and the batch sequence / call cadence of
fit_head(device_loop=True) over a recording stand-in.  No GPU needed."""
import ctypes as C
import logging
import os

import numpy as np
import pytest

import head_fit_ref as R

LOGGER = logging.getLogger('test_cpu_head_fit')


def test_head_fit_symbols_exist_and_reject_a_null_context():
    from zigp import _lib
    lib = _lib.load()
    assert _lib.HEAD_FIT_BLOCKS == 10 and C.sizeof(_lib.zigp_kron_head_fit_opts) == 10 * 8 + 2 * 10 * 4 + 3 * 8
    s, o = _lib.zigp_kron_params(), _lib.zigp_kron_head_fit_opts()
    x = np.zeros(4)
    rb = np.zeros(1, dtype=np.int64)
    rc = lib.zigp_kron_head_fit_steps(None, C.byref(s), _lib.LIK_GAUSSIAN, C.byref(o), x.ctypes.data, x.ctypes.data, x.ctypes.data, 4, 0, 1,
                                      rb.ctypes.data, 1, None, None, 1e-5, 1.0, 1, None, None)
    assert rc == _lib.ZIGP_EARG
    assert lib.zigp_kron_head_elbo_rows(None, C.byref(s), _lib.LIK_GAUSSIAN, 0, 1, 1e-5, 1.0, 0.0, 1, None, None, None, None) == _lib.ZIGP_EARG


def test_every_kron_entry_point_rejects_a_null_context():
    """Each zigp_kron_* entry point is a wrapper over a shared function that starts with the context check: with a NULL context every one
    returns ZIGP_EARG -- before it reads an argument, so the other pointers may be NULL too -- and zigp_kron_fit_steps_applied keeps its
    own return for it (ZIGP_EARG as an int64)."""
    from zigp import _lib
    lib = _lib.load()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith('zigp_kron_'))
    assert set(names) == {'zigp_kron_elbo', 'zigp_kron_elbo_rows', 'zigp_kron_fit_steps', 'zigp_kron_fit_steps_applied', 'zigp_kron_predict',
                          'zigp_kron_head_elbo', 'zigp_kron_head_elbo_rows', 'zigp_kron_head_fit_steps', 'zigp_kron_head_predict'}
    keep = []

    def blank(t):
        if t in (C.c_double,):
            return 0.0
        if t in (C.c_int32, C.c_int64, C.c_int):
            return 0
        if isinstance(t, type) and issubclass(t, C._Pointer):       # a struct the entry point would read: a zeroed one
            keep.append(t._type_())
            return C.byref(keep[-1])
        return None
    for n in names:
        res, args = _lib.SIGNATURES[n]
        assert args[0] is C.c_void_p, n
        rc = getattr(lib, n)(None, *[blank(t) for t in args[1:]])
        assert rc == _lib.ZIGP_EARG, (n, rc)


@pytest.mark.parametrize('lik', ['gaussian', 'bernoulli'])
def test_head_device_fit_equals_the_host_loop_on_the_oracle(lik):
    """20 steps at grid (6, 5) in calls of 7 + 7 + 6 with a host wrap-around batch mid-way: HeadDeviceFit over the oracle-backed stand-in ends
    within max(8 d, 1e-13) of the host loop on the same oracle (d: the +-1-ulp-nudged host run), parameters and history; the ParamSet
    round-trips (its values are the transforms of the fitter's free state, and a new fitter on it starts from that state)."""
    from onofftf.heads import HeadDeviceFit, HEAD_FIT_BLOCK_NAMES
    X, Y, mk = R.head_problem((6, 5), lik)
    seq, wi = R.rows_with_a_wrap(20)
    wraps = (np.ascontiguousarray(X[wi]), np.ascontiguousarray(Y[wi]))
    eng = R.OracleHeadEngine()
    a, b, dv = mk(), mk(), mk()
    ha = R.host_loop(eng, a, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps)
    hb = R.host_loop(eng, b, lik, seq, R.BATCH, R.JITTER, R.SCALE, X, Y, wraps, nudge_seed=1)
    eng.set_data(X, Y)
    fit = HeadDeviceFit(eng, dv, lik)
    assert fit.x.size == sum(R.block_sizes(fit.shape)) and len(fit.lr) == len(fit.positive) == len(fit.trainable) == 10
    hist = []
    for lo, hi in ((0, 7), (7, 14), (14, 20)):
        part = seq[lo:hi]
        ed, kl = fit.steps(part, R.BATCH, R.JITTER, R.SCALE, *(wraps if -1 in part else (None, None)))
        hist.append(np.stack([ed, kl], 1))
    assert fit.t == 20 and [c['t0'] for c in eng.fit_calls] == [0, 7, 14]
    d_par, d_hist = R.block_distance(b, a), R.hist_distance(hb, ha)
    e_par, e_hist = R.block_distance(dv, a), R.hist_distance(np.concatenate(hist), ha)
    print('%s: two host runs d_par %.3e d_hist %.3e | stand-in device loop - host: %.3e / %.3e' % (lik, d_par, d_hist, e_par, e_hist))
    assert e_par <= R.bound(d_par) and e_hist <= R.bound(d_hist)
    # the ParamSet round-trips
    o = 0
    for k, n in zip(HEAD_FIT_BLOCK_NAMES, fit.sizes):
        if k in dv.params:
            q = dv.params[k]
            assert np.array_equal(q.value.reshape(-1), np.asarray(q.transform.forward(fit.x[o:o + n])).reshape(-1)), k
        o += n
    again = HeadDeviceFit(eng, dv, lik)
    assert np.max(np.abs(again.x - fit.x)) <= 1e-12 * np.max(np.abs(fit.x))
    # the block a head does not have: an untrainable noise for the classifier; both have f_mu here or an untrainable 0
    names = dict(zip(HEAD_FIT_BLOCK_NAMES, fit.trainable))
    assert names['likelihood/variance'] == (lik == 'gaussian') and names['f_mu'] == (lik == 'bernoulli')


def test_fixed_and_missing_blocks_stay_where_they_are():
    """A fixed f_ind/z_0 is a block with trainable = 0: its x / m / v and its .value stay; a ParamSet without f_mu keeps a free value of 0;
    a fixed flag set between two calls is taken up."""
    from onofftf.heads import HeadDeviceFit
    X, Y, mk = R.head_problem((6, 5), 'gaussian')
    ps = mk()
    assert 'f_mu' not in ps.params
    ps.params['f_ind/z_0'].fixed = True
    z0 = ps.params['f_ind/z_0'].value.copy()
    eng = R.OracleHeadEngine()
    eng.set_data(X, Y)
    fit = HeadDeviceFit(eng, ps, 'gaussian')
    assert fit.trainable == [False, True, True, True, True, True, True, True, True, False]
    fit.m[:12] = 0.25
    fit.v[:12] = 0.5
    x0 = fit.x.copy()
    fit.steps([0, 700, 1400], R.BATCH, R.JITTER, R.SCALE)
    assert np.array_equal(fit.x[:12], x0[:12]) and np.all(fit.m[:12] == 0.25) and np.all(fit.v[:12] == 0.5)
    assert np.array_equal(ps.params['f_ind/z_0'].value, z0)
    assert fit.x[-1] == 0.0 and fit.m[-1] == 0.0 and fit.v[-1] == 0.0                      # the absent f_mu
    assert np.all(fit.x[12:-1] != x0[12:-1])                                               # everything else moved
    ps.params['f_ind/z_1'].fixed = True
    x1 = fit.x.copy()
    fit.steps([100], R.BATCH, R.JITTER, R.SCALE)
    assert eng.fit_calls[-1]['trainable'][:2] == [False, False] and np.array_equal(fit.x[:17], x1[:17]) and fit.t == 4
    with pytest.raises(ValueError, match='transform'):
        class Exp:                                     # neither Identity nor Log1pe(1e-6)
            forward, backward = staticmethod(np.exp), staticmethod(np.log)
        bad = mk()
        bad.params['f_kern/variance_0'].transform = Exp()
        HeadDeviceFit(eng, bad, 'gaussian')


class RecordingEngine:
    """set_data / kron_head_fit_steps that only record: which rows every step of every call was given"""

    def __init__(self):
        self.X = self.Y = None
        self.calls, self.batches, self.elbo_calls, self.wrap_pos = [], [], 0, []

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X), np.array(Y)

    def kron_head_elbo(self, *a, **k):
        self.elbo_calls += 1
        raise AssertionError('the device loop makes no kron_head_elbo call')

    def kron_head_fit_steps(self, shape, lik, x, m, v, lr, positive, trainable, t0, row_begin, batch, jitter=1e-5, scale=1.0, Xw=None, Yw=None, **kw):
        self.calls.append((t0, len(row_begin)))
        self.wrap_pos += [i for i, rb in enumerate(row_begin) if rb < 0 and i != len(row_begin) - 1]
        for rb in row_begin:
            if rb >= 0:
                self.batches.append((self.X[rb:rb + batch].copy(), self.Y[rb:rb + batch].copy()))
            else:
                k = -rb - 1
                self.batches.append((np.array(Xw[k * batch:(k + 1) * batch]), np.array(Yw[k * batch:(k + 1) * batch])))
        n = len(row_begin)
        return np.arange(t0, t0 + n, dtype=np.float64), np.zeros(n)


def test_fit_head_device_loop_sees_the_host_loop_s_batches_at_the_host_loop_s_cadence(tmp_path):
    """fit_head(device_loop=True) over the recording stand-in, 430 iterations of 700 rows on 3000 (an epoch boundary every ~4.3 batches),
    checkpoints every 150: the concatenated row ranges and wrap-around batches are the batches DataSet.next_batch hands the host loop
    from the same seed; a call ends at a wrap-around batch, at a checkpoint iteration and at every 100th iteration; history has one
    entry per iteration; the checkpoint exists."""
    from onofftf.heads import fit_head
    from onofftf.main import DataSet
    X, Y, mk = R.head_problem((6, 5), 'gaussian')
    num_iter, batch, save_every = 430, 700, 150
    eng, hist = RecordingEngine(), []
    ckpt = os.path.join(str(tmp_path), 'model')
    fit_head(mk(), 'gaussian', X, Y, num_iter, batch, LOGGER, ckpt=ckpt, eng=eng, save_every=save_every, history=hist, device_loop=True)
    assert eng.elbo_calls == 0 and len(eng.batches) == num_iter and len(hist) == num_iter
    assert hist == [-float(i) for i in range(num_iter)]                       # the stand-in's history: one cost per iteration, in order
    ds = DataSet(X, Y)
    for i in range(num_iter):
        xb, yb = ds.next_batch(batch)
        assert np.array_equal(xb, eng.batches[i][0]) and np.array_equal(yb, eng.batches[i][1]), i
    assert ds.epochs_completed >= 90 and not eng.wrap_pos                     # a wrap-around batch is the last step of its call
    # cadence: calls tile the iterations; none crosses a multiple of 100 or a checkpoint iteration (which is a call of its own)
    t = 0
    for t0, n in eng.calls:
        assert t0 == t and n >= 1
        assert (t0 // 100) == ((t0 + n - 1) // 100)
        for j in range(t0, t0 + n):
            if j % save_every == 0:
                assert n == 1
        t += n
    assert t == num_iter
    assert os.path.exists(ckpt + '.npz')
    # few wrap-around batches (10 rows of 3000), no checkpoints: the log cadence alone cuts the calls
    eng2, hist2 = RecordingEngine(), []
    fit_head(mk(), 'gaussian', X, Y, 250, 10, LOGGER, eng=eng2, save_every=0, history=hist2, device_loop=True)
    assert eng2.calls == [(0, 100), (100, 100), (200, 50)] and len(hist2) == 250
    # device_loop=False: the host loop, no fit call
    class HostOnly(R.OracleHeadEngine):
        def kron_head_fit_steps(self, *a, **k):
            raise AssertionError('device_loop=False makes no fit call')
    h2, e2 = [], HostOnly()
    fit_head(mk(), 'gaussian', X, Y, 3, 500, LOGGER, eng=e2, history=h2, device_loop=False)
    assert len(h2) == 3 and e2.elbo_calls == 3
