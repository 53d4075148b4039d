"""Host-side checks of the input-dimension limit of the dense path (ZIGP_MAX_D = 64): the Python constant follows the header, and the
refusals that need no device come before anything touches one."""
import os
import re

import numpy as np
import pytest

from conftest import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_d_follows_the_header():
    from zigp import _lib
    src = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    m = re.search(r'^#define\s+ZIGP_MAX_D\s+(\d+)\s*$', src, re.M)
    assert m and int(m.group(1)) == _lib.MAX_D == 64
    k = open(os.path.join(ROOT, 'zero-inflated-gp_amd', 'csrc', 'zigp_kernels.h')).read()
    assert int(re.search(r'constexpr int WIDE_MAXD = (\d+)', k).group(1)) == _lib.MAX_D
    assert int(re.search(r'constexpr int MAXD = (\d+)', k).group(1)) == _lib.DEVICE_FIT_MAX_D == 8


@pytest.mark.parametrize('D', [0, 65, 100])
def test_packed_parameters_refuse_a_dimension_out_of_range(D):
    from zigp.engine import _Packed
    X, Y, p = make_problem(10, 4, 3)
    p = dict(p, Zf=np.zeros((4, D)), Zg=np.zeros((4, D)), ell_f=np.ones(max(D, 1)), ell_g=np.ones(max(D, 1)))
    with pytest.raises(ValueError, match='64'):
        _Packed(p)


@pytest.mark.parametrize('D', [9, 64])
def test_packed_parameters_accept_wide_dimensions(D):
    from zigp.engine import _Packed
    X, Y, p = make_problem(10, 4, D)
    pk = _Packed(p)
    assert pk.struct.D == D and pk.arr['ell_f'].size == D and pk.arr['Zf'].shape == (4, D)
    assert _Packed(dict(p, ell_f=0.7)).arr['ell_f'].tolist() == [0.7] * D       # a scalar lengthscale broadcasts over every column


def test_model_refuses_before_it_opens_a_device():
    """A Linear mean function above 8 columns and an input wider than 64 raise in the constructor, ahead of the engine."""
    from onoffgpf import OnOffSVGP, OnOffLikelihood, kernels, mean_functions
    X, Y, p = make_problem(50, 5, 12)
    mk = lambda X, **kw: OnOffSVGP(X, Y, kernels.RBF(X.shape[1], ARD=True), kernels.RBF(X.shape[1], ARD=True), OnOffLikelihood(),
                                   np.zeros((5, X.shape[1])), np.zeros((5, X.shape[1])), **kw)
    with pytest.raises(ValueError, match='Linear mean function covers D <= 8'):
        mk(X, mean_function=mean_functions.Linear(np.zeros((12, 1)), 0.0))
    with pytest.raises(ValueError, match='1 <= D <= 64'):
        mk(np.zeros((50, 65)))


@pytest.mark.parametrize('Nc', [1024, 4096, 32768])
@pytest.mark.parametrize('M', [128, 1100])
def test_moments_product_tile_list_is_a_partition(M, Nc):
    """The split-K list of the wide Kuf gradient's moments product (zigp_host.h kgmom_tiles, through the planner zigp_elbo uses): every
    (row tile, slice) once, one column tile, the k ranges of a row tile cover [0, Nc / 16) without gap or overlap in slice order, one
    entry per workgroup, and a slice count that follows from (Mp, Nc) alone."""
    import ctypes as C
    from zigp import _lib
    lib = _lib.load()
    Mp = (M + 127) // 128 * 128
    cap = 3 + 5 * 64 * (Mp // 128)
    out = (C.c_int64 * cap)()
    assert lib.zigp_test_kgmom_list(M, Nc, cap, out) == 0
    S, per, n = out[0], out[1], out[2]
    print('KGMOM-LIST Mp=%d Nc=%d: %d slices, %d entries' % (Mp, Nc, S, n))
    assert per == 1 and n % per == 0 and n == S * (Mp // 128) and 1 <= S <= 64
    assert S == max(1, min(64, Nc // 16 // 16, 512 // (Mp // 128)))
    t = np.array(out[3:3 + 5 * n], dtype=np.int64).reshape(n, 5)
    assert len({(int(r[0]), int(r[4])) for r in t}) == n and np.all(t[:, 1] == 0)
    for bi in range(Mp // 128):
        rows = t[t[:, 0] == bi]
        rows = rows[np.argsort(rows[:, 4])]
        assert rows[:, 4].tolist() == list(range(S))
        assert rows[0, 2] == 0 and rows[-1, 3] == Nc // 16 and np.all(rows[1:, 2] == rows[:-1, 3]) and np.all(rows[:, 3] > rows[:, 2])
    out2 = (C.c_int64 * cap)()
    assert lib.zigp_test_kgmom_list(Mp, Nc, cap, out2) == 0 and list(out2) == list(out)      # a function of Mp, not of M
    assert lib.zigp_test_kgmom_list(M, Nc + 16, cap, out) == _lib.ZIGP_EARG
