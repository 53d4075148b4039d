"""Host-side checks of the Matern 3/2 and 5/2 kernels of the dense path (zigp_set_kernel; DenseEngine p['kern_f'] / p['kern_g'];
onoffgpf.kernels.Matern32 / Matern52): the CPU reference tests/matern_ref.py against closed forms, its derivative factor K' against
autograd, the fixtures' Kuu, and the refusals and prototypes that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import make_problem
import matern_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATERN = ('matern32', 'matern52')


def _closed(kind, r, var):
    """the two formulas written out with math.*, at the floored distance r"""
    if kind == 'matern32':
        return var * (1 + math.sqrt(3) * r) * math.exp(-math.sqrt(3) * r), 3 * var * math.exp(-math.sqrt(3) * r)
    return (var * (1 + math.sqrt(5) * r + 5 / 3 * r * r) * math.exp(-math.sqrt(5) * r),
            5 / 3 * var * (1 + math.sqrt(5) * r) * math.exp(-math.sqrt(5) * r))


@pytest.mark.parametrize('kind', MATERN)
def test_reference_against_closed_forms_at_r0_and_r1(kind):
    var, ell = 2.5, np.array([0.5, 2.0, 4.0])
    Z = np.array([[0.3, -1.0, 2.0]])
    X = np.vstack([Z, Z + ell * np.array([0.6, 0.0, 0.8])])      # r2 = 0 exactly, and r2 = 0.36 + 0.64 = 1
    K = mr.kern_K_np(kind, Z, X, ell, var)
    k0, _ = _closed(kind, 1e-6, var)
    k1, _ = _closed(kind, math.sqrt(1.0 + 1e-12), var)
    assert abs(K[0, 0] - k0) <= 4e-16 * k0 and abs(K[0, 1] - k1) <= 1e-15 * k1
    assert K[0, 0] < var and var - K[0, 0] < 3e-12 * var        # the r = 1e-6 value: var (1 - O(r^2)), not var
    # K(Z, Z): the diagonal goes through the floored distance too; Kdiag is the variance itself
    assert mr.kern_K_np(kind, Z, None, ell, var)[0, 0] == K[0, 0]
    # numbers a reader can check by hand: Matern32 at r = 1: (1 + sqrt3) exp(-sqrt3) = 0.48335772...; Matern52: (1 + sqrt5 + 5/3) exp(-sqrt5) = 0.52399411...
    want = {'matern32': 0.48335772, 'matern52': 0.52399411}[kind]
    assert abs(K[0, 1] / var - want) < 1e-8


@pytest.mark.parametrize('kind', MATERN)
def test_derivative_factor_against_autograd(kind):
    """K' = -dk / d(r2 / 2): the closed form of the reference (and of the kernels) against autograd of k, coincident points included"""
    var = 1.7
    r2 = torch.tensor([0.0, 1e-14, 1e-12, 1e-6, 0.01, 0.5, 1.0, 4.0, 30.0, 400.0], dtype=torch.float64, requires_grad=True)
    k = mr.k_of_r2(kind, r2, var)
    (g,) = torch.autograd.grad(k.sum(), r2)
    kd_auto = (-2.0 * g).numpy()
    kd = mr.kd_of_r2(kind, r2.detach(), var).numpy()
    assert np.all(np.isfinite(kd_auto)) and np.all(kd > 0)
    # autograd differentiates (1 + a r + ...) exp(-a r) term by term: at r = 1e-6 the terms a and -a (1 + a r) cancel to a^2 r, eleven
    # digits down, and dr/dr2 = 1 / (2 r) scales the rounding of that difference: 2e-16 / (a r) relative, 1.3e-10 at r = 1e-6
    r = np.sqrt(r2.detach().numpy() + 1e-12)
    bound = 1e-14 + 4e-16 / r
    assert np.all(np.abs(kd_auto - kd) <= bound * kd), (np.abs(kd_auto - kd) / kd, bound)
    for i, rr in enumerate(r):
        assert abs(kd[i] - _closed(kind, float(rr), var)[1]) <= 1e-15 * kd[i]
    # the chain rule the engine's reverse pass uses: dk/dz_d = K' (x_d - z_d) / ell_d^2, dk/dell_d = K' (x_d - z_d)^2 / ell_d^3, dk/dvar = K / var
    rs = np.random.RandomState(3)
    X, Z, ell = torch.tensor(rs.randn(7, 3)), torch.tensor(rs.randn(4, 3), requires_grad=True), torch.tensor([0.7, 1.3, 2.1], dtype=torch.float64, requires_grad=True)
    v = torch.tensor(var, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(rs.randn(4, 7))
    K = mr.kern_K(kind, Z, X, ell, v)
    gZ, gl, gv = torch.autograd.grad((w * K).sum(), (Z, ell, v))
    with torch.no_grad():
        Kd = mr.kd_of_r2(kind, mr.square_dist(Z, X, ell), v)
        df = X[None, :, :] - Z[:, None, :]
        assert torch.allclose(gZ, torch.sum((w * Kd)[:, :, None] * df, 1) / ell ** 2, rtol=1e-12, atol=1e-14)
        assert torch.allclose(gl, torch.sum((w * Kd)[:, :, None] * df ** 2, (0, 1)) / ell ** 3, rtol=1e-12, atol=1e-14)
        assert torch.allclose(gv, (w * K).sum() / v, rtol=1e-12, atol=1e-14)


# the shapes of tests/test_gpu_matern.py: N, Mf, Mg, D
FIXTURES = [(1500, 50, 37, 3), (700, 137, 137, 1), (900, 64, 64, 8)]


@pytest.mark.parametrize('kind', MATERN)
@pytest.mark.parametrize('N,Mf,Mg,D', FIXTURES)
def test_kuu_of_the_fixtures_is_symmetric_positive_definite(kind, N, Mf, Mg, D):
    X, Y, p = mr.problem(N, Mf, Mg, D)
    for tag in 'fg':
        K = mr.kern_K_np(kind, p['Z' + tag], None, p['ell_' + tag], p['var_' + tag]) + 1e-6 * np.eye(p['Z' + tag].shape[0])
        assert np.array_equal(K, K.T)
        w = np.linalg.eigvalsh(K)
        print('%s %s M=%d D=%d: eig min %.3e max %.3e cond %.2e' % (kind, tag, K.shape[0], D, w[0], w[-1], w[-1] / w[0]))
        assert w[0] > 0
        np.linalg.cholesky(K)
        assert np.all(np.diagonal(K) < p['var_' + tag] + 1e-6) and np.all(np.diagonal(K) > p['var_' + tag])     # var (1 - O(1e-12)) + jitter


def test_unknown_kernel_name_and_wide_matern_raise_before_a_device_is_opened():
    from zigp.engine import _Packed, kernel_kinds
    from zigp import _lib
    X, Y, p = make_problem(10, 4, 3)
    assert _Packed(p).kinds == (0, 0) and kernel_kinds(dict(kern_f='Matern52', kern_g='matern32')) == (_lib.KERN_MATERN52, _lib.KERN_MATERN32)
    for bad in ('matern12', 'exponential', 'Matern', 3, None):
        with pytest.raises(ValueError, match="'rbf', 'matern32' and 'matern52'"):
            _Packed(dict(p, kern_g=bad))
    X9, Y9, p9 = make_problem(10, 4, 9)
    assert _Packed(p9).D == 9                                    # RBF at D = 9 is the wide path
    with pytest.raises(ValueError, match=r"kern_f = 'matern52' and D = 9: the Matern kernels cover D in \[1, 8\]"):
        _Packed(dict(p9, kern_f='matern52'))
    with pytest.raises(ValueError, match=r"kern_g = 'matern32' and D = 9"):
        _Packed(dict(p9, kern_g='matern32'))
    assert _Packed(dict(make_problem(10, 4, 8)[2], kern_f='matern32', kern_g='matern52')).kinds == (1, 2)


def test_model_refuses_a_wide_matern_before_it_opens_a_device():
    from onoffgpf import OnOffSVGP, OnOffLikelihood, kernels
    X, Y, p = make_problem(50, 5, 9)
    with pytest.raises(ValueError, match='kerng is a Matern52 kernel and D = 9: the Matern kernels cover D <= 8'):
        OnOffSVGP(X, Y, kernels.RBF(9), kernels.Matern52(9), OnOffLikelihood(), np.zeros((5, 9)), np.zeros((5, 9)))
    with pytest.raises(ValueError, match='kernf is a Matern32 kernel and D = 9'):
        OnOffSVGP(X, Y, kernels.Matern32(9, ARD=True), kernels.RBF(9), OnOffLikelihood(), np.zeros((5, 9)), np.zeros((5, 9)))
    # the kernel classes: one constructor, the same parameters, the variance as Kdiag
    for cls, kind in ((kernels.RBF, 'rbf'), (kernels.Matern32, 'matern32'), (kernels.Matern52, 'matern52')):
        k = cls(3, variance=2.0, lengthscales=[0.5, 1.0, 2.0], ARD=True)
        assert isinstance(k, kernels.Stationary) and k.kind == kind and k.ell_vector().tolist() == [0.5, 1.0, 2.0]
        assert np.allclose(k.compute_Kdiag(np.zeros((4, 3))), 2.0)
        assert cls(3, lengthscales=0.7).ell_vector().tolist() == [0.7] * 3


def test_kind_constants_follow_the_header():
    from zigp import _lib
    src = open(os.path.join(ROOT, 'include', 'zigp.h')).read()
    for name, val in (('RBF', _lib.KERN_RBF), ('MATERN32', _lib.KERN_MATERN32), ('MATERN52', _lib.KERN_MATERN52)):
        m = re.search(r'^#define\s+ZIGP_KERN_%s\s+(\d+)\s*$' % name, src, re.M)
        assert m and int(m.group(1)) == val
    assert _lib.KERNELS == {'rbf': 0, 'matern32': 1, 'matern52': 2}
    k = open(os.path.join(ROOT, 'zero-inflated-gp_amd', 'csrc', 'zigp_kernels.h')).read()
    assert re.search(r'constexpr int KERN_RBF = 0, KERN_M32 = 1, KERN_M52 = 2;', k)
    assert int(re.search(r'constexpr int MAXD = (\d+)', k).group(1)) == _lib.MATERN_MAX_D


def test_new_entry_points_refuse_a_null_context():
    """the ctypes prototypes of the new entry points: a NULL context is ZIGP_EARG (no device is touched)"""
    from zigp import _lib
    lib = _lib.load()
    a = np.zeros(8)
    pa = a.ctypes.data
    assert lib.zigp_set_kernel(None, 0, _lib.KERN_MATERN52) == _lib.ZIGP_EARG
    assert lib.zigp_get_kernel(None, 0) == _lib.ZIGP_EARG
    assert lib.zigp_kern_K(None, _lib.KERN_MATERN32, pa, 2, None, 0, 1, pa, 1.0, pa) == _lib.ZIGP_EARG
    assert lib.zigp_test_kuf_kind(None, _lib.KERN_MATERN32, 2, 2, 1, pa, pa, pa, 1.0, pa, pa) == _lib.ZIGP_EARG
    assert lib.zigp_test_kgrad_kind(None, _lib.KERN_MATERN52, 2, 1, 1024, 2, 0, pa, pa, pa, pa, pa, pa, pa, pa, pa) == _lib.ZIGP_EARG
    for name in ('zigp_set_kernel', 'zigp_get_kernel', 'zigp_kern_K', 'zigp_test_kuf_kind', 'zigp_test_kgrad_kind'):
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == len(_lib.SIGNATURES[name][1])
