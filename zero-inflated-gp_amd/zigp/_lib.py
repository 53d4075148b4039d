"""ctypes binding of libzigp.so (include/zigp.h).  No CPU fallback: a missing library is an error."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get('ZIGP_LIB') or os.path.join(ROOT, 'lib', 'libzigp.so')   # ZIGP_LIB: A/B builds on one GPU box

ZIGP_OK, ZIGP_EARG, ZIGP_EHIP, ZIGP_ENOTPD, ZIGP_ECOMM = 0, -1, -2, -3, -4
COMM_ID_BYTES = 128
NCLASS = 10
LIK_ONOFF, LIK_GAUSSIAN, LIK_BERNOULLI = 0, 1, 2   # include/zigp.h ZIGP_LIK_*
KERN_RBF, KERN_MATERN32, KERN_MATERN52 = 0, 1, 2   # include/zigp.h ZIGP_KERN_*: kernel family of a dense latent (zigp_set_kernel) or of a Kronecker factor (zigp_set_kron_kernel)
KERNELS = {'rbf': KERN_RBF, 'matern32': KERN_MATERN32, 'matern52': KERN_MATERN52}
DENSITY_MAX_QUAD = 256   # include/zigp.h ZIGP_DENSITY_MAX_QUAD: nodes of the quadrature rule of the density calls
SCORE_MAX_LEVELS = 16    # include/zigp.h ZIGP_SCORE_MAX_LEVELS: quantile levels of one score call
MATERN_MAX_D = 8    # the Matern kernels cover the input dimensions of the per-dimension kernels (csrc/zigp_kernels.h MAXD)
PROF_CLASSES = ('gemm_A1', 'gemm_A2', 'gemm_H', 'gemm_J', 'syrk', 'kuf_build', 'pointwise', 'kgrad', 'mxm_stage', 'other')
PROF_KERNELS = {'gemm_A1': 'gemm_f64_kernel<1,1,2,false,1,8,EpiStoreColsum> (A1 = W K, W read through W^T)',
                'gemm_A2': 'gemm_f64_kernel<1,1,2,false,2,8,EpiColsum> (A2 = W^T A1, reduced to the column sums sum_m s^2 A2^2 in the epilogue; the panel is not stored; value-only ELBO and predict only)',
                'gemm_H': 'gemm_f64_kernel<1,1,2,false,1,8,EpiStore> (H = W diag(s^2) A2; not launched since round 4: folded into J\')',
                'gemm_J': 'gemm_f64_kernel<1,1,2,false,0,8,EpiStorePanelKColsum> (J\' = Q A2 = (Q W^T) A1, Q = Kuu^-1 diag(s^2) - I: the products H = W diag(s^2) A2 and J\' = W^T H - A2 as one full product on the A1 panel; the epilogue also reduces sum_m K J\', the variance term, so gradient steps launch no A2)',
                'syrk': 'gemm_f64_kernel<0,0,2,true,3,4,EpiAccum> (C1 += A1 G A1^T)'}

# double* everywhere in the C-ABI; typed as void* on the Python side so that a plain address (ndarray.ctypes.data, 1 us) can be passed
# or stored in a struct field -- ndarray.ctypes.data_as(POINTER(c_double)) costs 2.5 us and a Kronecker step hands over ~30 arrays
dp = C.c_void_p


MAX_D = 64           # ZIGP_MAX_D (include/zigp.h): input dimensions of the dense entry points
DEVICE_FIT_MAX_D = 8   # the device fit loops (zigp_fit_steps, zigp_fit_steps_mode) and a Linear mean function stop here


class ZigpError(RuntimeError):
    pass


class NotPositiveDefiniteError(ZigpError):
    """Cholesky failed (the reference raises tf.errors.InvalidArgumentError at this point)."""


class zigp_params(C.Structure):
    _fields_ = [('Mf', C.c_int32), ('Mg', C.c_int32), ('D', C.c_int32), ('reserved', C.c_int32),
                ('Zf', dp), ('Zg', dp), ('u_fm', dp), ('u_gm', dp), ('u_fs_sqrt', dp), ('u_gs_sqrt', dp),
                ('ell_f', dp), ('ell_g', dp), ('var_f', C.c_double), ('var_g', C.c_double), ('noise', C.c_double)]


class zigp_grads(C.Structure):
    _fields_ = [('Zf', dp), ('Zg', dp), ('u_fm', dp), ('u_gm', dp), ('u_fs_sqrt', dp), ('u_gs_sqrt', dp),
                ('ell_f', dp), ('ell_g', dp), ('var_f', C.c_double), ('var_g', C.c_double), ('noise', C.c_double)]


class zigp_kron_params(C.Structure):
    _fields_ = [('M0f', C.c_int32), ('M1f', C.c_int32), ('M0g', C.c_int32), ('M1g', C.c_int32),
                ('D0', C.c_int32), ('D1', C.c_int32), ('reserved0', C.c_int32), ('reserved1', C.c_int32),
                ('Z0f', dp), ('Z1f', dp), ('Z0g', dp), ('Z1g', dp),
                ('ell0f', dp), ('ell1f', dp), ('ell0g', dp), ('ell1g', dp),
                ('var0f', C.c_double), ('var1f', C.c_double), ('var0g', C.c_double), ('var1g', C.c_double),
                ('u_fm', dp), ('u_gm', dp), ('u_fs_sqrt', dp), ('u_gs_sqrt', dp), ('noise', C.c_double)]


class zigp_kron_grads(C.Structure):
    _fields_ = [('Z0f', dp), ('Z1f', dp), ('Z0g', dp), ('Z1g', dp),
                ('ell0f', dp), ('ell1f', dp), ('ell0g', dp), ('ell1g', dp),
                ('var0f', C.c_double), ('var1f', C.c_double), ('var0g', C.c_double), ('var1g', C.c_double),
                ('u_fm', dp), ('u_gm', dp), ('u_fs_sqrt', dp), ('u_gs_sqrt', dp), ('noise', C.c_double)]


PATH_MAX_S = 256   # include/zigp.h ZIGP_PATH_MAX_S: sample paths of one call
PATH_MAX_D = 8     # the path kernel is specialised per input dimension (csrc/zigp_paths.hip)


class zigp_path_latent(C.Structure):   # include/zigp.h "sample paths"
    _fields_ = [('kind', C.c_int32), ('M', C.c_int32), ('R', C.c_int32), ('reserved', C.c_int32), ('Z', dp), ('ell', dp), ('var', C.c_double),
                ('V', dp), ('omega', dp), ('phase', dp), ('amp', dp), ('lin', dp), ('shift', C.c_double)]


class zigp_path_draw(C.Structure):   # include/zigp.h "sample paths"
    _fields_ = [('R', C.c_int32), ('reserved', C.c_int32), ('omega0', dp), ('phase', dp), ('a', dp), ('eps', dp)]


KRON_PATH_MAX_M = 128   # include/zigp_kronpaths.h: inducing points per factor (csrc/zigp_kronpaths.hip KP_MAXM)


class zigp_kron_path_latent(C.Structure):   # include/zigp_kronpaths.h
    _fields_ = [('M0', C.c_int32), ('M1', C.c_int32), ('R', C.c_int32), ('reserved', C.c_int32), ('Z0', dp), ('Z1', dp), ('ell0', dp), ('ell1', dp),
                ('var0', C.c_double), ('var1', C.c_double), ('V', dp), ('omega', dp), ('phase', dp), ('amp', dp), ('shift', C.c_double)]


FIT_BLOCKS = 17   # include/zigp.h ZIGP_FIT_BLOCKS


class zigp_kron_fit_opts(C.Structure):
    _fields_ = [('lr', C.c_double * FIT_BLOCKS), ('positive', C.c_int32 * FIT_BLOCKS), ('reserved', C.c_int32),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double)]


HEAD_FIT_BLOCKS = 10   # include/zigp.h ZIGP_HEAD_FIT_BLOCKS


class zigp_kron_head_fit_opts(C.Structure):
    _fields_ = [('lr', C.c_double * HEAD_FIT_BLOCKS), ('positive', C.c_int32 * HEAD_FIT_BLOCKS), ('trainable', C.c_int32 * HEAD_FIT_BLOCKS),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double)]


DENSE_FIT_BLOCKS = 11   # include/zigp.h ZIGP_DENSE_FIT_BLOCKS
FIT_DIAG, FIT_WHITE, FIT_WHITE_FULL = 0, 1, 2   # include/zigp.h ZIGP_FIT_*: the `mode` of zigp_fit_steps_mode


class zigp_fit_opts(C.Structure):
    _fields_ = [('lr', C.c_double * DENSE_FIT_BLOCKS), ('positive', C.c_int32 * DENSE_FIT_BLOCKS), ('trainable', C.c_int32 * DENSE_FIT_BLOCKS),
                ('ell_size_f', C.c_int32), ('ell_size_g', C.c_int32), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double)]


class zigp_stage_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [('M', C.c_int32), ('reserved', C.c_int32), ('W', dp), ('v', dp), ('s2', dp), ('K', dp), ('Rt', dp),
                ('A1', dp), ('Jp', dp), ('part', dp)]


class zigp_stage_pointwise(C.Structure):   # include/zigp_diag.h
    _fields_ = [('mode', C.c_int32), ('repeat', C.c_int32),
                ('np_f', C.c_int32), ('np1_f', C.c_int32), ('np2_f', C.c_int32), ('np_g', C.c_int32), ('np1_g', C.c_int32), ('np2_g', C.c_int32),
                ('D', C.c_int32), ('mean_on', C.c_int32),
                ('part_f', dp), ('part_g', dp), ('Y', dp), ('X', dp),
                ('Nrows', C.c_int64), ('n0', C.c_int64), ('row_end', C.c_int64), ('Nc', C.c_int64),
                ('var_f', C.c_double), ('var_g', C.c_double), ('noise', C.c_double), ('g_offset', C.c_double), ('scale', C.c_double),
                ('mean_a', C.c_double * 8), ('mean_b', C.c_double),
                ('gm_f', dp), ('gv_f', dp), ('gm_g', dp), ('gv_g', dp), ('acc', dp), ('out9', dp)]


MXM_TAPS = ('C1', 'Y', 'T', 'U', 'V', 'R', 'dL', 'Q', 'QW', 'S', 'P', 'PSP')   # include/zigp_diag.h ZIGP_MXM_TAP_*
MXM_MODES = ('diag', 'white', 'white_full')                                      # zigp_stage_mxm.mode


class zigp_stage_mxm(C.Structure):   # include/zigp_diag.h
    _fields_ = [('M', C.c_int32), ('D', C.c_int32), ('mode', C.c_int32), ('with_data', C.c_int32), ('with_kl', C.c_int32), ('reserved', C.c_int32),
                ('jitter', C.c_double), ('pad', C.c_double),
                ('W', dp), ('L', dp), ('Kuu', dp), ('Z', dp), ('s', dp), ('u', dp), ('v', dp), ('alpha', dp), ('P', dp), ('C1', dp),
                ('krow', dp), ('a1gm', dp), ('du', dp), ('dsq', dp), ('dLq', dp), ('G', dp), ('tap', dp * len(MXM_TAPS))]


FWD_OUTS = ('W', 'v', 'alpha', 'Rt', 'dkinv', 'kl', 'P', 'Qt', 'Wp', 'Wt', 'wh', 'L', 'Kuu')   # include/zigp_diag.h ZIGP_FWD_*


class zigp_stage_pack_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [('M', C.c_int32), ('reserved', C.c_int32), ('krow', dp), ('du', dp), ('dsq', dp), ('s', dp), ('dLq', dp), ('kl_vec1', dp),
                ('kl_vec2', dp), ('ell', dp), ('var', C.c_double), ('kl', C.c_double)]


class zigp_stage_pack(C.Structure):   # include/zigp_diag.h
    _fields_ = [('D', C.c_int32), ('mode', C.c_int32), ('need_grad', C.c_int32), ('include_kl', C.c_int32), ('mean_on', C.c_int32),
                ('pw_blocks', C.c_int32), ('pw', dp), ('lat', zigp_stage_pack_latent * 2), ('out', dp), ('n_out', C.c_int64)]


class zigp_stage_kron_pointwise(C.Structure):   # include/zigp_diag.h
    _fields_ = [('lik', C.c_int32), ('mode', C.c_int32), ('dev_hyp', C.c_int32), ('sentinel_out', C.c_int32),
                ('N', C.c_int64), ('Nc', C.c_int64), ('ld_out', C.c_int64), ('part_f', dp), ('part_g', dp), ('Y', dp),
                ('var0f', C.c_double), ('var1f', C.c_double), ('var0g', C.c_double), ('var1g', C.c_double), ('noise', C.c_double),
                ('g_offset', C.c_double), ('f_offset', C.c_double), ('scale', C.c_double),
                ('gm_f', dp), ('gv_f', dp), ('dq0_f', dp), ('dq1_f', dp), ('gm_g', dp), ('gv_g', dp), ('dq0_g', dp), ('dq1_g', dp),
                ('acc', dp), ('out', dp)]


class zigp_kronf_tap_factor(C.Structure):   # include/zigp_diag.h
    _fields_ = [('K', dp), ('P', dp), ('PF', dp), ('dvec', dp), ('Zs', dp), ('zc', dp)]


class zigp_kronf_tap_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [('fac', zigp_kronf_tap_factor * 2), ('U', dp), ('S2', dp), ('T0', dp), ('T1', dp), ('Al', dp),
                ('AlF', dp), ('S2F', dp), ('AlTF', dp), ('S2TF', dp), ('part', dp), ('cot', dp), ('work', dp), ('inject', dp),
                ('klv', dp), ('krow', dp * 2), ('gu', dp), ('gs', dp), ('krow_first', dp * 2), ('Kd', dp * 2), ('work2', dp), ('krow2', dp * 2),
                ('G', dp * 2)]


KFF_FACTS = ('large', 'large_exact', 'nb0c', 'nb1c', 'nb0_f', 'nb1_f', 'nb0_g', 'nb1_g', 'Npad', 'ntiles', 'tpw_fwd', 'tpw_bwd', 'nparts', 'tps',
             'nranges', 'range_tiles', 'one_launch')   # include/zigp_diag.h ZIGP_KFF_*


class zigp_stage_kron_fused(C.Structure):   # include/zigp_diag.h
    _fields_ = [('lik', C.c_int32), ('include_kl', C.c_int32), ('p', C.POINTER(zigp_kron_params)), ('X', dp), ('Y', dp), ('N', C.c_int64),
                ('jitter', C.c_double), ('scale', C.c_double), ('g_offset', C.c_double), ('f_mu', C.c_double),
                ('lat', zigp_kronf_tap_latent * 2), ('facts', C.POINTER(C.c_int64)), ('elbo_data', dp), ('kl', dp),
                ('grads', C.POINTER(zigp_kron_grads)), ('d_f_mu', dp)]


KPT_FACTOR = ('K', 'L', 'W', 'P', 'krow_n', 'dP_red', 'dP_acc', 'Q', 'dP_comb', 'T', 'PdPP', 'G', 'krow')


class zigp_kronp_tap_factor(C.Structure):   # include/zigp_diag.h
    _fields_ = [(k, dp) for k in KPT_FACTOR]


class zigp_kronp_tap_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [('f', zigp_kronp_tap_factor * 2), ('U', dp), ('S2', dp), ('T0', dp), ('Al', dp), ('vec', dp), ('klv', dp), ('part', dp),
                ('inject', dp), ('cot', dp), ('planes_of', C.c_int32), ('planes', dp), ('dAl', dp), ('dS2', dp), ('T1_a', dp), ('dU', dp),
                ('T1_b', dp), ('gu', dp), ('gs', dp)]


KPF_LAT_FACTS = ('Mq0', 'Mq1', 'nb0', 'nb1', 'S_dP0', 'S_dP1', 'S_dAl', 'S_dS2')   # include/zigp_diag.h ZIGP_KPF_*: 'Nc', 'nk', then these per latent
KPF_COUNT = 2 + 2 * len(KPF_LAT_FACTS)
KP_REDUCTIONS = ('dP0', 'dP1', 'dAl', 'dS2')      # planes_of


class zigp_stage_kron_panels(C.Structure):   # include/zigp_diag.h
    _fields_ = [('lik', C.c_int32), ('include_kl', C.c_int32), ('p', C.POINTER(zigp_kron_params)), ('X', dp), ('Y', dp), ('N', C.c_int64),
                ('jitter', C.c_double), ('scale', C.c_double), ('g_offset', C.c_double), ('f_mu', C.c_double),
                ('lat', zigp_kronp_tap_latent * 2), ('facts', C.POINTER(C.c_int64)), ('elbo_data', dp), ('kl', dp),
                ('grads', C.POINTER(zigp_kron_grads)), ('d_f_mu', dp)]


KFU_FACTS = (('RES_KLV', 1), ('RES_KROW0', 1), ('RES_KROW1', 1), ('RES_GU', 1), ('RES_GS', 1), ('RES_SIZE', 1), ('RES_PWS', 1), ('RES_INFO', 1),
             ('n_res', 1), ('grid', 1), ('big_off', 9), ('hyp_off', 10), ('n_img', 1), ('off_hyp', 1), ('off_hyp2', 1), ('off_z', 4), ('off_u', 2),
             ('off_s', 2), ('KH_SIZE', 1), ('KH_FAC', 1), ('KH_INV', 1), ('KH_ZC', 1), ('KH_ELL', 1), ('KH_VAR', 1), ('KH_NOISE', 1),
             ('KH_FMU', 1))   # include/zigp_diag.h ZIGP_KFU_*: (name, entries)
KFU_COUNT = sum(n for _, n in KFU_FACTS)


class zigp_stage_kron_fit_update(C.Structure):   # include/zigp_diag.h
    _fields_ = [('lik', C.c_int32), ('n_steps', C.c_int32), ('shape', C.POINTER(zigp_kron_params)), ('lr', dp), ('positive', dp), ('trainable', dp),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('t0', C.c_int64), ('n_free', C.c_int64),
                ('x', dp), ('m', dp), ('v', dp), ('res', dp), ('n_res', C.c_int64), ('n_img', C.c_int64),
                ('snap_x', dp), ('snap_m', dp), ('snap_v', dp), ('snap_img', dp), ('hist', dp), ('fail', dp), ('elbo_data', dp), ('kl', dp),
                ('steps_applied', dp), ('facts', dp)]


DFU_FACTS = (('img_Z', 2), ('img_ell', 2), ('img_u', 2), ('img_s', 2), ('img_Zs', 2), ('Mp', 2), ('n_img', 1), ('n_packed', 1), ('grid', 1),
             ('tgrid', 1), ('DH_SIZE', 1), ('DH_LAT', 1), ('DH_INV', 1), ('DH_ELL', 1), ('DH_SCALE', 1), ('DH_VAR', 1), ('DH_PIVTOL', 1),
             ('DH_NOISE', 1))   # include/zigp_diag.h ZIGP_DFU_*
DFU_COUNT = sum(n for _, n in DFU_FACTS)


class zigp_stage_dense_fit_update(C.Structure):   # include/zigp_diag.h
    _fields_ = [('mode', C.c_int32), ('n_steps', C.c_int32), ('shape', C.POINTER(zigp_params)), ('opts', C.POINTER(zigp_fit_opts)),
                ('t0', C.c_int64), ('n_free', C.c_int64), ('jitter', C.c_double), ('x', dp), ('m', dp), ('v', dp), ('packed', dp), ('info', dp),
                ('n_packed', C.c_int64), ('n_img', C.c_int64), ('snap_x', dp), ('snap_m', dp), ('snap_v', dp), ('snap_img', dp), ('snap_H', dp),
                ('snap_Lraw', dp * 2), ('hist', dp), ('fail', dp), ('elbo_data', dp), ('kl', dp), ('steps_applied', dp), ('facts', dp)]


PWT_FIELDS = ('Kuu', 'W', 'Lq', 'u', 's', 'E', 'FT', 'rhs', 't', 'V0', 'KV', 'res', 't2', 'cor', 'G', 'H', 'V', 'tab')
PWF_FACTS = (('mode', 1), ('Sp', 1), ('nst', 1), ('ntile', 1), ('Mp', 2), ('M4', 2), ('R4', 2), ('F', 2))   # include/zigp_diag.h ZIGP_PWF_*
PWF_COUNT = sum(n for _, n in PWF_FACTS)


class zigp_pathw_tap_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [(k, dp) for k in PWT_FIELDS]


class zigp_stage_path_weights(C.Structure):   # include/zigp_diag.h
    _fields_ = [('p', C.POINTER(zigp_params)), ('jitter', C.c_double), ('draw_f', C.POINTER(zigp_path_draw)), ('draw_g', C.POINTER(zigp_path_draw)),
                ('S', C.c_int32), ('reserved', C.c_int32), ('lat', zigp_pathw_tap_latent * 2), ('facts', C.POINTER(C.c_int64))]


KWT_FIELDS = ('E', 'U', 'Sq', 'FZ', 'rhs', 'A1', 'B1', 'A2', 'V', 'tab')
KWF_FACTS = (('nst', 1), ('ntile', 1), ('Mq0', 2), ('Mq1', 2), ('M1p', 2), ('R4', 2), ('F', 2))   # include/zigp_diag.h ZIGP_KWF_*
KWF_COUNT = sum(n for _, n in KWF_FACTS)


class zigp_kpathw_tap_latent(C.Structure):   # include/zigp_diag.h
    _fields_ = [('K', dp * 2), ('W', dp * 2)] + [(k, dp) for k in KWT_FIELDS]


class zigp_stage_kron_path_weights(C.Structure):   # include/zigp_diag.h
    _fields_ = [('p', C.POINTER(zigp_kron_params)), ('lik', C.c_int32), ('S', C.c_int32), ('jitter', C.c_double),
                ('draw_f', C.POINTER(zigp_path_draw)), ('draw_g', C.POINTER(zigp_path_draw)), ('lat', zigp_kpathw_tap_latent * 2),
                ('facts', C.POINTER(C.c_int64))]


PSL_KINDS = ('diag', 'panel', 'trail', 'tri1', 'tri2')   # include/zigp_diag.h ZIGP_PSL_*
PSF_REC, PSF_PER = 8, 6                                    # ZIGP_PSF_*: header slots (Mp, nb, launches, images, info), slots per launch


class zigp_stage_potrf(C.Structure):   # include/zigp_diag.h
    _fields_ = [('n', C.c_int64), ('split_k', C.c_int32), ('reserved', C.c_int32), ('A', dp), ('L', dp), ('W', dp), ('T', dp), ('snap', dp),
                ('snap_cap', C.c_int64), ('facts', C.POINTER(C.c_int64)), ('facts_cap', C.c_int64)]


def unpack_facts(layout, arr):
    """facts array -> dict (an entry with more than one value: a list)"""
    out, o = {}, 0
    for name, n in layout:
        out[name] = int(arr[o]) if n == 1 else [int(a) for a in arr[o:o + n]]
        o += n
    return out


KPW_THREADS, KPW_ACC = 256, 5  # csrc/zigp_kron.hip: points per block and accumulators per block of the Kronecker point-wise kernels
STAGE_SENTINEL = float(np.frombuffer(bytes([0x7f]) * 8, dtype=np.float64)[0])   # ZIGP_STAGE_SENTINEL_BYTE in every byte: 1.38e306
KG_SPLIT, PW_PTS, PW_ACC = 4, 64, 13   # csrc/zigp_kernels.h

# name -> (restype, argtypes); mirrors include/zigp.h and include/zigp_diag.h exactly (tests check every declared symbol resolves)
SIGNATURES = {
    'zigp_create': (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    'zigp_destroy': (C.c_int, [C.c_void_p]),
    'zigp_last_error': (C.c_char_p, [C.c_void_p]),
    'zigp_last_info': (C.c_int, [C.c_void_p]),
    'zigp_set_chunk': (C.c_int, [C.c_void_p, C.c_int64]),
    'zigp_set_data': (C.c_int, [C.c_void_p, dp, dp, C.c_int64, C.c_int32]),
    'zigp_set_data_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    'zigp_select_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'zigp_elbo': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64,
                            C.c_int32, dp, dp, C.POINTER(zigp_grads)]),
    'zigp_fit_steps': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.POINTER(zigp_fit_opts), dp, dp, dp, C.c_int64, C.c_int64, C.c_int32,
                                 C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32, dp, dp]),
    'zigp_fit_steps_mode': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(zigp_params), C.POINTER(zigp_fit_opts), dp, dp, dp, C.c_int64, C.c_int64,
                                      C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32, dp, dp]),
    'zigp_fit_steps_applied': (C.c_int64, [C.c_void_p]),
    'zigp_predict': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), dp, C.c_int64, C.c_double, C.c_double, dp]),
    'zigp_predict_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p]),
    'zigp_prior_kl': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_double, dp]),
    'zigp_rbf_K': (C.c_int, [C.c_void_p, dp, C.c_int64, dp, C.c_int64, C.c_int32, dp, C.c_double, dp]),
    'zigp_kron_elbo': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), dp, dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_int32, dp, dp, C.POINTER(zigp_kron_grads), dp]),
    'zigp_kron_elbo_rows': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_int32, dp, dp, C.POINTER(zigp_kron_grads), dp]),
    'zigp_kron_fit_steps': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.POINTER(zigp_kron_fit_opts), dp, dp, dp, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_void_p, C.c_int64, dp, dp, C.c_double, C.c_double, C.c_int32, dp, dp]),
    'zigp_kron_fit_steps_applied': (C.c_int64, [C.c_void_p]),
    'zigp_test_trmm_list': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    'zigp_test_kgmom_list': (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    'zigp_test_sk_list': (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    'zigp_kron_predict': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), dp, C.c_int64, C.c_double, C.c_double, C.c_double, dp]),
    'zigp_get_chunk': (C.c_int64, [C.c_void_p, C.c_int32]),
    'zigp_get_chunk_rows': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64]),
    'zigp_set_pivot_rtol': (C.c_int, [C.c_void_p, C.c_double]),
    'zigp_comm_unique_id': (C.c_int, [C.c_void_p]),
    'zigp_comm_init': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'zigp_comm_destroy': (C.c_int, [C.c_void_p]),
    'zigp_comm_available': (C.c_int, [C.POINTER(C.c_int32)]),
    'zigp_comm_set_timeout': (C.c_int, [C.c_void_p, C.c_double]),
    'zigp_comm_allreduce_host': (C.c_int, [C.c_void_p, dp, C.c_int64]),
    'zigp_comm_info': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'zigp_set_overlap': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_set_kron_panels': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_set_kron_range_tiles': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_set_mean_function': (C.c_int, [C.c_void_p, dp, C.c_int32, C.c_double]),
    'zigp_get_mean_function_grad': (C.c_int, [C.c_void_p, dp, C.c_int32, dp]),
    'zigp_set_whiten': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_get_whiten': (C.c_int, [C.c_void_p]),
    'zigp_set_q_full': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_get_q_full': (C.c_int, [C.c_void_p]),
    'zigp_set_kernel': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'zigp_get_kernel': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_set_kron_kernel': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    'zigp_get_kron_kernel': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'zigp_set_kron_matern_fused': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_get_kron_matern_fused': (C.c_int, [C.c_void_p]),
    'zigp_kern_K': (C.c_int, [C.c_void_p, C.c_int32, dp, C.c_int64, dp, C.c_int64, C.c_int32, dp, C.c_double, dp]),
    'zigp_kron_head_elbo': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, dp, dp, C.c_int64, C.c_double, C.c_double,
                                      C.c_double, C.c_int32, dp, dp, C.POINTER(zigp_kron_grads), dp]),
    'zigp_kron_head_elbo_rows': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                           C.c_double, C.c_int32, dp, dp, C.POINTER(zigp_kron_grads), dp]),
    'zigp_kron_head_fit_steps': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, C.POINTER(zigp_kron_head_fit_opts), dp, dp, dp, C.c_int64,
                                           C.c_int64, C.c_int32, C.c_void_p, C.c_int64, dp, dp, C.c_double, C.c_double, C.c_int32, dp, dp]),
    'zigp_kron_head_predict': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, dp, C.c_int64, C.c_double, C.c_double, dp]),
    'zigp_head_elbo': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_int64, C.c_int32, dp, dp,
                                 C.POINTER(zigp_grads)]),
    'zigp_head_predict': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_int32, dp, C.c_int64, C.c_double, dp]),
    'zigp_head_predict_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]),
    'zigp_density_rows': (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, C.c_int64, C.c_double, dp, dp, C.c_int32, dp, dp]),
    'zigp_predict_density': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), dp, dp, C.c_int64, C.c_double, C.c_double, dp, dp, C.c_int32, dp, dp]),
    'zigp_predict_density_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                              dp, dp, C.c_int32, C.c_void_p, dp]),
    'zigp_density_rows_centred': (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp, C.c_int64, C.c_double, dp, dp, C.c_int32, dp, dp, dp]),
    'zigp_predict_density_centred': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), dp, dp, C.c_int64, C.c_double, C.c_double, dp, dp, C.c_int32,
                                               dp, dp, dp]),
    'zigp_predict_density_centred_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                                      dp, dp, C.c_int32, C.c_void_p, dp, C.c_void_p]),
    'zigp_score_rows': (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, C.c_int64, C.c_double, dp, dp, C.c_int32, dp, C.c_int32, dp, dp, dp, dp]),
    'zigp_predict_scores': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), dp, dp, C.c_int64, C.c_double, C.c_double, dp, dp, C.c_int32, dp, C.c_int32,
                                      dp, dp, dp, dp]),
    'zigp_predict_scores_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                             dp, dp, C.c_int32, dp, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, dp]),
    'zigp_path_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int64, dp]),
    'zigp_path_rows_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'zigp_sample_paths': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), dp, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, dp]),
    'zigp_sample_paths_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_void_p]),
    'zigp_kmeans': (C.c_int, [C.c_void_p, dp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int32, C.c_void_p, C.c_void_p, dp,
                              C.POINTER(C.c_int32)]),
    'zigp_kmeans_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int32, C.c_void_p,
                                     C.c_void_p, dp, C.POINTER(C.c_int32)]),
    'zigp_kmeans_resident': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int32, C.c_void_p, C.c_void_p, dp, C.POINTER(C.c_int32)]),
    'zigp_profile_enable': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_profile_get': (C.c_int, [C.c_void_p, dp, C.POINTER(C.c_int64), dp]),
    'zigp_profile_reset': (C.c_int, [C.c_void_p]),
    'zigp_profile_totals': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'zigp_profile_sampling': (C.c_int, [C.c_void_p, C.c_int32]),
    'zigp_clock_stamp': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'zigp_test_gemm': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp]),
    'zigp_test_kuf': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, dp, dp, dp, C.c_double, dp]),
    'zigp_test_potrf_trtri': (C.c_int, [C.c_void_p, C.c_int64, dp, dp, dp, C.c_int32]),
    'zigp_test_potrf_stages': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_potrf)]),
    'zigp_test_chunk_forward': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(zigp_stage_latent), C.POINTER(C.c_int64)]),
    'zigp_test_latents_forward': (C.c_int, [C.c_void_p, C.POINTER(zigp_params), C.c_double, C.c_int32, C.POINTER(dp), C.POINTER(dp)]),
    'zigp_test_pointwise': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_pointwise)]),
    'zigp_test_chunk_forward_white': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(zigp_stage_latent), C.POINTER(C.c_int64)]),
    'zigp_test_pointwise_white': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_pointwise)]),
    'zigp_test_pointwise_head': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(zigp_stage_pointwise)]),
    'zigp_test_q_full_forward': (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp]),
    'zigp_test_q_full_dlq': (C.c_int, [C.c_void_p, C.c_int32, dp, dp, C.c_int32, dp]),
    'zigp_test_kgrad': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int32, dp]),
    'zigp_test_kuf_kind': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, dp, dp, dp, C.c_double, dp, dp]),
    'zigp_test_kgrad_kind': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp, dp]),
    'zigp_test_rank_update': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(dp), C.POINTER(dp), dp, C.POINTER(C.c_int64)]),
    'zigp_test_mxm_backward': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_mxm)]),
    'zigp_test_dense_pack': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_pack)]),
    'zigp_test_kron_pointwise': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_kron_pointwise)]),
    'zigp_test_kron_fused_step': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_kron_fused)]),
    'zigp_test_kron_panel_step': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_kron_panels)]),
    'zigp_test_kron_fit_update': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_kron_fit_update)]),
    'zigp_test_dense_fit_update': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_dense_fit_update)]),
    'zigp_test_path_weights': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_path_weights)]),
    'zigp_test_kron_path_weights': (C.c_int, [C.c_void_p, C.POINTER(zigp_stage_kron_path_weights)]),
    'zigp_test_kron_kbuild': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, C.c_double, dp]),
    'zigp_test_kron_colsum': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp]),
    'zigp_test_kron_da': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, dp, dp, dp, dp, dp, dp, dp]),
    'zigp_test_kron_kgrad': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, dp, dp, dp, dp]),
    'zigp_test_kron_kbuild_kind': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, dp, dp,
                                             C.c_double, dp, dp]),
    'zigp_test_kron_kgrad_kind': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, dp, dp, dp, dp, dp,
                                            dp, dp, dp, dp, dp]),
}

# include/zigp_kronpaths.h (the header zigp.h includes for the Kronecker sample paths): bound by load() like SIGNATURES
KRON_PATH_SIGNATURES = {
    'zigp_kron_path_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int64, dp]),
    'zigp_kron_path_rows_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    'zigp_kron_sample_paths': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_int32, dp]),
    'zigp_kron_sample_paths_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'zigp_kron_head_sample_paths': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, dp, C.c_int64, C.c_double, C.c_double, C.c_void_p,
                                              C.c_int32, dp]),
    'zigp_kron_head_sample_paths_device': (C.c_int, [C.c_void_p, C.POINTER(zigp_kron_params), C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                                     C.c_void_p, C.c_int32, C.c_void_p]),
}

# include/zigp_ensemble.h (the header zigp.h includes for the sample-path scores): bound by load() like SIGNATURES
ENS_CHUNK = 64                # ZIGP_ENS_CHUNK
ENS_VARIO_MAX_ROWS = 4096     # ZIGP_ENS_VARIO_MAX_ROWS


class zigp_ens_opts(C.Structure):
    _fields_ = [('fair', C.c_int32), ('vario_p', C.c_double)]


_ENS_ARGS = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32,
             C.POINTER(zigp_ens_opts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
ENSEMBLE_SIGNATURES = {
    'zigp_ensemble_scores': (C.c_int, _ENS_ARGS),
    'zigp_ensemble_scores_device': (C.c_int, _ENS_ARGS),
}

_lib = None


def load():
    """Load libzigp.so; raises ZigpError when it has not been built (there is NO CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZigpError('libzigp.so not found at %s: build it first (python __graft_entry__.py / zigp.build.build()). '
                        'This engine has no CPU fallback.' % LIB_PATH)
    # PyTorch wheels bundle their own libamdhip64; a process must not end up with two HIP runtimes (the second one sees
    # no GPUs).  Loading torch's copy first lets libzigp.so bind to the same runtime, so engine buffers and torch tensors
    # (zigp_set_data_device, the all-reduce buffer) live in one context.  Without torch the system runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(KRON_PATH_SIGNATURES.items()) + list(ENSEMBLE_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def as_f64(a, shape=None):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def ptr(a):
    """address of a float64 C-contiguous array (the caller keeps the array alive for the duration of the call)"""
    return a.ctypes.data
