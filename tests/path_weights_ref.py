"""Restatements of the weight stage of the sample paths (csrc/zigp_paths.hip path_weight_stage, csrc/zigp_kronpaths.hip
kron_path_weight_stage; the taps of zigp_test_path_weights / zigp_test_kron_path_weights, include/zigp_diag.h), shared by
test_cpu_path_weights_ref.py and test_gpu_path_weight_stages.py: every launch in plain NumPy on the operands it is handed, in float64 and in
numpy.longdouble, with the error weight S = sum |a| |b| of every element of a product (as kronf_ref.py); the whole sequences built from
them, with the deliberate mistakes of the CPU test's catalogue; the acceptance rules of the three tiers; and the fixtures both files use.

All operands here are the LIVE parts: (M, M) matrices, (M, S) right-hand sides (the device pads M to 128 rows by the identity and S to
128 columns by zeros; the padding is judged on its own, exactly)."""
import functools
import math
from collections import OrderedDict

import numpy as np

import paths_ref as pr
import kronpaths_ref as kr
from zigp import pathwise

EPS = pr.EPS
LD = np.longdouble
SENT = float(np.frombuffer(bytes([0x7f]) * 8, dtype=np.float64)[0])      # ZIGP_STAGE_SENTINEL_BYTE in every byte
BAR = 8.0            # residual of a solve against SciPy's Cholesky solve of the same operands: the project's bar for P_p


def rup(n, k):
    return -(-n // k) * k


def tiles(S):
    """(sample tiles per pass, tiles in the table) of S samples: path_tiles_per_pass and its round-up"""
    nt = -(-S // 16)
    nst = 4 if nt >= 4 else 2 if nt >= 2 else 1
    return nst, rup(nt, nst)


def _a(x, dt):
    return np.asarray(x, dtype=dt)


# ---- the launches -------------------------------------------------------------------------------------------------------------------------
def gemm(A, B, dt=np.float64):
    """(A B, S = |A| |B|) in dt"""
    A, B = _a(A, dt), _a(B, dt)
    return A @ B, np.abs(A) @ np.abs(B)


def rhs_diag(u, s, E, fZ, dt=np.float64):
    """k_path_rhs mode 0: (u + s o E) - f_Z, f_Z (M, S)"""
    return (_a(u, dt).reshape(-1, 1) + _a(s, dt).reshape(-1, 1) * _a(E, dt)) - _a(fZ, dt)


def rhs_white(u, s, E, G, dt=np.float64):
    """k_path_rhs mode 1: (u + s o E) - G"""
    return (_a(u, dt).reshape(-1, 1) + _a(s, dt).reshape(-1, 1) * _a(E, dt)) - _a(G, dt)


def rhs_full(u, H, G, dt=np.float64):
    """k_path_rhs mode 2: (u + H) - G"""
    return (_a(u, dt).reshape(-1, 1) + _a(H, dt)) - _a(G, dt)


def fill_v(V, M4, tab):
    """k_path_fill_v on a table (ntile, F, 16) that holds the host's staging: rows < M4 take V (M, S), zero behind M and behind S"""
    V = np.asarray(V)
    M, S = V.shape
    out = np.array(tab, dtype=V.dtype)
    pad = np.zeros((M4, out.shape[0] * 16), dtype=V.dtype)
    pad[:M, :S] = V
    out[:, :M4, :] = pad.reshape(M4, out.shape[0], 16).transpose(1, 0, 2)
    return out


def staged_tab(a, var, R4, M4, S):
    """The table as the host stages it: zeros in the kernel rows, a sqrt(2 var / R) in the cosine rows (a (R, S))"""
    a = np.asarray(a, dtype=np.float64)
    R = a.shape[0]
    ntile = tiles(S)[1]
    tab = np.zeros((ntile, M4 + R4, 16))
    if R:
        amp = np.zeros((R4, ntile * 16))
        amp[:R, :S] = a * math.sqrt(2.0 * var / R)
        tab[:, M4:, :] = amp.reshape(R4, ntile, 16).transpose(1, 0, 2)
    return tab


# ---- the dense sequence ---------------------------------------------------------------------------------------------------------------------
DENSE_MUTATIONS = ('no_refine', 'cor_sub', 'no_jitter', 'wwt', 'plus_fz', 's_squared', 'e_stride', 'tile_shift', 'tab_unzeroed')


def dense_sequence(mode, Kuu, W, u, s, E, fZ, tab0, Lq=None, dt=np.float64, mutate=None, jitter=0.0):
    """Every launch of path_weight_stage for one latent, each on the OUTPUT of the one before: dict name -> value (the names of the
    hook's taps; FT is fZ transposed), plus 'S_' + name for the products.  mode 0 Diag, 1 White, 2 WhiteFull.  mutate: one of
    DENSE_MUTATIONS -- the float64 sequence with that mistake stands in for a wrong device in the CPU test."""
    M, S = np.shape(E)
    o = {}
    W_, Kuu_ = _a(W, dt), _a(Kuu, dt)
    Ein = np.asarray(E, dtype=np.float64)
    if mutate == 'e_stride':      # E (Mp, Sp) read as if its row stride were S
        Sp = rup(S, 128)
        flat = np.zeros((M, Sp))
        flat[:, :S] = Ein
        Ein = flat.reshape(-1)[:M * S].reshape(M, S)
    sd = np.asarray(s, dtype=np.float64)
    if mutate == 's_squared':
        sd = sd * sd
    first, second = (W_.T, W_) if mutate == 'wwt' else (W_, W_.T)      # the solve is second (first rhs)
    if mode == 0:
        o['rhs'] = rhs_diag(u, sd, Ein, -_a(fZ, dt) if mutate == 'plus_fz' else fZ, dt)
        o['t'], o['S_t'] = gemm(first, o['rhs'], dt)
        o['V0'], o['S_V0'] = gemm(second, o['t'], dt)
        o['KV'], o['S_KV'] = gemm(Kuu_ - dt(jitter) * np.eye(M, dtype=dt) if mutate == 'no_jitter' else Kuu_, o['V0'], dt)
        o['res'] = o['rhs'] - o['KV']
        o['t2'], o['S_t2'] = gemm(first, o['res'], dt)
        o['cor'], o['S_cor'] = gemm(second, o['t2'], dt)
        o['V'] = o['V0'] if mutate == 'no_refine' else o['V0'] - o['cor'] if mutate == 'cor_sub' else o['V0'] + o['cor']
    else:
        o['G'], o['S_G'] = gemm(W_, fZ, dt)
        if mode == 2:
            o['H'], o['S_H'] = gemm(np.tril(_a(Lq, dt)), Ein, dt)
            o['rhs'] = rhs_full(u, o['H'], -o['G'] if mutate == 'plus_fz' else o['G'], dt)
        else:
            o['rhs'] = rhs_white(u, sd, Ein, -o['G'] if mutate == 'plus_fz' else o['G'], dt)
        o['V'], o['S_V'] = gemm(first.T if mutate == 'wwt' else W_.T, o['rhs'], dt)
    M4 = rup(M, 4)
    V = np.asarray(o['V'], dtype=np.float64)
    if mutate == 'tile_shift':
        V = np.concatenate([V[:, 16:], np.zeros((M, 16))], axis=1)[:, :S] if S > 16 else V
    o['tab'] = fill_v(V, M4, tab0)
    if mutate == 'tab_unzeroed':
        o['tab'][:, M:M4, :] = SENT
    return o


def residual_ld(Kuu, rhs, V):
    """max |rhs - Kuu V| in long double"""
    return float(np.max(np.abs(_a(rhs, LD) - _a(Kuu, LD) @ _a(V, LD))))


def scipy_solve(Kuu, rhs):
    from scipy.linalg import cho_factor, cho_solve
    return cho_solve(cho_factor(np.asarray(Kuu, dtype=np.float64), lower=True), np.asarray(rhs, dtype=np.float64))


def solve_ratio(Kuu, rhs, V):
    """r(V) / r(V_scipy): the dense solve tier's figure (the bar is BAR)"""
    return residual_ld(Kuu, rhs, V) / max(residual_ld(Kuu, rhs, scipy_solve(Kuu, rhs)), 1e-300)


# ---- the acceptance rules -------------------------------------------------------------------------------------------------------------------
def bound_ok(got, ref64, truth, Sw):
    """(ok, largest err / (eps S)) of the standing rule err <= 4 err_np + 16 eps S per element"""
    truth = _a(truth, LD)
    err, err_np = np.abs(_a(got, LD) - truth), np.abs(_a(ref64, LD) - truth)
    Sw = _a(Sw, LD)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(Sw > 0, err / (EPS * Sw), np.where(err == 0, 0.0, np.inf))
    return bool(np.all(err <= 4 * err_np + 16 * EPS * Sw)), float(np.max(ratio)) if ratio.size else 0.0


def exact_ok(got, want):
    """== everywhere and no sentinel left"""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    return bool(got.shape == want.shape and np.array_equal(got, want) and not np.any(got == SENT))


def check_dense(mode, inp, out, dyadic=True):
    """The three tiers on one latent: inp the stage's inputs (Kuu, W, u, s, E, fZ, tab0, Lq), out the outputs under judgement (the
    device's taps, or a sequence of dense_sequence).  Every launch is restated on ITS inputs as `out` holds them.  dyadic: u, s and eps
    are multiples of 2^-8, 2^-8 and 2^-10 below 8, so that fma(s, eps, u) and s eps + u are the same number and k_path_rhs is judged with
    ==; with real values (the solve tier's fixtures) its two roundings are judged by the bound rule with S = |u| + |s| |eps| + |f_Z|.
    Returns (failures: list of 'tier:launch', figures: dict launch -> err / (eps S), or the solve ratio under 'solve')."""
    fail, fig = [], {}
    Kuu, W, u, s, E, fZ = (inp[k] for k in ('Kuu', 'W', 'u', 's', 'E', 'fZ'))
    M = np.shape(E)[0]

    def product(name, A, B):
        ok, fig[name] = bound_ok(out[name], gemm(A, B)[0], *gemm(A, B, LD))
        if not ok:
            fail.append('bound:' + name)

    def exact(name, want):
        if not exact_ok(out[name], want):
            fail.append('exact:' + name)

    def rhs_rule(f, *args):
        if dyadic:
            return exact('rhs', f(*args))
        Sw = np.abs(np.asarray(u)).reshape(-1, 1) + np.abs(np.asarray(s)).reshape(-1, 1) * np.abs(E) + np.abs(args[-1])
        ok, fig['rhs'] = bound_ok(out['rhs'], f(*args), f(*args, dt=LD), Sw)
        if not ok:
            fail.append('bound:rhs')

    if mode == 0:
        rhs_rule(rhs_diag, u, s, E, fZ)
        product('t', W, out['rhs'])
        product('V0', np.asarray(W).T, out['t'])
        product('KV', Kuu, out['V0'])
        exact('res', np.asarray(out['rhs']) - np.asarray(out['KV']))
        product('t2', W, out['res'])
        product('cor', np.asarray(W).T, out['t2'])
        exact('V', np.asarray(out['V0']) + np.asarray(out['cor']))
        fig['solve'] = solve_ratio(Kuu, out['rhs'], out['V'])
        if not fig['solve'] <= BAR:
            fail.append('solve:V')
    else:
        product('G', W, fZ)
        if mode == 2:
            product('H', np.tril(inp['Lq']), E)
            exact('rhs', rhs_full(u, out['H'], out['G']))
        else:
            rhs_rule(rhs_white, u, s, E, out['G'])
        product('V', np.asarray(W).T, out['rhs'])
    exact('tab', fill_v(np.asarray(out['V'], dtype=np.float64), rup(M, 4), inp['tab0']))
    return fail, fig


# ---- the Kronecker launches and sequence ----------------------------------------------------------------------------------------------------
def kp_left(A, X, ta=False, dt=np.float64):
    """k_kp_left: Y_s = op(A) X_s, X (S, M0, M1), k ascending; (Y, S = |op A| |X|)"""
    A, X = _a(A, dt), _a(X, dt)
    A = A.T if ta else A
    Y, Sw = np.zeros(X.shape, dtype=dt), np.zeros(X.shape, dtype=dt)
    for k in range(A.shape[1]):
        term = A[None, :, k, None] * X[:, k, None, :]
        Y, Sw = Y + term, Sw + np.abs(term)
    return Y, Sw


def kp_right(X, B, tb=False, dt=np.float64):
    """k_kp_right: Y_s = X_s op(B), k ascending; (Y, S)"""
    X, B = _a(X, dt), _a(B, dt)
    B = B.T if tb else B
    Y, Sw = np.zeros(X.shape, dtype=dt), np.zeros(X.shape, dtype=dt)
    for k in range(B.shape[0]):
        term = X[:, :, k, None] * B[None, None, k, :]
        Y, Sw = Y + term, Sw + np.abs(term)
    return Y, Sw


def kp_rhs(U, Sq, E, FZ, dt=np.float64):
    """k_kp_rhs: rhs[s] = (U + Sq o E_s) - FZ_s as (S, M0, M1); E (M, S) as the draw holds it"""
    S, M0, M1 = np.shape(FZ)
    Es = _a(E, dt).T.reshape(S, M0, M1)
    return (_a(U, dt).reshape(1, M0, M1) + _a(Sq, dt).reshape(1, M0, M1) * Es) - _a(FZ, dt)


def kp_fill_v(V, tab):
    """k_kp_fill_v: tab[tile][i M1p + j][c] = V[16 tile + c][i][j], zero for j >= M1 and behind S"""
    V = np.asarray(V, dtype=np.float64)
    S, M0, M1 = V.shape
    M1p = rup(M1, 4)
    out = np.array(tab, dtype=np.float64)
    pad = np.zeros((out.shape[0] * 16, M0, M1p))
    pad[:S, :, :M1] = V
    out[:, :M0 * M1p, :] = pad.reshape(out.shape[0], 16, M0 * M1p).transpose(0, 2, 1)
    return out


def kron_staged_tab(a, var0, var1, M0, M1, R4, S):
    a = np.asarray(a, dtype=np.float64)
    R, ntile, coff = a.shape[0], tiles(S)[1], M0 * rup(M1, 4)
    tab = np.zeros((ntile, coff + R4, 16))
    if R:
        amp = np.zeros((R4, ntile * 16))
        amp[:R, :S] = a * math.sqrt(2.0 * (var0 * var1) / R)
        tab[:, coff:, :] = amp.reshape(R4, ntile, 16).transpose(1, 0, 2)
    return tab


KRON_MUTATIONS = ('w1_not_transposed', 'swap_left_right', 'fill_ij')


def _padI(W, n):
    out = np.eye(n, dtype=np.asarray(W).dtype)
    m = min(n, np.shape(W)[0])
    out[:m, :m] = np.asarray(W)[:m, :m]
    return out


def kron_sequence(W0, W1, U, Sq, E, FZ, tab0, dt=np.float64, mutate=None):
    """Every launch of kron_path_weight_stage for one latent, each on the output of the one before (names of the hook's taps)"""
    S, M0, M1 = np.shape(FZ)
    o = {'rhs': kp_rhs(U, Sq, E, FZ, dt)}
    if mutate == 'swap_left_right':      # W1 from the left and W0 from the right: each read at the other's size out of its identity-padded image
        A, B = _padI(_a(W1, dt), M0), _padI(_a(W0, dt), M1)
    else:
        A, B = _a(W0, dt), _a(W1, dt)
    o['A1'], o['S_A1'] = kp_left(A, o['rhs'], False, dt)
    o['B1'], o['S_B1'] = kp_right(o['A1'], B, mutate != 'w1_not_transposed', dt)
    o['A2'], o['S_A2'] = kp_left(A, o['B1'], True, dt)
    o['V'], o['S_V'] = kp_right(o['A2'], B, False, dt)
    V = np.asarray(o['V'], dtype=np.float64)
    if mutate == 'fill_ij':              # V read at [j][i]: index j M1 + i of the sample's M0 M1 block, kept inside it
        i, j = np.meshgrid(np.arange(M0), np.arange(M1), indexing='ij')
        V = V.reshape(S, -1)[:, np.minimum(j * M1 + i, M0 * M1 - 1)]
    o['tab'] = kp_fill_v(V, tab0)
    return o


def kron_residual(K0, K1, rhs, V, dt):
    """(rhs_s - K0 V_s K1, S_w = |K0| |V_s| |K1| + |rhs_s|) in dt, the products in the kernels' order"""
    KV, _ = kp_left(K0, V, False, dt)
    KVK, _ = kp_right(KV, K1, False, dt)
    a, _ = kp_left(np.abs(K0), np.abs(V), False, dt)
    Sw, _ = kp_right(a, np.abs(K1), False, dt)
    return _a(rhs, dt) - KVK, Sw + np.abs(_a(rhs, dt))


def check_kron(inp, out, dyadic=True):
    """The tiers on one Kronecker latent: inp (K, W: pairs of live matrices; U, Sq, E, FZ, tab0), out the outputs under judgement.
    dyadic: as check_dense -- k_kp_rhs with == (dyadic u, s, eps) or under the bound rule with S = |U| + |Sq| |E_s| + |FZ_s|.
    Returns (failures, figures); the solve rule is res <= 4 res_np + 16 eps S_w per element, res_np the float64 sequence on the same W_p"""
    fail, fig = [], {}
    (K0, K1), (W0, W1) = inp['K'], inp['W']

    def product(name, f, *args):
        ok, fig[name] = bound_ok(out[name], f(*args)[0], *f(*args, dt=LD))
        if not ok:
            fail.append('bound:' + name)

    rhs64 = kp_rhs(inp['U'], inp['Sq'], inp['E'], inp['FZ'])
    if dyadic:
        if not exact_ok(out['rhs'], rhs64):
            fail.append('exact:rhs')
    else:
        S_, M0_, M1_ = rhs64.shape
        Sw = (np.abs(inp['U']).reshape(1, M0_, M1_) + np.abs(inp['Sq']).reshape(1, M0_, M1_) * np.abs(np.asarray(inp['E']).T.reshape(S_, M0_, M1_))
              + np.abs(inp['FZ']))
        ok, fig['rhs'] = bound_ok(out['rhs'], rhs64, kp_rhs(inp['U'], inp['Sq'], inp['E'], inp['FZ'], LD), Sw)
        if not ok:
            fail.append('bound:rhs')
    product('A1', kp_left, W0, out['rhs'], False)
    product('B1', kp_right, out['A1'], W1, True)
    product('A2', kp_left, W0, out['B1'], True)
    product('V', kp_right, out['A2'], W1, False)
    if not exact_ok(out['tab'], kp_fill_v(out['V'], inp['tab0'])):
        fail.append('exact:tab')
    res, Sw = kron_residual(K0, K1, out['rhs'], out['V'], LD)
    ref = kron_sequence(W0, W1, inp['U'], inp['Sq'], inp['E'], inp['FZ'], inp['tab0'])
    res_np = kron_residual(K0, K1, ref['rhs'], ref['V'], LD)[0]
    fig['solve'] = float(np.max(np.abs(res) / (EPS * Sw)))
    fig['solve_np'] = float(np.max(np.abs(res_np) / (EPS * Sw)))
    if not np.all(np.abs(res) <= 4 * np.abs(res_np) + 16 * EPS * Sw):
        fail.append('solve:V')
    return fail, fig


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def quantise(a, bits):
    """Multiples of 2^-bits of magnitude below 8: products and sums of two such numbers are exact in float64"""
    return np.clip(np.round(np.asarray(a, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits, -7.5, 7.5)


def _case(shape, S, mode, R, kern=None, quant=True):
    return dict(shape=shape, S=S, mode=mode, R=R, kern=kern or {}, quant=quant)


# name -> (N, Mf, Mg, D) of matern_ref.problem, S, mode, R.  Every M pair at S = 20 (one, two and three 128-row blocks, heavy and no padding);
# every S at (50, 37) (1 .. 4 sample tiles, 33 -> three tiles rounded up to four; one and two 128-column blocks); every mode at (129, 137),
# S = 129.  Mf != Mg and S != M wherever the Diag mode's transposed f_Z read could otherwise match by accident.
DENSE_CASES = OrderedDict([
    ('m1_1', _case((12, 1, 1, 1), 20, 0, 8)),
    ('m50_37', _case((100, 50, 37, 3), 20, 0, 64)),
    ('m128_128', _case((300, 128, 128, 2), 20, 1, 8)),
    ('m129_137', _case((300, 129, 137, 3), 20, 2, 8)),
    ('m260_129', _case((400, 260, 129, 3), 20, 0, 8)),
    ('s1', _case((100, 50, 37, 3), 1, 0, 0)),
    ('s16', _case((100, 50, 37, 3), 16, 1, 0)),
    ('s17', _case((100, 50, 37, 3), 17, 2, 8)),
    ('s33_matern', _case((100, 50, 37, 3), 33, 0, 8, dict(kern_f='matern32', kern_g='matern52'))),
    ('s128', _case((100, 50, 37, 3), 128, 1, 8)),
    ('s129', _case((100, 50, 37, 3), 129, 2, 0)),
    ('s256', _case((100, 50, 37, 3), 256, 0, 8)),
    ('modes_diag', _case((300, 129, 137, 3), 129, 0, 8)),
    ('modes_white', _case((300, 129, 137, 3), 129, 1, 8)),
    ('modes_full', _case((300, 129, 137, 3), 129, 2, 8)),
    # the solve tier's fixtures: real u, s and eps.  (700, 137, 137, 1): cond(Kuu) about 4e8
    ('solve_1d', _case((700, 137, 137, 1), 20, 0, 200, quant=False)),
    ('solve_3d', _case((1500, 50, 37, 3), 20, 0, 200, dict(kern_f='matern52'), quant=False)),
])
DENSE_JITTER = 1e-6


@functools.lru_cache(maxsize=None)
def dense_problem(name):
    """(p, draws) of a dense case: computed once, shared, read-only"""
    import matern_ref as mr
    import fullcov_ref as fr
    k = DENSE_CASES[name]
    X, Y, p = mr.problem(*k['shape'])
    p = dict(p, **k['kern'])
    if k['quant']:
        for t in 'fg':
            p['u_%sm' % t] = quantise(p['u_%sm' % t], 8)
            p['u_%ss_sqrt' % t] = np.maximum(quantise(p['u_%ss_sqrt' % t], 8), 2.0 ** -8)
    if k['mode'] == 2:
        p = fr.make_lq(p, seed=3, negative=2)
    elif k['mode'] == 1:
        p = dict(p, whiten=True)
    rs = np.random.RandomState(9 + sum(map(ord, name)))
    D = p['Zf'].shape[1]
    draws = {t: pathwise.draw(p.get('kern_' + t, 'rbf'), k['R'], D, p['Z' + t].shape[0], k['S'], rs) for t in 'fg'}
    if k['quant']:
        for t in 'fg':
            draws[t]['eps'] = quantise(draws[t]['eps'], 10)
    for d in list(draws.values()) + [p]:
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return p, draws


def dense_host_inputs(name, tag):
    """The stage's inputs of latent `tag` restated on the host in float64 -- what the CPU test feeds the sequences in place of the taps:
    Kuu = k(Z, Z) + jitter I, W = L^-1 by a triangular solve, fZ = f_prior(Z) (M, S), the staged table"""
    from scipy.linalg import solve_triangular
    p, draws = dense_problem(name)
    k = DENSE_CASES[name]
    Z = np.asarray(p['Z' + tag], dtype=np.float64)
    M, D = Z.shape
    ell = np.broadcast_to(np.asarray(p['ell_' + tag], dtype=np.float64).reshape(-1), (D,))
    var = float(np.squeeze(p['var_' + tag]))
    Kuu = pr.kern_np(p.get('kern_' + tag, 'rbf'), Z, Z, ell, var) + DENSE_JITTER * np.eye(M)
    W = solve_triangular(np.linalg.cholesky(Kuu), np.eye(M), lower=True)
    d = draws[tag]
    R4 = rup(int(d['R']), 4)
    sq = np.asarray(p['u_%ss_sqrt' % tag], dtype=np.float64)
    inp = dict(Kuu=Kuu, W=W, u=np.asarray(p['u_%sm' % tag], dtype=np.float64).reshape(-1), E=np.asarray(d['eps']),
               fZ=pathwise.prior_np(Z, ell, var, d).T, tab0=staged_tab(d['a'], var, R4, rup(M, 4), k['S']))
    if k['mode'] == 2:
        inp['Lq'], inp['s'] = sq.reshape(M, M), np.diag(sq.reshape(M, M)).copy()
    else:
        inp['s'] = sq.reshape(-1)
    return inp


def dense_tap_inputs(name, h, tap):
    """The same dict from the hook's taps of latent h (engine.test_path_weights): the live parts of the padded device images"""
    p, draws = dense_problem(name)
    tag = 'fg'[h]
    M, S = p['Z' + tag].shape[0], DENSE_CASES[name]['S']
    inp = dict(Kuu=tap['Kuu'][:M, :M], W=tap['W'][:M, :M], u=tap['u'][:M], s=tap['s'][:M], E=tap['E'][:M, :S], fZ=tap['FT'][:S, :M].T,
               tab0=staged_tab(draws[tag]['a'], float(np.squeeze(p['var_' + tag])), rup(int(draws[tag]['R']), 4), rup(M, 4), S))
    if 'Lq' in tap:
        inp['Lq'] = tap['Lq'][:M, :M]
    return inp


# Kronecker: name -> grids per latent, (D0, D1), S, R, lik, kinds.  1 x 1; 3 x 5 (M1p pads 5 to 8); 32 x 32; 10 x 100; 16 x 112; 128 x 128 at
# S = 4; two latents with different grids; a Gaussian and a Bernoulli head; a Matern factor pair; S = 1, 17, 129 on the small grids; D0 + D1
# from 2 to 8.
KRON_CASES = OrderedDict([
    ('k1x1', dict(grids=[(1, 1), (3, 5)], D=(1, 1), S=1, R=8, lik='onoff')),
    ('k3x5_s17', dict(grids=[(3, 5), (5, 3)], D=(2, 1), S=17, R=0, lik='onoff')),
    ('k3x5_s129', dict(grids=[(3, 5)], D=(1, 3), S=129, R=8, lik='gaussian')),
    ('k32x32', dict(grids=[(32, 32), (10, 100)], D=(2, 3), S=17, R=8, lik='onoff')),
    ('k16x112', dict(grids=[(16, 112)], D=(3, 3), S=17, R=8, lik='bernoulli')),
    ('k10x100_matern', dict(grids=[(10, 100)], D=(3, 4), S=20, R=8, lik='gaussian', kinds=('matern32', 'matern52'))),
    ('k128x128', dict(grids=[(128, 128)], D=(4, 4), S=4, R=4, lik='gaussian')),
])
KRON_JITTER = 1e-5


@functools.lru_cache(maxsize=None)
def kron_problem(name):
    """(p, draws, tags) of a Kronecker case: inducing grids on [0, 1]^D_q with lengthscales of kronpaths_ref.random_latent, dyadic u, s and
    eps (the exact tier)"""
    k = KRON_CASES[name]
    rs = np.random.RandomState(300 + sum(map(ord, name)))
    D0, D1 = k['D']
    tags = 'fg'[:len(k['grids'])]
    p, draws = {}, {}
    for t, (M0, M1) in zip(tags, k['grids']):
        p['Z' + t] = [rs.rand(M0, D0), rs.rand(M1, D1)]
        p['ell_' + t] = [(0.25 + 0.2 * rs.rand(D0)) * math.sqrt(D0), (0.25 + 0.2 * rs.rand(D1)) * math.sqrt(D1)]
        p['var_' + t] = [1.0 + rs.rand(), 0.5 + rs.rand()]
        p['u_%sm' % t] = quantise(0.5 * rs.randn(M0 * M1, 1), 8)
        p['u_%ss_sqrt' % t] = np.maximum(quantise(0.3 + rs.rand(M0 * M1, 1), 8), 2.0 ** -8)
        p['noise'] = 0.01
        if k.get('kinds'):
            p['kern_' + t] = k['kinds']
        draws[t] = pathwise.kron_draw(k.get('kinds', 'rbf'), k['R'], D0, D1, M0, M1, k['S'], rs)
        draws[t]['eps'] = quantise(draws[t]['eps'], 10)
    return p, draws, tags


def kron_tap_inputs(p, draws, tag, tap, S):
    M0, M1 = p['Z' + tag][0].shape[0], p['Z' + tag][1].shape[0]
    d = draws[tag]
    v = [float(np.squeeze(x)) for x in p['var_' + tag]]
    return dict(K=[tap['K'][0][:M0, :M0], tap['K'][1][:M1, :M1]], W=[tap['W'][0][:M0, :M0], tap['W'][1][:M1, :M1]], U=tap['U'], Sq=tap['Sq'],
                E=tap['E'], FZ=tap['FZ'], tab0=kron_staged_tab(d['a'], v[0], v[1], M0, M1, rup(int(d['R']), 4), S))


def kron_host_inputs(p, draws, tag, jitter, S, kinds=None):
    """The Kronecker stage's inputs restated on the host (kinds: the factors' kernel names, default RBF): K_p + jitter I, W_p = L_p^-1, FZ"""
    from scipy.linalg import solve_triangular
    Z = p['Z' + tag]
    M0, M1 = Z[0].shape[0], Z[1].shape[0]
    d = draws[tag]
    v = [float(np.squeeze(x)) for x in p['var_' + tag]]
    kinds = kinds or ('rbf', 'rbf')
    K = [pr.kern_np(kinds[q], Z[q], Z[q], p['ell_' + tag][q], v[q]) + jitter * np.eye(Z[q].shape[0]) for q in range(2)]
    W = [solve_triangular(np.linalg.cholesky(Kq), np.eye(Kq.shape[0]), lower=True) for Kq in K]
    ell = np.concatenate([np.broadcast_to(np.asarray(p['ell_' + tag][q], dtype=np.float64).reshape(-1), (Z[q].shape[1],)) for q in range(2)])
    fZ = pathwise.prior_np(pathwise.kron_grid(Z[0], Z[1]), ell, v[0] * v[1], d)      # (S, M)
    return dict(K=K, W=W, U=np.asarray(p['u_%sm' % tag], dtype=np.float64).reshape(-1), Sq=np.asarray(p['u_%ss_sqrt' % tag], dtype=np.float64).reshape(-1),
                E=np.asarray(d['eps']), FZ=fZ.reshape(S, M0, M1), tab0=kron_staged_tab(d['a'], v[0], v[1], M0, M1, rup(int(d['R']), 4), S))


KRON_SOLVE_CASES = tuple(kr.MODEL_CASES) + ('pptr32',)


@functools.lru_cache(maxsize=None)
def kron_solve_problem(name):
    """(p, draws, S, jitter) of a fixture of the Kronecker solve tier: a model case of kronpaths_ref with its seeded draws (R = 200,
    S = 20), or the precipitation data at the reference's initialisation on 32 x 32 inducing points (cond(K_s) about 5e7; R = 64, S = 20)"""
    import kron_nd
    if name != 'pptr32':
        return kron_nd.problem(name)[2], kr.model_draws(name), kr.MODEL_S, kr.MODEL_JITTER
    p = kron_nd.pptr_problem((32, 32))[4]
    rs = np.random.RandomState(77)
    draws = {}
    for t in 'fg':
        Z0, Z1 = p['Z' + t]
        draws[t] = pathwise.kron_draw('rbf', 64, Z0.shape[1], Z1.shape[1], Z0.shape[0], Z1.shape[0], 20, rs)
    return p, draws, 20, kr.MODEL_JITTER
