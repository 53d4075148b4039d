"""Kronecker (space x time) problems at ANY column split (D0, D1), shared by test_cpu_kron_nd.py and test_gpu_kron_nd.py.

* `make_kron_problem_nd` is the generator: D0 "spatial" columns on [0, 10], D1 "temporal" columns on [0, 1], ~60 % exact zeros in Y,
  lengthscales that follow the inducing spacing of each factor (so every dimension carries weight and the factor matrices stay
  well-conditioned).  test_gpu_kron.make_kron_problem (2 + 1 columns) stays what the older tests use.
* `CASES` is the table of factor dimensions / grids that walks every variant of the Kronecker kernels (the route of each case is the
  comment next to it; zigp_kronf.hip kf_plan decides it), `FIT_CASES` / `HEAD_FIT_CASES` the small fixtures of the device fit loops.
* `_factored_with_oracle_inverse`, `fixture_floor_and_cond` measure what the REFERENCE alone does on a fixture: the distance of the
  factored algebra from the literal dense order (the op-order floor) and cond(K_p + jitter).  test_cpu_kron_nd.py pins both for
  every case; the GPU tolerances of test_gpu_kron_nd.py mean something only because of that.
* `problem`, `oracle_predict`, `oracle_grad` cache a case's arrays and its oracle results: each is computed once per session, shared by
  the tests that need it and never written to.
* `BLOCK_CASES` (with `block_problem`, `block_oracle_predict`, `block_oracle_grad`, `BLOCK_EDGE_GRIDS`) are the grids beyond one 128-row
  block of the GEMM-panel path: test_cpu_kron_blocks.py pins them, test_gpu_kron_blocks.py and test_gpu_kron_panel_stages.py use them.
"""
import functools
from collections import OrderedDict

import numpy as np

JITTER = 1e-5
RANGE = (10.0, 1.0)       # range of a column of factor 0 / factor 1


def make_kron_problem_nd(N, M0, M1, D0, D1, seed, M0g=None, M1g=None, shift=0.0, c=1.2):
    """X: D0 columns uniform on [0, 10], then D1 columns uniform on [0, 1]; Y as make_kron_problem (~60 % exact zeros).
    Inducing inputs of a factor with D = 1: linspace(0, 1, M) + 0.3 / M randn, scaled to the factor's range; with D >= 2: uniform in
    the range.  Lengthscale per factor: c range Mmax^(-1/D) sqrt(D) (1 + 0.2 rand(D)), Mmax the larger of the f and g counts (g: 0.85
    of that, its own draw).  c: scalar or (c0, c1), one per factor -- smaller is better conditioned.  Variances, u_*, noise as
    make_kron_problem.  shift is added to every column of X and of the inducing inputs."""
    rs = np.random.RandomState(seed)
    D = (D0, D1)
    c = (float(c), float(c)) if np.isscalar(c) else (float(c[0]), float(c[1]))
    X = np.hstack([rs.rand(N, D0) * RANGE[0], rs.rand(N, D1) * RANGE[1]])
    f = np.sin(X[:, 0]) + np.cos(3 * X[:, D0])
    Y = np.where(rs.rand(N) > 0.6, np.abs(f + 0.3 * rs.randn(N)), 0.0)[:, None]
    M0g, M1g = M0g or M0, M1g or M1
    Mf, Mg = (M0, M1), (M0g, M1g)

    def inducing(M, q):
        if D[q] == 1:
            return (np.linspace(0, 1, M) + 0.3 / M * rs.randn(M))[:, None] * RANGE[q]
        return rs.rand(M, D[q]) * RANGE[q]

    def ell(q, k):
        Mmax = max(Mf[q], Mg[q])
        return k * c[q] * RANGE[q] * Mmax ** (-1.0 / D[q]) * np.sqrt(D[q]) * (1 + 0.2 * rs.rand(D[q]))

    p = dict(Zf=[inducing(M0, 0), inducing(M1, 1)], Zg=[inducing(M0g, 0), inducing(M1g, 1)],
             ell_f=[ell(0, 1.0), ell(1, 1.0)], ell_g=[ell(0, 0.85), ell(1, 0.85)],
             var_f=[np.array([2.0]), np.array([1.5])], var_g=[np.array([1.2]), np.array([0.9])],
             u_fm=0.1 * rs.randn(M0 * M1, 1), u_gm=0.1 * rs.randn(M0g * M1g, 1),
             u_fs_sqrt=0.5 + rs.rand(M0 * M1, 1), u_gs_sqrt=0.5 + rs.rand(M0g * M1g, 1), noise=0.05)
    if shift:
        X = X + shift
        p['Zf'] = [Z + shift for Z in p['Zf']]
        p['Zg'] = [Z + shift for Z in p['Zg']]
    return X, Y, p


def _case(D, f, g=None, N=300, c=1.2):
    return dict(D=D, f=f, g=g, N=N, c=c)


# id -> (D0, D1), f grid, g grid (None: as f), N (never a multiple of 16: a ragged last tile), c of the lengthscale recipe.
# c is tuned per case on the CPU (test_cpu_kron_nd.py) until the reference alone holds floor <= 1e-8 and cond <= 1e5.
CASES = OrderedDict([
    ('d11', _case((1, 1), (20, 24), N=300)),                                # small <2,2>, SPEC case 1 twice
    ('d11b', _case((1, 1), (32, 32), N=333)),                               # small <2,2>, full blocks, no padding rows
    ('d31', _case((3, 1), (32, 32), N=350, c=0.5)),                         # SPEC case 3
    ('d21-12', _case((2, 1), (10, 20), N=301, c=1.0)),                      # <1,2>
    ('d21-21', _case((2, 1), (20, 10), N=302, c=0.5)),                      # <2,1>
    ('d21-mix', _case((2, 1), (32, 32), (10, 12), N=375, c=0.5)),           # block counts differ: one launch per latent
    ('d21-mix2', _case((2, 1), (10, 30), (30, 10), N=345, c=0.8)),          # <1,2> and <2,1> in one step
    ('d42', _case((4, 2), (32, 20), N=421, c=0.5)),                         # loop form (default of the switch)
    ('d71', _case((7, 1), (12, 30), N=310)),                                # 15 moment columns, first factor
    ('d17', _case((1, 7), (24, 24), N=330, c=0.8)),                         # 15 moment columns, second factor
    ('d77', _case((7, 7), (32, 32), N=455, c=0.65)),                        # both at the edge
    ('L32', _case((3, 2), (14, 100), N=390, c=(0.8, 0.2))),                 # large <1,7>, !SPEC loop
    ('L51', _case((5, 1), (16, 112), (9, 50), N=305, c=0.8)),               # large, the latents differ
    ('L77', _case((7, 7), (10, 100), N=347, c=0.5)),                        # large at the edge
    ('p81', _case((8, 1), (20, 20), N=317, c=0.8)),                         # panels because of D
    ('p28', _case((2, 8), (10, 100), N=365, c=0.5)),                        # panels because of D, large grid
    ('p88', _case((8, 8), (17, 17), N=700)),                                # panels, one padded block
    ('p43', _case((4, 3), (40, 40), N=323, c=0.5)),                         # panels because of size
])
FUSED = [k for k in CASES if not k.startswith('p')]

# the device fit loops: small grids, cond(K_p) <= 1e3 (the conditioning at which the loop tolerances were measured)
FIT_N = 3000              # rows of a fit fixture (head_fit_ref.N_ROWS)
FIT_CASES = OrderedDict([
    ('d31', _case((3, 1), (6, 5), N=FIT_N, c=0.3)),
    ('d71', _case((7, 1), (6, 5), N=FIT_N, c=0.8)),
    ('L32', _case((3, 2), (10, 50), N=FIT_N, c=(0.5, 0.25))),
])
HEAD_FIT_CASES = ('d31', 'd71')
SHIFT_CASE = 'd21-mix'
SHIFT = 3.0               # the largest shift tried at which the oracle's own error is <= 1e-9: test_cpu_kron_nd.py::test_oracle_at_shifted_inputs


# The finish-stage edge grids (tests/test_gpu_kronf_stages.py): N = 33 rows; the smallest grid the entry points accept is ONE point per factor
# (validate_kron refuses M <= 0 only).  EDGE_C is the lengthscale constant c of these problems: tests/test_cpu_kronf_finish_ref.py shows on the
# CPU that every deliberate mistake of the finish stage is caught on each of them at this c.
EDGE_C = 0.5
EDGE_GRIDS = [(1, 1), (15, 17), (16, 16), (17, 31), (32, 32), (16, 112), (9, 50), (10, 100), (1, 112)]
EDGE_DS = [(1, 1), (7, 7)]


@functools.lru_cache(maxsize=None)
def edge_problem(grid, D, g=None):
    """(X, Y, p) of an edge grid at N = 33 (read-only); g: the g latent's grid when it differs"""
    X, Y, p = make_kron_problem_nd(33, grid[0], grid[1], D[0], D[1], 4000 + 131 * grid[0] + grid[1] + 7 * D[0], M0g=g and g[0], M1g=g and g[1], c=EDGE_C)
    _freeze(X, Y, p)
    return X, Y, p


def pptr_problem(grid):
    """(Xtrain, Ytrain, x minibatch, y minibatch, p) of the precipitation data at the reference's initialisation on `grid` x `grid` inducing
    points (the ill-conditioned init: cond(K_s) ~ 5e7 at 32 x 32) with a 1000-row minibatch as DataSet.next_batch hands it out"""
    import os
    from onofftf.model import init_params, engine_params
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pptr.npz'))
    Xtr, Ytr = d['Xtrain'].copy(), d['Ytrain']
    Xtr[:, 2] /= 1000.0                                   # scripts/create_cvsplits.py:17
    np.random.seed(7)
    p = engine_params(init_params(Xtr, grid, grid, kmeans_seed=3))
    idx = np.random.RandomState(11).permutation(Xtr.shape[0])[:1000]     # shuffled rows
    return Xtr, Ytr, np.ascontiguousarray(Xtr[idx]), np.ascontiguousarray(Ytr[idx]), p


def _seed(name):
    return 1000 + list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def problem(name, N=None, shift=0.0):
    """(X, Y, p) of a case of CASES (read-only: shared between tests); N overrides the case's row count (shard additivity)."""
    k = CASES[name]
    g = k['g'] or (None, None)
    X, Y, p = make_kron_problem_nd(N or k['N'], k['f'][0], k['f'][1], k['D'][0], k['D'][1], _seed(name), M0g=g[0], M1g=g[1], shift=shift, c=k['c'])
    _freeze(X, Y, p)
    return X, Y, p


# Grids beyond ONE 128-row block of the GEMM-panel path (operands are padded to 128: every grid above has Mq0 = Mq1 = 128 and one block per
# factor).  id -> as CASES; the comment is (block counts nb0, nb1) per latent and what the case is there for.  The c of each case is tuned on
# the CPU (test_cpu_kron_blocks.py) to the same fixture conditions.  A table of its own: _seed indexes into CASES.
BLOCK_CASES = OrderedDict([
    ('b21', _case((2, 1), (130, 12), N=301, c=0.4)),                        # 2, 1: Mq0 = 256 != Mq1 = 128
    ('b12', _case((1, 2), (9, 130), N=303, c=0.5)),                         # 1, 2: the transposed strides
    ('bmix', _case((2, 1), (130, 12), (12, 130), N=305, c=0.5)),            # f 2, 1 and g 1, 2 in one step
    ('b3', _case((1, 1), (257, 5), N=1031, c=0.5)),                         # 3, 1; Nc = 2048: nk = 128, dP0's split-K has S = 56 != nk
    ('bedge', _case((3, 1), (129, 9), (128, 9), N=307, c=0.4)),             # f 2, 1 (one real row in the second block) beside g 1, 1 (no padding)
    ('b22', _case((2, 1), (130, 129), N=309, c=0.35)),                       # 2, 2: four output tiles per split-K slice; literal form 16 770^2
])
# further grids of the stage tests (tests/test_gpu_kron_panel_stages.py), block_edge_problem(grid): one point in a factor beside two
# blocks, a full block beside one row past it, a ragged second block beside three points
BLOCK_EDGE_GRIDS = [(1, 130), (128, 129), (200, 3)]
BLOCK_EDGE_C = 0.35


@functools.lru_cache(maxsize=None)
def block_edge_problem(grid):
    """(X, Y, p) of a grid of BLOCK_EDGE_GRIDS at N = 33 rows and (D0, D1) = (1, 1) (read-only)"""
    X, Y, p = make_kron_problem_nd(33, grid[0], grid[1], 1, 1, 6000 + 131 * grid[0] + grid[1], c=BLOCK_EDGE_C)
    _freeze(X, Y, p)
    return X, Y, p


BLOCK_LITERAL = [k for k in BLOCK_CASES if k != 'b22']      # cases whose literal (dense) oracle is evaluated; b22: kronp_ref.factored_* only


BLOCK_MATERN = ('b21', ('matern32', 'rbf'), ('matern52', 'matern52'))      # case, kinds of f, kinds of g: the Matern run of the block cases


def block_matern_fixture():
    """(X, Y, p) of the BLOCK_MATERN case with its kinds in p (arrays shared with block_problem's cache)"""
    import kron_matern_ref as kmr
    X, Y, p = block_problem(BLOCK_MATERN[0])
    return X, Y, kmr.with_kinds(p, BLOCK_MATERN[1], BLOCK_MATERN[2])


@functools.lru_cache(maxsize=None)
def block_matern_oracle():
    """(predict rows at g_offset 0, (elbo, data, kl, grads)) of the Matern fixture from tests/kron_matern_ref.py (literal order)"""
    import kron_matern_ref as kmr
    X, Y, p = block_matern_fixture()
    return kmr.kron_build_predict(X, p, JITTER, 0.0), kmr.kron_elbo_and_grad(X, Y, p, JITTER, scale=block_scale(BLOCK_MATERN[0]))


@functools.lru_cache(maxsize=None)
def block_problem(name, N=None):
    """(X, Y, p) of a case of BLOCK_CASES (read-only); N overrides the case's row count"""
    k = BLOCK_CASES[name]
    g = k['g'] or (None, None)
    X, Y, p = make_kron_problem_nd(N or k['N'], k['f'][0], k['f'][1], k['D'][0], k['D'][1], 5000 + list(BLOCK_CASES).index(name), M0g=g[0], M1g=g[1],
                                   c=k['c'])
    _freeze(X, Y, p)
    return X, Y, p


def block_scale(name):
    return 105280.0 / BLOCK_CASES[name]['N']


def block_counts(name):
    """((nb0, nb1) of f, (nb0, nb1) of g): 128-row blocks per factor"""
    k = BLOCK_CASES[name]
    return tuple(tuple(-(-m // 128) for m in grid) for grid in (k['f'], k['g'] or k['f']))


@functools.lru_cache(maxsize=None)
def block_oracle_predict(name, g_offset):
    """the 9 prediction rows: the literal oracle, for b22 the factored restatement (pinned to the literal one in test_cpu_kron_blocks.py)"""
    X, Y, p = block_problem(name)
    if name in BLOCK_LITERAL:
        import zigp_oracle as o
        return tuple(np.asarray(r).reshape(-1) for r in o.kron_build_predict(X, p, JITTER, g_offset))
    import kronp_ref
    return tuple(kronp_ref.factored_predict(X, p, JITTER, g_offset))


@functools.lru_cache(maxsize=None)
def block_oracle_grad(name, include_kl=True, scale=None):
    """(elbo, data, kl, grads) at jitter 1e-5 and the case's scale (or `scale`), from the same reference as block_oracle_predict"""
    X, Y, p = block_problem(name)
    scale = block_scale(name) if scale is None else scale
    if name in BLOCK_LITERAL:
        import zigp_oracle_torch as ot
        return ot.kron_elbo_and_grad(X, Y, p, JITTER, scale=scale, include_kl=include_kl)
    import kronp_ref
    return kronp_ref.factored_elbo_and_grad(X, Y, p, JITTER, scale=scale, include_kl=include_kl)


@functools.lru_cache(maxsize=None)
def fit_problem(name):
    k = FIT_CASES[name]
    X, Y, p = make_kron_problem_nd(k['N'], k['f'][0], k['f'][1], k['D'][0], k['D'][1], 2000 + list(FIT_CASES).index(name), c=k['c'])
    _freeze(X, Y, p)
    return X, Y, p


READ_ONLY_NOTE = 'ignore:The given NumPy array is not writable'      # torch's note on wrapping a frozen array: the oracle only reads it


def _freeze(X, Y, p):
    for a in [X, Y] + [v for k in p if isinstance(p[k], list) for v in p[k]] + [v for v in p.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)


def head_params(p):
    return {k: p[k] for k in ('Zf', 'ell_f', 'var_f', 'u_fm', 'u_fs_sqrt', 'noise')}


@functools.lru_cache(maxsize=None)
def oracle_predict(name, g_offset, shift=0.0):
    import zigp_oracle as o
    X, Y, p = problem(name, shift=shift)
    return tuple(np.asarray(r).reshape(-1) for r in o.kron_build_predict(X, p, JITTER, g_offset))


def case_scale(name):
    return 105280.0 / CASES[name]['N']


@functools.lru_cache(maxsize=None)
def oracle_grad(name, shift=0.0):
    """(elbo, data, kl, grads) of zigp_oracle_torch.kron_elbo_and_grad at jitter 1e-5 and the case's scale"""
    import zigp_oracle_torch as ot
    X, Y, p = problem(name, shift=shift)
    return ot.kron_elbo_and_grad(X, Y, p, JITTER, scale=case_scale(name))


def _factored_with_oracle_inverse(X, p, tag, jit):
    """The FACTORED identities the engine evaluates, on the CPU with the oracle's own np.linalg.inv (LAPACK LU, as
    tf.matrix_inverse scripts/onoff.py:192): its distance from the literal dense order is the floor that the op order alone
    sets (tests/test_cpu_oracle.py::test_factored_kronecker_algebra_differs_...; tools/lu_vs_chol_experiment.py)."""
    import zigp_oracle as o
    Z, ell, var = p['Z' + tag], p['ell_' + tag], [float(np.squeeze(v)) for v in p['var_' + tag]]
    P = [np.linalg.inv(o.rbf_K(Z[q], None, ell[q], var[q]) + jit * np.eye(Z[q].shape[0])) for q in range(2)]
    d0 = Z[0].shape[1]
    k0, k1 = o.rbf_K(Z[0], X[:, :d0], ell[0], var[0]), o.rbf_K(Z[1], X[:, d0:], ell[1], var[1])
    M0, M1 = Z[0].shape[0], Z[1].shape[0]
    U, S2 = p['u_%sm' % tag].reshape(M0, M1), np.square(p['u_%ss_sqrt' % tag]).reshape(M0, M1)
    a0, a1 = P[0] @ k0, P[1] @ k1
    mu = np.einsum('in,ij,jn->n', k0, P[0] @ U @ P[1], k1)
    vv = var[0] * var[1] - (k0 * a0).sum(0) * (k1 * a1).sum(0) + np.einsum('in,ij,jn->n', a0 ** 2, S2, a1 ** 2)
    return mu, vv


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def fixture_floor_and_cond(X, p, ref=None, jit=JITTER):
    """(op-order floor, max cond(K_p + jitter)) of a fixture: the floor is the distance of the factored algebra, evaluated with
    np.linalg.inv, from the literal dense oracle on the predictive means and variances of both latents."""
    import zigp_oracle as o
    ref = ref if ref is not None else o.kron_build_predict(X, p, jit, 0.0)
    floor, cond = 0.0, 0.0
    for tag, (im, iv) in (('f', (3, 4)), ('g', (5, 6))):
        mu, vv = _factored_with_oracle_inverse(X, p, tag, jit)
        floor = max(floor, _relerr(mu, ref[im]), _relerr(vv, ref[iv]))
        for q in range(2):
            Z = p['Z' + tag][q]
            K = o.rbf_K(Z, None, p['ell_' + tag][q], float(np.squeeze(p['var_' + tag][q]))) + jit * np.eye(Z.shape[0])
            cond = max(cond, float(np.linalg.cond(K)))
    return floor, cond


def fixture_cond(p, jit=JITTER):
    """max cond(K_p + jitter) over the four factors alone (a grid whose literal form is too large for the floor)"""
    import zigp_oracle as o
    return max(float(np.linalg.cond(o.rbf_K(p['Z' + tag][q], None, p['ell_' + tag][q], float(np.squeeze(p['var_' + tag][q])))
                                    + jit * np.eye(p['Z' + tag][q].shape[0]))) for tag in 'fg' for q in range(2))


def rbf_K_difference_form(X, X2, lengthscales, variance):
    """variance exp(-sum_d ((x_d - z_d) / l_d)^2 / 2) from the DIFFERENCES: no cancellation however far the inputs lie from 0 (the
    oracle's rbf_K expands the square, onofftf/main.py:41-51)"""
    X2 = X if X2 is None else X2
    d = (np.asarray(X)[:, None, :] - np.asarray(X2)[None, :, :]) / np.asarray(lengthscales).reshape(1, 1, -1)
    return variance * np.exp(-np.sum(np.square(d), 2) / 2)
