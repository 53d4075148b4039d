"""The blocked Cholesky and its inverse (potrf_trtri_jobs, csrc/zigp_host.h; k_potrf_diag, csrc/zigp_kernels.h) restated on the CPU, launch by
launch -- TEST INFRASTRUCTURE ONLY.

THE CHAIN, for a matrix padded with the identity to Mp = nb 128.  Per block column j: the one-workgroup kernel factors the diagonal block
(L_jj, and W_jj = L_jj^-1 by three levels: 16 x 16 inverses, the coupling block of each 32-panel, the blocks at panel distance 1, 2, 3);
the panel product L[bi][j] = A[bi][j] W_jj^T for bi > j (a multiplication by the inverse, not a triangular solve); the trailing update
A[bi][bj] -= L[bi][j] L[bj][j]^T for j < bj <= bi.  Then W by recursive doubling over groups of b = 1, 2, 4 .. diagonal blocks:
tri1  T = L21 W11 and tri2  W21 = -W22 T.  With split-K every block product is cut into S = max(1, min(8, minlen, 512 // tiles)) slices of
its k range (k-steps of 16 columns, slice s = [len s // S, len (s + 1) // S)) whose partial tiles are added in slice order.

A RUN is what DenseEngine.test_potrf_stages returns, or emulate() below: dict(L, W, T, Mp, nb, info, launches=[dict(kind, idx, tiles, S,
npan, snap)]).  restate(run, A) evaluates every launch from the images the launch read -- the snapshot behind one launch is the "before"
image of the next -- and returns name -> (value, S, mask) with name = 'panel:j', 'trail:j', 'tri1:b', 'tri2:b': value the whole [Mp][Mp]
image the launch leaves (what it does not write: the image before), S the sum of absolute terms per element (|before| included where the
launch accumulates; 0 where it does not write, so that an element written out of place breaks its bar), mask the elements it writes.
tap_of(run, name) is the image the run holds for that entry.  dtype=np.longdouble gives the truth (2^-64 against bars of 16 * 2^-53),
np.float64 the NumPy evaluation whose error the bar of a product launch is measured in:

    RULE 1 (sums of products on given operands: panel, trail, tri1, tri2 and the ordered plane sum inside them; the coupling and distance
    blocks of the diagonal kernel):     err_gpu <= 4 err_np + 16 EPS S.

THE DIAGONAL KERNEL has no tap inside it; diag_checks() holds its outputs level by level against sub-blocks of its own final L^, W^ (no
sub-block is overwritten by a later level), EPS = 2^-53 the unit roundoff:

    factor      |A_jj - L^ L^T|_ik <= (min(i, k) + 1 + C) EPS (|L^| |L^|^T)_ik              (Higham, Accuracy and Stability, Thm 10.3, per element)
    16 x 16     |W^ L^ - I|        <= (16 + C) EPS |W^| |L^|                                (the side the recurrence w_rj = -w_jj sum w_rk l_kj solves)
    coupling    W^21  against  -W^22 (L^21 W^11)                                            (rule 1)
    distance    W^_ij against  -W^_ii sum_{x = j .. i-1} L^_ix W^_xj                        (rule 1)

C = 3, DERIVED FROM THE KERNEL'S ARITHMETIC, not from its results.  The textbook count min(i, k) + 1 is: one rounding per product and per
subtraction of the min(i, k) earlier columns, plus ONE for the division by l_kk (an exactly rounded square root adds nothing at first
order to l_kk^2).  The kernel forms fewer roundings in the sums (fma chains; MFMA accumulators subtracted once per 32-column panel) but
replaces the division and the square root:
  * potrf_rsqrt: the hardware estimate + two Newton steps y <- fma(y / 2, e, y), e = fma(-d y, y, 1).  After the first step the
    quadratic term is below 2^-52; in the second, e carries the rounding of d y (absolute EPS, halved by the step: 0.5 EPS) and the final
    fma rounds once (1 EPS):  rd = d^-1/2 (1 + dr), |dr| <= 1.5 EPS.
  * the `sq` correction: sq0 = fl(d rd), sq = fma(rd / 2, fma(-sq0, sq0, d), sq0) is one Newton step of the square root from an iterate that
    is already within 2.5 EPS: its quadratic term vanishes, the final fma rounds once:  l_kk = sqrt(d) (1 + ds), |ds| <= 1 EPS.
  * the reciprocal multiply (potrf_factor_cols, and x = a rd in potrf_solve_rows): l_ik = fl(s rd) = s rd (1 + dm), so
    l_ik l_kk = s (1 + dm)(1 + dr)(1 + ds): 1 + 1.5 + 1 = 3.5 EPS where the division gives 1 EPS.
  Hence C = ceil(3.5 - 1) = 3 (the diagonal element: l_kk^2 = d (1 + ds)^2, 2 EPS, is inside it).  In the 16 x 16 inverse w_jj = rd_j, so
  w_jj l_jj - 1 = (1 + dr)(1 + ds) - 1 <= 2.5 EPS, and w_rj l_jj carries the same factor on top of the at most 15 fma roundings and the
  final multiply of its sum: <= (16 + C) EPS.

EXACT FAMILY.  N[i][j] = h(i, j) in {-3 .. 3} where i > j and i % 3 == j % 3 + 1, else 0 (h: the project's aperiodic integer hash, _pat of
tests/test_gpu_stages.py), so N maps residue class 0 -> 1 -> 2 and N^3 = 0;  d_j in {1/2, 1, 2} without period;  L0 = (I + N) diag(d),
W0 = diag(d)^-1 (I - N + N^2), A = L0 L0^T.  Everything is a small dyadic number, every pivot is 1/4, 1 or 4, every partial sum of every
product is exact in any order: the chain must return L0 and W0 bit for bit whatever the slice count or tile order.
"""
import numpy as np

EPS = 2.0 ** -53          # unit roundoff of float64
C_DIAG = 3                # see the derivation above
LD = np.longdouble
SENTINEL = float(np.frombuffer(bytes([0x7f]) * 8, dtype=np.float64)[0])
BM, PNB, PHB, KB = 128, 32, 16, 8     # block, panel and half-panel sizes; k-steps of 16 columns per block
KINDS = ('diag', 'panel', 'trail', 'tri1', 'tri2')
MUTATIONS = ('dropslice',   # a split-K slice left out of the plane sum
             'dupslice',    # a slice added twice
             'kshort',      # the last slice one k-step short
             'noT',         # the panel product with W_jj instead of W_jj^T
             'nosign',      # tri2 without its sign
             'Woff',        # one element of a W snapshot off by 1e-11 relative
             'nocouple',    # the coupling block of a 32-panel left zero
             'upper')       # a tile above the diagonal written by the trailing update


# ----------------------------------------------------------------------------------------------------------------------------------
# families
# ----------------------------------------------------------------------------------------------------------------------------------
def _hash(i, j, shift):
    """the 32-bit integer hash of tests/test_gpu_stages.py::_pat (no symmetry, no period)"""
    i, j = np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(0x9E3779B1) + j * np.uint64(0x85EBCA77) + np.uint64((shift + 1) * 0xC2B2AE3D)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return h


def exact_family(n, seed=0):
    """(A, L0, W0) of the exact family; seed: a second pattern, so that a term that happens to be zero in one is not in the other"""
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    N = np.where((i > j) & (i % 3 == j % 3 + 1), (_hash(i, j, seed) % np.uint64(7)).astype(np.float64) - 3.0, 0.0)
    d = 2.0 ** ((_hash(np.arange(n), 0 * np.arange(n) + 12345, seed + 17) % np.uint64(3)).astype(np.float64) - 1.0)
    L0 = (np.eye(n) + N) * d[None, :]
    W0 = (np.eye(n) - N + N @ N) / d[:, None]
    return L0 @ L0.T, L0, W0


def exact_with_pivot(n, p, value, seed=0):
    """the exact family with pivot p (1-based) made exactly `value`: every earlier column is untouched and still exact"""
    A, L0, _ = exact_family(n, seed)
    A = A.copy()
    A[p - 1, p - 1] += value - L0[p - 1, p - 1] ** 2
    return A


def rbf_family(n, ell, seed=0, D=2, jitter=1e-6):
    """(a) Kuu of n random inducing inputs in the unit square: exp(-|z - z'|^2 / 2 ell^2) + jitter I"""
    Z = np.random.default_rng(1000 + seed).random((n, D))
    r2 = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * r2 / ell ** 2) + jitter * np.eye(n)


ELL_MID, ELL_HIGH = 0.03, 0.25       # (a) cond ~ 1e4 (n = 200 .. 520) and 1e7 .. 1e9 (n = 200 .. 1024), pinned in tests/test_cpu_potrf_ref.py
COND_MID, COND_HIGH, COND_B = (1e3, 1e5), (1e7, 1e9), (1e2, 1e4)


def bbt_family(n, seed=0):
    """(b) B B^T + I, B standard normal: dense signs, cond ~ 4 n"""
    B = np.random.default_rng(2000 + seed).standard_normal((n, n))
    return B @ B.T + np.eye(n)


def graded_scale(n, seed=0):
    """D = 2^-14 .. 2^14 (covers 10^-4 .. 10^4), graded and shuffled; powers of two, so that D A D is an exact scaling"""
    e = np.round(np.linspace(-14, 14, n))
    return 2.0 ** np.random.default_rng(3000 + seed).permutation(e)


def family(name, n, seed=0):
    if name == 'a_mid':
        return rbf_family(n, ELL_MID, seed)
    if name == 'a_high':
        return rbf_family(n, ELL_HIGH, seed)
    if name == 'b':
        return bbt_family(n, seed)
    if name == 'c':
        D = graded_scale(n, seed)
        return rbf_family(n, ELL_HIGH, seed) * D[:, None] * D[None, :]
    raise KeyError(name)


FAMILIES = ('a_mid', 'a_high', 'b', 'c')


# ----------------------------------------------------------------------------------------------------------------------------------
# the plan: launches and slice counts
# ----------------------------------------------------------------------------------------------------------------------------------
def slice_count(tiles, minlen=KB):
    """run_gemm_sk_tiles' rule"""
    return max(1, min(8, minlen, 512 // tiles))


def _groups(nb, b):
    """(lo, mid, hi) of every doubling group at distance b that has a lower half"""
    return [(lo, lo + b, min(lo + 2 * b, nb)) for lo in range(0, nb, 2 * b) if lo + b < nb]


def tiles_of(kind, idx, nb):
    """[(bi, bj, k0, k1)]: output tiles of a launch with the block columns [k0, k1) of its k range"""
    if kind == 'panel':
        return [(bi, idx, idx, idx + 1) for bi in range(idx + 1, nb)]
    if kind == 'trail':
        return [(bi, bj, idx, idx + 1) for bi in range(idx + 1, nb) for bj in range(idx + 1, bi + 1)]
    if kind == 'tri1':
        return [(bi, bj, bj, mid) for lo, mid, hi in _groups(nb, idx) for bi in range(mid, hi) for bj in range(lo, mid)]
    if kind == 'tri2':
        return [(bi, bj, mid, bi + 1) for lo, mid, hi in _groups(nb, idx) for bi in range(mid, hi) for bj in range(lo, mid)]
    raise KeyError(kind)


def plan(n, split_k):
    """the launches of one job of size n in launch order: [dict(kind, idx, tiles, S, npan)] (S = 0: one workgroup per tile)"""
    Mp = -(-n // BM) * BM
    nb = Mp // BM
    out = []
    for j in range(nb):
        nreal = max(0, min(BM, n - j * BM))
        out.append(dict(kind='diag', idx=j, tiles=1, S=0, npan=-(-nreal // PNB)))
        if j + 1 < nb:
            for kind in ('panel', 'trail'):
                t = tiles_of(kind, j, nb)
                out.append(dict(kind=kind, idx=j, tiles=len(t), S=slice_count(len(t)) if split_k else 0, npan=0))
    b = 1
    while b < nb:
        for kind in ('tri1', 'tri2'):
            t = tiles_of(kind, b, nb)
            out.append(dict(kind=kind, idx=b, tiles=len(t), S=slice_count(len(t), min(k1 - k0 for _, _, k0, k1 in t) * KB) if split_k else 0, npan=0))
        b *= 2
    return out


def facts_of(run):
    return [{k: l[k] for k in ('kind', 'idx', 'tiles', 'S', 'npan')} for l in run['launches']]


# ----------------------------------------------------------------------------------------------------------------------------------
# one launch
# ----------------------------------------------------------------------------------------------------------------------------------
def _blk(X, bi, bj0, bj1=None):
    return X[bi * BM:(bi + 1) * BM, bj0 * BM:(bj0 + 1 if bj1 is None else bj1) * BM]


def _prod(A, B, S, _mut, with_S):
    """A [m][K] B [K][n] as S ordered k slices (S <= 1 and no mistake: one product); returns (value, sum of absolute terms)"""
    ks = A.shape[1] // 16
    if S <= 1 and not (set(_mut) & {'dropslice', 'dupslice', 'kshort'}):
        v = A @ B
    else:
        S = max(1, S)
        v = np.zeros((A.shape[0], B.shape[1]), dtype=A.dtype)
        for s in range(S):
            k0, k1 = ks * s // S, ks * (s + 1) // S
            if s == S - 1 and 'dropslice' in _mut:
                continue
            if s == S - 1 and 'kshort' in _mut:
                k1 -= 1
            part = A[:, 16 * k0:16 * k1] @ B[16 * k0:16 * k1]
            v = v + part
            if s == 0 and 'dupslice' in _mut:
                v = v + part
    return v, (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64) if with_S else None)


def apply_launch(l, Li, Wi, Ti, nb, dtype=np.float64, _mut=(), with_S=True):
    """A product launch l on the images it reads -> (which image it writes, value, S, mask).  value: the whole image in dtype."""
    kind, j = l['kind'], l['idx']
    Lx, Wx, Tx = (np.asarray(X, dtype=dtype) for X in (Li, Wi, Ti))
    which = {'panel': 'L', 'trail': 'L', 'tri1': 'T', 'tri2': 'W'}[kind]
    out = {'L': Lx, 'T': Tx, 'W': Wx}[which].copy()
    Sm = np.zeros(out.shape)
    mask = np.zeros(out.shape, dtype=bool)
    tiles = list(tiles_of(kind, j, nb))
    if kind == 'trail' and 'upper' in _mut and j + 2 < nb:
        tiles.append((j + 1, j + 2, j, j + 1))
    for bi, bj, k0, k1 in tiles:
        if kind == 'panel':
            Wjj = _blk(Wx, j, j)
            v, S = _prod(_blk(Lx, bi, j), Wjj if 'noT' in _mut else Wjj.T, l['S'], _mut, with_S)
        elif kind == 'trail':
            v, S = _prod(_blk(Lx, bi, j), _blk(Lx, bj, j).T, l['S'], _mut, with_S)
            before = _blk(Lx, bi, bj)
            v = before - v
            if with_S:
                S = S + np.abs(before).astype(np.float64)
        elif kind == 'tri1':
            v, S = _prod(_blk(Lx, bi, k0, k1), Wx[k0 * BM:k1 * BM, bj * BM:(bj + 1) * BM], l['S'], _mut, with_S)
        else:
            v, S = _prod(_blk(Wx, bi, k0, k1), Tx[k0 * BM:k1 * BM, bj * BM:(bj + 1) * BM], l['S'], _mut, with_S)
            if 'nosign' not in _mut:
                v = -v
        out[bi * BM:(bi + 1) * BM, bj * BM:(bj + 1) * BM] = v
        mask[bi * BM:(bi + 1) * BM, bj * BM:(bj + 1) * BM] = True
        if with_S:
            Sm[bi * BM:(bi + 1) * BM, bj * BM:(bj + 1) * BM] = S
    return which, out, (Sm if with_S else None), mask


# ----------------------------------------------------------------------------------------------------------------------------------
# the diagonal kernel: emulation and level checks
# ----------------------------------------------------------------------------------------------------------------------------------
def _inv16(L, dinv, dtype):
    """potrf_invert16: columns right to left, w_rj = -w_jj sum_{k = j+1 .. r} w_rk l_kj, w_jj = the reciprocal the factor kept"""
    n = L.shape[0]
    W = np.zeros((n, n), dtype=dtype)
    for j in range(n - 1, -1, -1):
        W[j, j] = dinv[j]
        for r in range(j + 1, n):
            W[r, j] = -dinv[j] * (W[r, j + 1:r + 1] @ L[j + 1:r + 1, j])
    return W


def diag_block(A, npan, dtype=np.float64, _mut=()):
    """k_potrf_diag on one 128 x 128 block in `dtype`: (L, W, bad).  The lower triangle of A is read; rows / columns >= 32 npan pass through
    (identity padding).  bad: 0 or the 1-based column of the first pivot that is not > 0 (what the kernel reports; it then writes nothing)."""
    S = np.tril(np.asarray(A, dtype=dtype)).copy()
    nreal = npan * PNB
    dinv = np.ones(BM, dtype=dtype)
    half = dtype(0.5)
    for jb in range(0, nreal, PNB):
        for j in range(jb, jb + PNB):
            d = S[j, j]
            if not d > 0:
                return None, None, j + 1
            rd = dtype(1) / np.sqrt(d)
            sq = d * rd
            sq = sq + half * rd * (d - sq * sq)
            dinv[j] = rd
            S[j, j] = sq
            S[j + 1:nreal, j] = S[j + 1:nreal, j] * rd
            hi = jb + PNB
            S[j + 1:nreal, j + 1:hi] -= np.outer(S[j + 1:nreal, j], S[j + 1:hi, j])
        if jb + PNB < nreal:
            P = S[jb + PNB:nreal, jb:jb + PNB]
            S[jb + PNB:nreal, jb + PNB:nreal] -= P @ P.T
    L = np.tril(S)
    W = np.eye(BM, dtype=dtype)
    for p0 in range(0, nreal, PHB):
        W[p0:p0 + PHB, p0:p0 + PHB] = _inv16(L[p0:p0 + PHB, p0:p0 + PHB], dinv[p0:p0 + PHB], dtype)
    for pb in range(0, nreal, PNB):
        a, b, c = slice(pb, pb + PHB), slice(pb + PHB, pb + PNB), None
        if 'nocouple' not in _mut or pb != PNB * ((npan - 1) // 2):
            W[b, a] = -(W[b, b] @ (L[b, a] @ W[a, a]))
    for dist in range(1, npan):
        for bq in range(npan - dist):
            jb, ib = bq * PNB, (bq + dist) * PNB
            T = L[ib:ib + PNB, jb:ib] @ W[jb:ib, jb:jb + PNB]
            W[ib:ib + PNB, jb:jb + PNB] = -(np.tril(W[ib:ib + PNB, ib:ib + PNB]) @ T)
    return L, np.tril(W), 0


def _rule1(got, expr, S):
    """(err, bar) of rule 1: expr(dtype) evaluates the launch's expression in that dtype"""
    truth = expr(LD)
    err_np = np.abs(np.asarray(expr(np.float64), dtype=LD) - truth)
    return np.abs(np.asarray(got, dtype=LD) - truth), 4 * err_np + 16 * EPS * np.asarray(S, dtype=LD)


def ratio(err, bar):
    """largest err / bar (0 / 0 = 0; an error where the bar is 0: inf)"""
    err, bar = np.asarray(err, dtype=LD), np.asarray(bar, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.inf))
    return float(np.max(r))


def diag_checks(Ain, Lh, Wh, npan):
    """The level checks of one diagonal launch: Ain the block the kernel read (lower triangle), Lh / Wh the blocks it wrote.
    Returns {level: err / bar}, levels 'factor', 'inv16', 'couple', 'dist', 'pad' ('pad': 0 or inf -- rows beyond the factored panels must
    pass through bit for bit, and both outputs must be exact zero above the diagonal)."""
    nreal = npan * PNB
    Ain, Lh, Wh = (np.asarray(X, dtype=np.float64) for X in (Ain, Lh, Wh))
    out = {}
    I = np.eye(BM)
    pad_ok = (np.array_equal(np.triu(Lh, 1), np.zeros((BM, BM))) and np.array_equal(np.triu(Wh, 1), np.zeros((BM, BM)))
              and np.array_equal(Lh[nreal:], np.tril(Ain)[nreal:]) and np.array_equal(Wh[nreal:], I[nreal:])
              and not np.any(np.signbit(np.triu(Lh, 1))) and not np.any(np.signbit(np.triu(Wh, 1))))
    out['pad'] = 0.0 if pad_ok else np.inf
    r = nreal
    Ll, Wl = Lh[:r, :r].astype(LD), Wh[:r, :r].astype(LD)
    low = np.tril(np.ones((r, r), dtype=bool))
    res = np.abs(np.tril(Ain[:r, :r]).astype(LD) - np.tril(Ll @ Ll.T))
    cnt = np.minimum(np.arange(r)[:, None], np.arange(r)[None, :]) + 1 + C_DIAG
    out['factor'] = ratio(res[low], (cnt * EPS * (np.abs(Lh[:r, :r]) @ np.abs(Lh[:r, :r]).T))[low])
    worst = {'inv16': 0.0, 'couple': 0.0, 'dist': 0.0}
    for p0 in range(0, r, PHB):
        s = slice(p0, p0 + PHB)
        res = np.abs(Wl[s, s] @ Ll[s, s] - I[:PHB, :PHB])
        worst['inv16'] = max(worst['inv16'], ratio(res, (PHB + C_DIAG) * EPS * (np.abs(Wh[s, s]) @ np.abs(Lh[s, s]))))
    for pb in range(0, r, PNB):
        a, b = slice(pb, pb + PHB), slice(pb + PHB, pb + PNB)
        expr = lambda dt: -(Wh[b, b].astype(dt) @ (Lh[b, a].astype(dt) @ Wh[a, a].astype(dt)))
        worst['couple'] = max(worst['couple'], ratio(*_rule1(Wh[b, a], expr, np.abs(Wh[b, b]) @ (np.abs(Lh[b, a]) @ np.abs(Wh[a, a])))))
    for ip in range(npan):
        for jp in range(ip):
            i_, j_, x_ = slice(ip * PNB, (ip + 1) * PNB), slice(jp * PNB, (jp + 1) * PNB), slice(jp * PNB, ip * PNB)
            expr = lambda dt: -(Wh[i_, i_].astype(dt) @ (Lh[i_, x_].astype(dt) @ Wh[x_, j_].astype(dt)))
            worst['dist'] = max(worst['dist'], ratio(*_rule1(Wh[i_, j_], expr, np.abs(Wh[i_, i_]) @ (np.abs(Lh[i_, x_]) @ np.abs(Wh[x_, j_])))))
    out.update(worst)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# runs: emulation, restatement, checks
# ----------------------------------------------------------------------------------------------------------------------------------
def padded(A):
    """what the hook uploads: A with the identity behind it, [Mp][Mp]"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    Mp = -(-n // BM) * BM
    P = np.eye(Mp)
    P[:n, :n] = A
    return P


def emulate(A, split_k=True, dtype=np.float64, _mut=()):
    """The chain in NumPy `dtype`, in the shape of a run (snapshots included; images are stored as float64): every launch's output is the
    value of its restatement on the images before it, the diagonal launches are diag_block()."""
    n = np.asarray(A).shape[0]
    Li = padded(A).astype(dtype)
    Mp = Li.shape[0]
    nb = Mp // BM
    Wi, Ti = np.zeros((Mp, Mp), dtype=dtype), np.full((Mp, Mp), SENTINEL, dtype=dtype)
    run = dict(Mp=Mp, nb=nb, info=0, launches=[])
    f64 = lambda X: np.array(X, dtype=np.float64)
    for l in plan(n, split_k):
        l = dict(l)
        if l['kind'] == 'diag':
            j = l['idx']
            s = slice(j * BM, (j + 1) * BM)
            Lj, Wj, bad = diag_block(Li[s, s], l['npan'], dtype, _mut)
            if bad and not run['info']:
                run['info'] = j * BM + bad
            if not bad:
                Li[s, s], Wi[s, s] = Lj, Wj
            l['snap'] = (f64(Li), f64(Wi))
        else:
            which, v, _, _ = apply_launch(l, Li, Wi, Ti, nb, dtype, _mut, with_S=False)
            if which == 'L':
                Li = v
            elif which == 'W':
                Wi = v
            else:
                Ti = v
            l['snap'] = (f64(v),)
        run['launches'].append(l)
    for bi in range(nb - 1):
        Li[bi * BM:(bi + 1) * BM, (bi + 1) * BM:] = 0
    run.update(L=f64(Li), W=f64(Wi), T=f64(Ti))
    return run


def states(run, A):
    """[(L, W, T) images before launch k], k = 0 .. len(launches) (the last entry: after the last launch)"""
    Mp = run['Mp']
    cur = dict(L=padded(A), W=np.zeros((Mp, Mp)), T=np.full((Mp, Mp), SENTINEL))
    out = [(cur['L'], cur['W'], cur['T'])]
    for l in run['launches']:
        if l['kind'] == 'diag':
            cur['L'], cur['W'] = l['snap']
        else:
            cur[{'panel': 'L', 'trail': 'L', 'tri1': 'T', 'tri2': 'W'}[l['kind']]] = l['snap'][0]
        out.append((cur['L'], cur['W'], cur['T']))
    return out


def name_of(l):
    return '%s:%d' % (l['kind'], l['idx'])


def restate(run, A, dtype=np.float64, _mut=(), with_S=True, only=None):
    """name -> (value, S, mask) of every product launch of the run (only: a set of names), each from the images the launch read"""
    st = states(run, A)
    out = {}
    for k, l in enumerate(run['launches']):
        if l['kind'] == 'diag' or (only is not None and name_of(l) not in only):
            continue
        _, v, S, mask = apply_launch(l, *st[k], run['nb'], dtype, _mut, with_S)
        out[name_of(l)] = (v, S, mask)
    return out


def tap_of(run, name):
    """the image the run holds for a restate() entry"""
    for l in run['launches']:
        if name_of(l) == name:
            return l['snap'][-1]
    raise KeyError(name)


def check_products(run, A, _mut=(), only=None):
    """{name: err / bar} of rule 1 for every product launch: the run's image against the long-double restatement, err_np from the float64 one.
    An element outside the launch's tiles has S = 0 and err_np = 0: it must equal the image before, bit for bit."""
    tru = restate(run, A, LD, _mut, with_S=False, only=only)
    f64 = restate(run, A, np.float64, _mut, with_S=True, only=only)
    out = {}
    for name, (v, S, mask) in f64.items():
        t = tru[name][0]
        got = np.asarray(tap_of(run, name), dtype=LD)
        if not np.array_equal(np.asarray(tap_of(run, name))[~mask], np.asarray(v)[~mask]):
            out[name] = np.inf      # (also keeps the sentinel of T out of the arithmetic below)
            continue
        err = np.abs(got[mask] - t[mask])
        err_np = np.abs(np.asarray(v, dtype=LD)[mask] - t[mask])
        out[name] = ratio(err, 4 * err_np + 16 * EPS * np.asarray(S, dtype=LD)[mask])
    return out


def check_diags(run, A, only=None):
    """{'diag:j': {level: err / bar}}: every diagonal launch against the block it read; everything outside its block must be untouched"""
    st = states(run, A)
    out = {}
    for k, l in enumerate(run['launches']):
        if l['kind'] != 'diag' or (only is not None and l['idx'] not in only):
            continue
        j = l['idx']
        s = slice(j * BM, (j + 1) * BM)
        Lb, Wb, _ = st[k]
        La, Wa = l['snap']
        r = diag_checks(Lb[s, s], La[s, s], Wa[s, s], l['npan'])
        keep = np.ones(Lb.shape, dtype=bool)
        keep[s, s] = False
        if not (np.array_equal(La[keep], Lb[keep]) and np.array_equal(Wa[keep], Wb[keep])):
            r['pad'] = np.inf
        out[name_of(l)] = r
    return out


def check_final(run):
    """the images the chain returns: identity padding is part of the level checks; here the strict upper triangles (exact +0) and that L, W, T
    are what the last launches left (L: with its strictly-upper blocks cleared)"""
    Mp, nb = run['Mp'], run['nb']
    ok = True
    for X in (run['L'], run['W']):
        up = np.triu(X, 1)
        ok &= np.array_equal(up, np.zeros((Mp, Mp))) and not np.any(np.signbit(up))
    last = {}
    for l in run['launches']:
        if l['kind'] == 'diag':
            last['L'], last['W'] = l['snap']
        else:
            last[{'panel': 'L', 'trail': 'L', 'tri1': 'T', 'tri2': 'W'}[l['kind']]] = l['snap'][0]
    if 'L' in last:
        Lz = last['L'].copy()
        for bi in range(nb - 1):
            Lz[bi * BM:(bi + 1) * BM, (bi + 1) * BM:] = 0
        ok &= np.array_equal(Lz, run['L']) and np.array_equal(last['W'], run['W'])
        ok &= np.array_equal(last.get('T', np.full((Mp, Mp), SENTINEL)), run['T'])
    return bool(ok)


def mutate_run(run, mut):
    """a copy of the run with one mistake put into its images (the mistakes that are not a wrong restatement): 'Woff', 'upper'"""
    out = dict(run, launches=[dict(l, snap=tuple(s.copy() for s in l['snap'])) for l in run['launches']])
    if mut == 'Woff':
        l = [l for l in out['launches'] if l['kind'] == 'tri2'][-1]
        W = l['snap'][0]
        i, j = np.unravel_index(np.argmax(np.abs(np.tril(W, -BM))), W.shape)
        W[i, j] *= 1 + 1e-11
    elif mut == 'upper':
        l = [l for l in out['launches'] if l['kind'] == 'trail'][0]
        j = l['idx']
        l['snap'][0][(j + 1) * BM:(j + 2) * BM, (j + 2) * BM:(j + 3) * BM] += 1.0
    else:
        raise KeyError(mut)
    return out


def worst(*dicts):
    """largest ratio per launch kind / level over check_products and check_diags results"""
    out = {}
    for d in dicts:
        for name, r in d.items():
            if isinstance(r, dict):
                for lvl, x in r.items():
                    out['diag.' + lvl] = max(out.get('diag.' + lvl, 0.0), x)
            else:
                k = name.split(':')[0]
                out[k] = max(out.get(k, 0.0), r)
    return out
