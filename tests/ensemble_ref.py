"""Reference for the sample-path scores (include/zigp_ensemble.h; csrc/zigp_ensemble.hip).

* `scores_np`   a NumPy restatement of the kernels IN THEIR DOCUMENTED ORDER: rows of a group in chunks of CHUNK = 64 from the group's
                start, four interleaved row classes per chunk added as ((q0 + q1) + q2) + q3, chunks ascending from +0, the correctly
                rounded square root, c_t = sum_{s<t} D(s, t) with s ascending, the sum over t ascending, two divisions and one
                subtraction; the variogram by 64 x 64 tiles, a thread's 4 x 4 pairs k outer and l inner, the xor tree of a wave, the four
                waves in order, tiles ascending.  The kernels contract `a d * d + acc` and `w x + t` into one fma where NumPy rounds the
                product first: on operands whose products are exact (the exact tier's small integers) the two agree bit for bit.
                With dtype=np.longdouble the same code is the truth for the larger fixtures (the order is then immaterial).
* `scores_mp`   the definition from the same float64 inputs with every operation at 50 digits (mpmath): the truth for the small fixtures.
* weights       per output a first-order error weight S_w, built with the computation in the convention of tests/kronf_ref.py: the sum
                of the magnitudes after every rounding, each operand that is itself computed entering with its own weight -- carried
                through the square root (w(D) = w(D^2) / (2 D) + D) and the final differences.  One rounding moves a value by at most
                eps / 2 of its magnitude, so an evaluation in this order is within eps S_w / 2 of the exact value to first order.
"""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
CHUNK = 64          # ZIGP_ENS_CHUNK
TILE = 64           # rows of a variogram tile
FLOOR = 8.0         # score_ref.FLOOR: the bar for NumPy alone, in eps S_w
SIZES = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


def _pw(d, p):
    """|d|^p for p in (0.5, 1, 2) without pow"""
    if p == 0.5:
        return np.sqrt(np.abs(d))
    return np.abs(d) if p == 1 else d * d


def _seq(terms, wts, dtype):
    """sum of the rows of `terms` in ascending order from +0 with the weight: the terms' own weights plus every partial sum's magnitude"""
    acc = np.zeros(terms.shape[1:], dtype=dtype)
    w = np.zeros(terms.shape[1:], dtype=dtype)
    for t, e in zip(terms, wts):
        acc = acc + t
        w = w + e + np.abs(acc)
    return acc, w


def _score_of(c, wc, S, den, dtype):
    """c_S / S - (sum_{t=1}^{S-1} c_t) / den from the column sums c[t] (t = 0 .. S) and their weights"""
    s2, w2 = _seq(c[1:S], wc[1:S], dtype) if S > 1 else (dtype(0), dtype(0))
    a, b = c[S] / dtype(S), s2 / dtype(den)
    v = a - b
    return v, wc[S] / S + abs(a) + w2 / den + abs(b) + abs(v)


def _columns(M, W, S, dtype):
    """c_t = sum_{s<t} M[s, t], s ascending from +0, for t = 0 .. S, with weights"""
    c, wc = np.zeros(S + 1, dtype=dtype), np.zeros(S + 1, dtype=dtype)
    for t in range(1, S + 1):
        c[t], wc[t] = _seq(M[:t, t], W[:t, t], dtype)
    return c, wc


def _vario_tile(Xi, Xj, yi, yj, ai, aj, same, p, S, dtype):
    """one 64 x 64 tile (rows padded with NaN-free zeros and masked): the workgroup's sum in the kernel's order, and its weight"""
    ni, nj = Xi.shape[1], Xj.shape[1]
    m = np.zeros((ni, nj), dtype=dtype)
    wm = np.zeros((ni, nj), dtype=dtype)
    for s in range(S):
        t = _pw(Xi[s][:, None] - Xj[s][None, :], p)
        m = m + t
        wm = wm + (p + 1) * np.abs(t) + np.abs(m)
    ob = _pw(yi[:, None] - yj[None, :], p)
    mean = m / dtype(S)
    r = ob - mean
    wr = (p + 1) * np.abs(ob) + wm / S + np.abs(mean) + np.abs(r)
    aa = ai[:, None] * aj[None, :]
    term = (aa * r) * r
    wt = 2 * aa * np.abs(r) * wr + 3 * np.abs(term)
    mask = np.ones((ni, nj), dtype=bool)
    if same:
        mask = np.arange(ni)[:, None] < np.arange(nj)[None, :]
    T = np.zeros((TILE, TILE), dtype=dtype)
    WT = np.zeros((TILE, TILE), dtype=dtype)
    T[:ni, :nj] = np.where(mask, term, 0)
    WT[:ni, :nj] = np.where(mask, wt, 0)
    # thread (a, b) owns rows 4a + k, columns 4b + l: k outer, l inner
    ws = np.zeros((16, 16), dtype=dtype)
    ww = np.zeros((16, 16), dtype=dtype)
    for k in range(4):
        for l in range(4):
            ws = ws + T[k::4, l::4]
            ww = ww + WT[k::4, l::4] + np.abs(ws)
    v, w = ws.reshape(4, 64), ww.reshape(4, 64)          # tid = 16 a + b: four waves of 64 lanes
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
        w = w + w[:, lane ^ o] + np.abs(v)
    tot, wtot = _seq(v[:, 0], w[:, 0], dtype)
    return tot, wtot


def scores_np(E, y, a, off, fair=False, vario_p=None, dtype=np.float64, want=('total', 'energy')):
    """dict of (value, weight) pairs per output -- 'total' (S, G), 'total_obs', 'crps_total', 'energy', 'dist' (G, S+1, S+1), 'variogram'
    (G, when vario_p is given) -- for the ensemble E (S, N; any row stride), observation y, weights a (None: 1) and boundaries off."""
    E = np.asarray(E)
    S, N = E.shape
    P, G = S + 1, len(off) - 1
    X = np.concatenate([E, np.asarray(y).reshape(1, N)], axis=0).astype(dtype)
    A = np.ones(N, dtype=dtype) if a is None else np.asarray(a).astype(dtype)
    den = S * (S - 1) if fair else S * S
    res = {k: (np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype))
           for k, shape in (('total', (S, G)), ('total_obs', (G,)), ('crps_total', (G,)), ('energy', (G,)), ('dist', (G, P, P)), ('variogram', (G,)))}
    for g in range(G):
        lo, hi = int(off[g]), int(off[g + 1])
        if hi == lo:
            continue
        if 'total' in want:
            T, WT = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
            for c0 in range(lo, hi, CHUNK):
                t, wt = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
                for n in range(c0, min(c0 + CHUNK, hi)):
                    prod = A[n] * X[:, n]
                    t = t + prod
                    wt = wt + np.abs(prod) + np.abs(t)
                T = T + t
                WT = WT + wt + np.abs(T)
            res['total'][0][:, g], res['total'][1][:, g] = T[:S], WT[:S]
            res['total_obs'][0][g], res['total_obs'][1][g] = T[S], WT[S]
            M = np.abs(T[:, None] - T[None, :])
            c, wc = _columns(M, WT[:, None] + WT[None, :] + M, S, dtype)
            res['crps_total'][0][g], res['crps_total'][1][g] = _score_of(c, wc, S, den, dtype)
        if 'energy' in want:
            Q, WQ = np.zeros((P, P), dtype=dtype), np.zeros((P, P), dtype=dtype)
            for c0 in range(lo, hi, CHUNK):
                cls, wcl = [], []
                for q in range(4):
                    acc, w = np.zeros((P, P), dtype=dtype), np.zeros((P, P), dtype=dtype)
                    for n in range(c0 + q, min(c0 + CHUNK, hi), 4):
                        d = X[:, n, None] - X[None, :, n]
                        term = (A[n] * d) * d
                        acc = acc + term
                        w = w + 4 * np.abs(term) + np.abs(acc)
                    cls.append(acc); wcl.append(w)
                ch = cls[0] + cls[1]; wch = wcl[0] + wcl[1] + np.abs(ch)
                ch = ch + cls[2]; wch = wch + wcl[2] + np.abs(ch)
                ch = ch + cls[3]; wch = wch + wcl[3] + np.abs(ch)
                Q = Q + ch
                WQ = WQ + wch + np.abs(Q)
            D = np.sqrt(Q)
            WD = np.where(D > 0, WQ / (2 * np.where(D > 0, D, 1)), 0) + D
            res['dist'][0][g], res['dist'][1][g] = D, WD
            c, wc = _columns(D, WD, S, dtype)
            res['energy'][0][g], res['energy'][1][g] = _score_of(c, wc, S, den, dtype)
        if vario_p is not None:
            n = hi - lo
            nt = (n + TILE - 1) // TILE
            parts, wparts = [], []
            for tj in range(nt):
                for ti in range(tj + 1):
                    i0, i1, j0, j1 = lo + ti * TILE, min(lo + (ti + 1) * TILE, hi), lo + tj * TILE, min(lo + (tj + 1) * TILE, hi)
                    v, w = _vario_tile(X[:S, i0:i1], X[:S, j0:j1], X[S, i0:i1], X[S, j0:j1], A[i0:i1], A[j0:j1], ti == tj, vario_p, S, dtype)
                    parts.append(v); wparts.append(w)
            res['variogram'][0][g], res['variogram'][1][g] = _seq(np.array(parts, dtype=dtype), np.array(wparts, dtype=dtype), dtype)
    return res


def scores_mp(E, y, a, off, fair=False, vario_p=None, dps=50):
    """the definition at 50 digits from the float64 inputs; dict of float arrays rounded once at the end (plus 'dist')"""
    import mpmath as mp
    E = np.asarray(E, dtype=np.float64)
    S, N = E.shape
    P, G = S + 1, len(off) - 1
    out = {k: np.zeros(shape) for k, shape in (('total', (S, G)), ('total_obs', (G,)), ('crps_total', (G,)), ('energy', (G,)), ('dist', (G, P, P)),
                                               ('variogram', (G,)))}
    with mp.workdps(dps):
        X = [[mp.mpf(float(v)) for v in row] for row in E] + [[mp.mpf(float(v)) for v in np.asarray(y).reshape(-1)]]
        A = [mp.mpf(1) if a is None else mp.mpf(float(a[n])) for n in range(N)]
        c = mp.mpf(1) / (S * (S - 1) if fair else S * S)
        pw = (lambda d: mp.sqrt(abs(d))) if vario_p == 0.5 else (lambda d: abs(d)) if vario_p == 1 else (lambda d: d * d)
        for g in range(G):
            rows = range(int(off[g]), int(off[g + 1]))
            T = [mp.fsum(A[n] * X[m][n] for n in rows) for m in range(P)]
            D = [[mp.sqrt(mp.fsum(A[n] * (X[u][n] - X[v][n]) ** 2 for n in rows)) for v in range(P)] for u in range(P)]
            for s in range(S):
                out['total'][s, g] = float(T[s])
            out['total_obs'][g] = float(T[S])
            out['crps_total'][g] = float(mp.fsum(abs(T[s] - T[S]) for s in range(S)) / S
                                         - c * mp.fsum(abs(T[s] - T[t]) for t in range(S) for s in range(t)))
            out['energy'][g] = float(mp.fsum(D[s][S] for s in range(S)) / S - c * mp.fsum(D[s][t] for t in range(S) for s in range(t)))
            out['dist'][g] = np.array([[float(D[u][v]) for v in range(P)] for u in range(P)])
            if vario_p is not None:
                out['variogram'][g] = float(mp.fsum(A[i] * A[j] * (pw(X[S][i] - X[S][j]) - mp.fsum(pw(X[s][i] - X[s][j]) for s in range(S)) / S) ** 2
                                                    for j in rows for i in rows if i < j))
    return out


# ---- fixtures of the bound tier: a posterior-like cloud around y with spreads of 1e-3 .. 1 of |y| (close members included) ----
BOUND_S = (1, 2, 3, 15, 16, 17, 64, 256)
BOUND_G = (1, 3, 70)
VARIO_PS = (0.5, 1.0, 2.0)
MP_MAX_S = 3          # the small fixtures: mpmath is the truth; longdouble for the rest


def group_sizes(S, G):
    if G == 1:
        return [2 * CHUNK + 3]
    if G == 3:
        return [CHUNK - 1, CHUNK, CHUNK + 1]
    cyc = [0, 1, 2, 0, 5, 1, 3, 2, 0, 4] if S == 256 else [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 0, 2 * CHUNK + 3, 7, 0]
    sizes = [cyc[i % len(cyc)] for i in range(70)]
    if S == 256:
        sizes[11], sizes[40] = CHUNK + 1, CHUNK - 1             # 300 rows at most in all (2 CHUNK + 3 is the G = 1 fixture)
    return sizes


@functools.lru_cache(maxsize=None)
def fixture(S, G):
    """dict(E (S, ld) with ld > N -- use E[:, :N] --, N, y, a (None / unequal / with exact zeros), off, fair)"""
    k = BOUND_S.index(S) + BOUND_G.index(G)
    rs = np.random.RandomState(1000 + 10 * S + G)
    sizes = group_sizes(S, G)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    y = np.where(rs.rand(N) < 0.3, 0.0, rs.gamma(2.0, 3.0, N)) + 0.25
    spread = 10.0 ** rs.uniform(-3, 0, S)
    Ebuf = np.full((S, N + 5), np.nan)
    Ebuf[:, :N] = y[None, :] + spread[:, None] * np.abs(y)[None, :] * rs.randn(S, N)
    a = None
    if k % 3 == 1:
        a = 0.5 + 2.0 * rs.rand(N)
    elif k % 3 == 2:
        a = np.where(rs.rand(N) < 0.25, 0.0, 0.1 + rs.rand(N))
    return dict(S=S, G=G, N=N, Ebuf=Ebuf, E=Ebuf[:, :N], y=y, a=a, off=off, fair=bool(k % 2) and S > 1)


@functools.lru_cache(maxsize=None)
def reference(S, G, vario_p=None):
    """(restatement dict of (value, weight), truth dict of values) for a fixture; vario_p None: everything but the variogram"""
    f = fixture(S, G)
    want = ('total', 'energy') if vario_p is None else ()
    ref = scores_np(f['E'], f['y'], f['a'], f['off'], f['fair'], vario_p, want=want)
    if S <= MP_MAX_S and G <= 3:
        truth = scores_mp(f['E'], f['y'], f['a'], f['off'], f['fair'], vario_p)
    else:
        truth = {k: v[0] for k, v in scores_np(f['E'], f['y'], f['a'], f['off'], f['fair'], vario_p, dtype=np.longdouble, want=want).items()}
    return ref, truth


def keys_of(vario_p):
    return ('variogram',) if vario_p is not None else ('total', 'total_obs', 'crps_total', 'energy', 'dist')


def ratio(got, ref_w, truth):
    """max over the elements of |got - truth| / (eps S_w), 0 where the weight and the error are both 0"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(truth, dtype=np.longdouble)).astype(np.float64)
    w = np.asarray(ref_w, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where((err == 0) & (w == 0), 0.0, err / (EPS * w))
    return float(np.max(r)) if r.size else 0.0


def integer_case(seed, S, sizes, weighted):
    """small-integer operands: every product, square and sum of the scores' first stage is exact in float64"""
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    E = rs.randint(-8, 9, size=(S, N)).astype(np.float64)
    y = rs.randint(-8, 9, size=N).astype(np.float64)
    a = rs.randint(0, 4, size=N).astype(np.float64) if weighted else None
    return E, y, a, off


def ensemble_crps_sorted(x, y, fair=False):
    """ensemble CRPS of the scalar sample x against y by the sort-based form: mean |x - y| - c sum_{i<j} |x_i - x_j| with
    sum_{i<j} |x_i - x_j| = sum_i (2 i - S + 1) x_(i)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    S = x.size
    pair = float(np.sum((2 * np.arange(S) - S + 1) * x))
    return float(np.mean(np.abs(x - y))) - pair / (S * (S - 1) if fair else S * S)
