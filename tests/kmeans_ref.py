"""A second, independent evaluation of the Lloyd iterations of include/zigp.h ("inducing inputs") for the tests: distances and cluster
means in np.longdouble, sums by math.fsum, plain loops over the clusters -- nothing shared with zigp.inducing.kmeans_np or the library.
Also the seeded blob fixtures of the k-means tests and the error figures the project's rule err_gpu <= 4 err_np + 16 eps S needs."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps

# (seed, K blobs, rows per blob, D, extra uniform rows): N = 493, 533, 301, 607; M = K
FIXTURES = ((7, 12, 40, 3, 13), (8, 33, 16, 2, 5), (9, 5, 60, 8, 1), (10, 20, 30, 9, 7))
MIN_GAP = 1e-6     # the fixtures' precondition: no row ever sits closer than this (relatively) to a tie between its two nearest centroids


def blobs(seed, K, per, D, extra):
    """(X (N, D), C0 (K, D)): K centres uniform in [0, 10]^D, `per` rows = centre + 0.3 randn around each, `extra` uniform rows, shuffled;
    the start is K distinct rows drawn next from the same generator"""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(0.0, 10.0, (K, D))
    X = np.vstack([np.repeat(centres, per, axis=0) + 0.3 * rng.randn(K * per, D), rng.uniform(0.0, 10.0, (extra, D))])
    X = np.ascontiguousarray(X[rng.permutation(X.shape[0])])
    idx = rng.choice(X.shape[0], K, replace=False)
    return X, np.ascontiguousarray(X[idx])


def distances(X, C):
    """d(i, j) = sum_k (x_ik - c_jk)^2 in long double, (N, M)"""
    Xl, Cl = np.asarray(X, dtype=np.longdouble), np.asarray(C, dtype=np.longdouble)
    d = np.zeros((Xl.shape[0], Cl.shape[0]), dtype=np.longdouble)
    for k in range(Xl.shape[1]):
        e = Xl[:, k:k + 1] - Cl[None, :, k]
        d = d + e * e
    return d


def means_of(X, labels, C, S_prev=None):
    """The update for given labels: (new C float64, counts, S) -- long-double sums by fsum over each cluster's rows; an empty cluster keeps
    its row of C.  S (M, D) = sum |x| / count, the scale of the accuracy rule; an empty cluster keeps its row of S_prev (0 without one):
    the scale of the update that made its centroid."""
    M, D = C.shape
    out, S = np.array(C, dtype=np.float64), np.zeros((M, D)) if S_prev is None else np.array(S_prev, dtype=np.float64)
    counts = np.zeros(M, dtype=np.int64)
    for j in range(M):
        rows = np.nonzero(labels == j)[0]
        counts[j] = rows.size
        if rows.size == 0:
            continue
        for k in range(D):
            col = X[rows, k]
            out[j, k] = float(np.longdouble(math.fsum(col)) / np.longdouble(rows.size))
            S[j, k] = math.fsum(np.abs(col)) / rows.size
    return out, counts, S


def means_np_error(X, labels, C):
    """|float64 NumPy means - the long-double means| per entry: err_np of the rule (0 for an empty cluster)"""
    ref, counts, _ = means_of(X, labels, C)
    err = np.zeros_like(ref)
    for j in np.nonzero(counts)[0]:
        err[j] = np.abs(X[labels == j].sum(axis=0) / counts[j] - ref[j])
    return err


def lloyd(X, C0, max_iter):
    """The whole run: dict(C, labels, counts, inertia [n_iter], changed [n_iter], n_iter, min_gap, S).  The centroids are carried in float64
    between iterations (each update rounded once from its long-double value); min_gap is the smallest (d2 - d1) / d2 over all rows and
    iterations, d1 <= d2 a row's two smallest distances (inf for M = 1)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    N, M = X.shape[0], C.shape[0]
    labels, inertia, changed, min_gap = None, [], [], np.inf
    counts, S, n_made = np.zeros(M, dtype=np.int64), np.zeros(C.shape), np.zeros(M, dtype=np.int64)
    for _ in range(max_iter):
        d = distances(X, C)
        new = np.zeros(N, dtype=np.int32)
        best = np.zeros(N, dtype=np.longdouble)
        for i in range(N):
            j = 0
            for q in range(1, M):
                if d[i, q] < d[i, j]:
                    j = q
            new[i], best[i] = j, d[i, j]
        if M > 1:
            two = np.sort(d, axis=1)[:, :2]
            ok = two[:, 1] > 0
            min_gap = min(min_gap, float(np.min((two[ok, 1] - two[ok, 0]) / two[ok, 1])) if ok.any() else 0.0)
            if not ok.all():
                min_gap = 0.0
        inertia.append(math.fsum(float(v) for v in best))
        changed.append(N if labels is None else int(np.count_nonzero(new != labels)))
        labels = new
        C, counts, S = means_of(X, labels, C, S)
        n_made = np.where(counts > 0, counts, n_made)
        if changed[-1] == 0:
            break
    return dict(C=C, labels=labels, counts=counts, inertia=np.array(inertia), changed=np.array(changed, dtype=np.int64), n_iter=len(changed),
                min_gap=min_gap, S=S, n_made=n_made)


_RUNS = {}


def fixture_run(i):
    """(X, C0, the reference run with max_iter = 100) of FIXTURES[i], computed once per process and shared; callers do not write to it"""
    if i not in _RUNS:
        X, C0 = blobs(*FIXTURES[i])
        _RUNS[i] = (X, C0, lloyd(X, C0, 100))
    return _RUNS[i]
