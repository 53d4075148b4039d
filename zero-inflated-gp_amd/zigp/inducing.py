"""Inducing inputs by k-means (include/zigp.h "inducing inputs"): the start rows, the argument checks of DenseEngine.kmeans* and
`kmeans_np`, the NumPy restatement of the Lloyd iterations that libzigp runs on the device.  The finite procedure is the definition:

  iteration t = 1, 2, ... with the current C (M, D):
    d(i, j)   = sum_k (x_ik - c_jk)^2, k ascending, the difference form
    label_i   = the LOWEST j attaining min_j d(i, j)
    c_j      <- sum of the rows of label j / count_j where count_j > 0; an empty cluster keeps its centroid
    inertia_t = sum_i d(i, label_i) against C before the update; changed_t = rows whose label differs from iteration t - 1, changed_1 = N
  stop after the first t with changed_t = 0, or at t = max_iter.

Seeding beyond a sample of rows, restarts, weights and a tolerance stop are the caller's."""
import numpy as np

KMEANS_MAX_M = 4096   # include/zigp.h ZIGP_KMEANS_MAX_M
MAX_D = 64            # include/zigp.h ZIGP_MAX_D
MAX_ITER = 1 << 20


def sample_rows(N, M, seed):
    """M distinct row indices out of N from np.random.RandomState(seed), in the order drawn"""
    N, M = int(N), int(M)
    if not 1 <= M <= N:
        raise ValueError('sample_rows: need 1 <= M <= N, got M = %d, N = %d' % (M, N))
    return np.random.RandomState(seed).choice(N, M, replace=False).astype(np.int64)


def check_sizes(N, D, M, max_iter):
    """The size refusals of the k-means calls, raised before the library is touched"""
    if not 1 <= D <= MAX_D:
        raise ValueError('kmeans: D must be in [1, %d], got %d' % (MAX_D, D))
    if N < 1 or N >= 2 ** 31:
        raise ValueError('kmeans: N must be in [1, 2^31), got %d' % N)
    if M < 1:
        raise ValueError('kmeans: M must be >= 1, got %d' % M)
    if M > KMEANS_MAX_M:
        raise ValueError('kmeans: M must be <= %d (ZIGP_KMEANS_MAX_M), got %d' % (KMEANS_MAX_M, M))
    if M > N:
        raise ValueError('kmeans: M must be <= N, got M = %d, N = %d' % (M, N))
    if not 1 <= max_iter <= MAX_ITER:
        raise ValueError('kmeans: max_iter must be in [1, %d], got %d' % (MAX_ITER, max_iter))


def check_cols(cols, ld):
    """cols = None (every column) or (col0, D): the D columns from col0 of rows that have ld; returns (col0, D)"""
    if cols is None:
        return 0, int(ld)
    try:
        col0, D = (int(v) for v in cols)
    except (TypeError, ValueError):
        raise ValueError('kmeans: cols must be None or (col0, D)')
    if col0 < 0 or D < 1 or col0 + D > ld:
        raise ValueError('kmeans: cols = (col0, D) needs col0 >= 0, D >= 1 and col0 + D <= %d columns, got (%d, %d)' % (ld, col0, D))
    return col0, D


def check_init(init, M, D):
    """an (M, D) start as a fresh float64 array (the library writes into it)"""
    C0 = np.array(init, dtype=np.float64, order='C')
    if C0.shape != (int(M), int(D)):
        raise ValueError('kmeans: init must be (M, D) = (%d, %d), not %s' % (M, D, C0.shape))
    return C0


def kmeans_np(X, C0, max_iter=100):
    """The definition above on the host.  X (N, D), C0 (M, D); returns (C, info) with info = dict(labels int32 [N], counts int64 [M],
    inertia [n_iter], changed int64 [n_iter], n_iter, n_empty)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64, order='C')
    if X.ndim != 2 or C.ndim != 2 or X.shape[1] != C.shape[1]:
        raise ValueError('kmeans_np: X must be (N, D) and C0 (M, D)')
    N, D = X.shape
    M = C.shape[0]
    check_sizes(N, D, M, int(max_iter))
    labels = None
    inertia, changed = [], []
    counts = np.zeros(M, dtype=np.int64)
    for t in range(int(max_iter)):
        d = np.zeros((N, M))
        for k in range(D):                                  # k ascending
            e = X[:, k:k + 1] - C[None, :, k]
            d += e * e
        new = np.argmin(d, axis=1).astype(np.int32)         # the first minimum: the lowest j
        inertia.append(float(np.sum(d[np.arange(N), new])))
        changed.append(N if labels is None else int(np.count_nonzero(new != labels)))
        labels = new
        counts = np.bincount(labels, minlength=M).astype(np.int64)
        for j in np.nonzero(counts)[0]:
            C[j] = X[labels == j].sum(axis=0) / counts[j]
        if changed[-1] == 0:
            break
    return C, dict(labels=labels, counts=counts, inertia=np.array(inertia), changed=np.array(changed, dtype=np.int64),
                   n_iter=len(changed), n_empty=int(np.count_nonzero(counts == 0)))
