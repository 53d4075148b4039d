"""Host side of the sample-path scores (include/zigp_ensemble.h): how `groups` becomes the boundaries the
library takes, and every refusal that comes before the library is touched.  Pure NumPy: nothing here needs a GPU."""
import numpy as np

from . import _lib

MAX_S = 256                      # ZIGP_PATH_MAX_S
VARIO_P = (0.5, 1.0, 2.0)
MEMBERS = ('f', 'g', 'gf')


def plan_groups(groups, N):
    """(off, order, labels) for N rows.  groups None: one group.  Boundaries (G + 1 non-decreasing integers from 0 to N): as they are.
    Integer labels (N entries): groups in ascending label order, `labels` the distinct labels in that order; when the labels are not
    non-decreasing, `order` is the stable sort that makes them so (apply it to the columns), else None.  N entries that also read as
    boundaries (G + 1 = N, from 0 to N, non-decreasing) are boundaries."""
    N = int(N)
    if groups is None:
        return np.array([0, N], dtype=np.int64), None, None
    g = np.asarray(groups)
    if g.ndim != 1 or g.size < 1 or not (np.issubdtype(g.dtype, np.integer) or (np.issubdtype(g.dtype, np.floating) and np.all(g == np.round(g)))):
        raise ValueError('groups must be None, G + 1 integer boundaries from 0 to N, or N integer labels')
    g = g.astype(np.int64)
    as_bounds = g.size >= 2 and g[0] == 0 and g[-1] == N and np.all(np.diff(g) >= 0)
    if g.size != N or as_bounds:
        if not as_bounds:
            raise ValueError('groups: %d entries are neither N = %d labels nor boundaries that start at 0, end at N and never decrease' % (g.size, N))
        return np.ascontiguousarray(g), None, None
    labels, inv, counts = np.unique(g, return_inverse=True, return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    order = None if np.all(np.diff(g) >= 0) else np.argsort(inv, kind='stable')
    return off, order, labels


def check_args(S, N, off, weights, variogram, fair):
    """The refusals of an ensemble_scores call that need no device; returns the zigp_ens_opts record"""
    if not 1 <= int(S) <= MAX_S:
        raise ValueError('E must have 1 <= S <= %d members (ZIGP_PATH_MAX_S), not %d' % (MAX_S, S))
    if not 1 <= int(N) < 2 ** 31:
        raise ValueError('E must have 1 <= N < 2^31 rows, not %d' % N)
    if fair and int(S) == 1:
        raise ValueError('fair=True needs at least two members (c = 1 / (S (S - 1)))')
    if variogram is not None and float(variogram) not in VARIO_P:
        raise ValueError('variogram must be None or the order p in (0.5, 1, 2), not %r' % (variogram,))
    if variogram is not None and np.max(np.diff(off)) > _lib.ENS_VARIO_MAX_ROWS:
        raise ValueError('variogram: groups has a group of %d rows, more than %d (ZIGP_ENS_VARIO_MAX_ROWS)'
                         % (int(np.max(np.diff(off))), _lib.ENS_VARIO_MAX_ROWS))
    if isinstance(weights, np.ndarray) and not (np.all(np.isfinite(weights)) and np.all(weights >= 0)):
        raise ValueError('weights must be finite and >= 0')
    o = _lib.zigp_ens_opts()
    o.fair, o.vario_p = 1 if fair else 0, 0.0 if variogram is None else float(variogram)
    return o


def member_plane(member):
    if member not in MEMBERS:
        raise ValueError("member must be 'f', 'g' or 'gf', not %r" % (member,))
    return member
