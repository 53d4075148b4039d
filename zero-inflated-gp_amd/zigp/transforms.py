"""Parameter transforms of the reference's Param objects (host-side chain rule).

GPflow 0.4.0 `transforms.positive` = `Log1pe` (un-vendored; used at onoffgpf/OnOffSVGP.py:61,63,
onoffgpf/OnOffLikelihood.py:26, scripts/onoff.py:88-123):  y = log(1 + exp(x)) + 1e-6,
x = ys + log(-expm1(-ys)) with ys = max(y - 1e-6, eps).  [GPflow-recall; SURVEY.md a9]
"""
import numpy as np


class Identity:
    def forward(self, x):
        return x

    def backward(self, y):
        return y

    def grad_free(self, x, dy):
        """dL/dx given dL/dy (y = forward(x))."""
        return dy

    def __repr__(self):
        return 'Identity'


class Log1pe:
    def __init__(self, lower=1e-6):
        self._lower = lower

    def forward(self, x):
        x = np.asarray(x, dtype=np.float64)
        return np.logaddexp(0.0, x) + self._lower          # overflow-safe softplus

    def backward(self, y):
        ys = np.maximum(np.asarray(y, dtype=np.float64) - self._lower, np.finfo(np.float64).eps)
        return ys + np.log(-np.expm1(-ys))

    def grad_free(self, x, dy):
        x = np.asarray(x, dtype=np.float64)
        return np.asarray(dy) * (0.5 * (1.0 + np.tanh(0.5 * x)))   # sigmoid(x)

    def __repr__(self):
        return '+ve'


positive = Log1pe()


class LowerTriangular:
    """GPflow 0.4.0 `transforms.LowerTriangular(N)` for one matrix (num_latent = 1; onoffgpf/OnOffSVGP.py:65-71): the free vector holds
    the N(N+1)/2 entries of the lower triangle in row-major order -- the diagonal unconstrained, as in GPflow -- and the value is the
    (N, N) matrix (or (N, N, 1): the trailing axis of length 1 does not change the order) with an exactly zero strict upper triangle.
    The free size differs from the value's size: `free_size` tells ParamSet / AdamGroups.  [GPflow-recall; SURVEY.md a9]"""

    def __init__(self, N):
        self.N = int(N)
        self._rows, self._cols = np.tril_indices(self.N)      # row-major order of the lower triangle

    def free_size(self):
        return self.N * (self.N + 1) // 2

    def forward(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.free_size():
            raise ValueError('LowerTriangular(%d): the free vector has %d entries, not %d' % (self.N, self.free_size(), x.size))
        y = np.zeros((self.N, self.N))
        y[self._rows, self._cols] = x
        return y

    def backward(self, y):
        y = np.asarray(y, dtype=np.float64)
        if y.size != self.N * self.N:
            raise ValueError('LowerTriangular(%d): the value must be (%d, %d)' % (self.N, self.N, self.N))
        return y.reshape(self.N, self.N)[self._rows, self._cols]

    def grad_free(self, x, dy):
        """dL/dx given dL/dy: the lower-triangle entries of dy (whatever dy holds above the diagonal has no free variable)."""
        return np.asarray(dy, dtype=np.float64).reshape(self.N, self.N)[self._rows, self._cols]

    def __repr__(self):
        return 'LowerTriangular(%d)' % self.N
