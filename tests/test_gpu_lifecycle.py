"""Create / destroy cycles of a DenseEngine: zigp_destroy hands back every device allocation of the context -- the dense and
Kronecker buffers, the tile-list cache, the status word -- including what a call that failed with ZIGP_ENOTPD left behind."""
import numpy as np
import pytest

from conftest import make_problem
from test_gpu_kron import make_kron_problem

pytestmark = pytest.mark.gpu

# Free device memory after a destroy may differ from the first post-warm-up reading by at most this much.  Measured on one MI355X:
# 0 bytes after each of the four cycles.  The bound leaves a little room for the runtime's own bookkeeping and stays below every
# matrix and panel a cycle allocates (an M x M matrix at Mp = 256 is 512 KiB; a cycle allocates tens of MB in all).
FREE_TOL = 256 << 10


def _cycle():
    import zigp
    e = zigp.DenseEngine(0)
    try:
        X, Y, p = make_problem(3000, 200, 3, seed=3, Mg=136)
        e.set_chunk(1024)      # three chunks: the chunk loop's side-stream sections run
        e.set_data(X, Y)
        ed, kl, g = e.elbo(p)
        assert np.isfinite(ed) and np.isfinite(kl)
        assert np.all(np.isfinite(e.predict(p, X[:700])))
        Xk, Yk, pk = make_kron_problem(400, 6, 5, seed=14, M0g=7, M1g=4)
        a = e.kron_elbo(pk, Xk, Yk, jitter=1e-5, scale=3.0)                       # fused Kronecker path
        e.set_kron_panels(True)
        b = e.kron_elbo(pk, Xk, Yk, jitter=1e-5, scale=3.0)                       # panel (GEMM-core) path
        assert np.isfinite(a[0]) and np.isfinite(b[0])
        Xb, Yb, pb = make_problem(500, 32, 3, seed=1)                             # the input of test_gpu_dense.py::test_not_pd_raises
        pb['Zf'][5, 0] = np.nan
        e.set_data(Xb, Yb)
        with pytest.raises(zigp.NotPositiveDefiniteError):
            e.elbo(pb, jitter=0.0)
    finally:
        e.close()


def test_create_destroy_returns_device_memory():
    import torch
    torch.cuda.init()
    _cycle()                   # warm: code objects loaded, the runtime's pools set up
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    deltas = []
    for _ in range(4):
        _cycle()
        torch.cuda.synchronize()
        deltas.append(free0 - torch.cuda.mem_get_info()[0])
    print('free device memory after each destroy, relative to the first (bytes lost):', deltas)
    assert all(abs(d) <= FREE_TOL for d in deltas), deltas
