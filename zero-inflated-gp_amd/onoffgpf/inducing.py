"""Inducing inputs for OnOffSVGP by k-means on the device.  The reference notebook hands the model inducing inputs picked on the host
(scipy.cluster.vq.kmeans, as scripts/onoff.py:67 does for the Kronecker model); this is the same step at the sizes the dense path runs:
Lloyd iterations from M sampled rows, on the GPU (zigp.DenseEngine.kmeans)."""
import numpy as np

import zigp


def kmeans_inducing(X, M, seed=None, device=0, engine=None, max_iter=100):
    """Z (M, D) for `Zf` / `Zg` of OnOffSVGP: the centroids of Lloyd's iterations on X (N, D), started from the M rows
    zigp.inducing.sample_rows(N, M, seed).  engine: a DenseEngine to run on (its resident data is not touched); None: one is created
    on `device` for the call.  An empty cluster keeps its start row, so Z always has M rows."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.ndim != 2:
        raise ValueError('X must be (N, D)')
    own = engine is None
    eng = zigp.DenseEngine(device) if own else engine
    try:
        return eng.kmeans(X, M, seed=seed, max_iter=max_iter)
    finally:
        if own:
            eng.close()
