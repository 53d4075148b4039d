"""Quadrature rules for the standard normal, as the density calls take them (include/zigp.h "predictive density")."""
import numpy as np


def gauss_hermite(n):
    """(nodes, weights) of the n-point Gauss-Hermite rule normalised for N(0, 1): sum_i w_i h(x_i) ~ E[h(x)], sum w_i = 1.
    numpy.polynomial.hermite_e.hermegauss with the weights divided by sqrt(2 pi).  Beyond some 180 nodes the outermost weights are
    denormal or underflow to zero in float64; a zero weight carries nothing, so those nodes are dropped (the density calls refuse a
    weight that is not positive) and the rule returned may be a few nodes shorter than n."""
    n = int(n)
    if n < 1:
        raise ValueError('gauss_hermite: n must be at least 1')
    x, w = np.polynomial.hermite_e.hermegauss(n)
    w = w / np.sqrt(2.0 * np.pi)
    keep = w > 0
    return np.ascontiguousarray(x[keep]), np.ascontiguousarray(w[keep])
