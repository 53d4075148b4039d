"""CPU: the variance a gradient step takes from the J' panel, var = sigma^2 + colsum(K o (Q W^T) A1), is as accurate as the W-form
var - sum A1^2 + sum s^2 A2^2 of value-only calls: against an 80-bit evaluation, within 10x of the W-form error plus 1e-12 (cfg2 and the
parity tests' shapes; tools/rform_accuracy.py also runs cfg3)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import rform_accuracy as ra  # noqa: E402

CASES = ra.cases(full=False)


@pytest.mark.parametrize('case', CASES, ids=[c[0].replace(' ', '_').replace('/', '-') for c in CASES])
def test_rform_variance_matches_wform_accuracy(case):
    name, Z, ellv, var, s, X = case
    cond, ew, er = ra.variance_errors(Z, ellv, var, s, X)
    print('%s cond %.2e W-form %.2e R-form %.2e' % (name, cond, ew, er))
    assert er <= 10.0 * ew + 1e-12, (name, cond, ew, er)
