"""The argument the max form of relax_kt's fold rests on, checked on the CPU with numpy and
without reference to any kernel: if every candidate is NaN or has its sign bit clear, then with m = maxNum of the
candidates, `x < m ? m : x` has the bits of the sequential fold `x = x < c ? c : x` for EVERY x -- and a -0.0 among the
candidates breaks it."""
import itertools

import numpy as np
import pytest


def _values(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    fi = np.finfo(dtype)
    if dtype == np.float32:
        nans = np.array([0x7FC01234, 0xFFC00001, 0x7F800001], dtype=u).view(dtype)   # payload, negative, signalling
    else:
        nans = np.array([0x7FF8000000012345, 0xFFF8000000000001, 0x7FF0000000000001], dtype=u).view(dtype)
    den = fi.smallest_subnormal
    xs = np.concatenate([nans, np.array([0.0, -0.0, den, -den, np.inf, -np.inf, 0.5, 1.0, -1.0, 2.0, 3.0], dtype=dtype)])
    cands = np.array([0.0, np.nan, den, den * 1000, 0.5, 1.0, 3.0, np.inf], dtype=dtype)
    return xs, cands, u


def _sequential(x, cs):
    for c in cs:
        x = np.where(x < c, c, x)
    return x


def _max_form(x, cs):
    m = cs[0]
    for c in cs[1:]:
        m = np.fmax(m, c)          # IEEE maxNum: a NaN operand is ignored, NaN if both are
    return np.where(x < m, m, x)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_max_form_equals_the_sequential_fold_for_every_x(dtype):
    xs, cands, u = _values(dtype)
    assert len(xs) == 14 and len(cands) == 8
    total = 0
    with np.errstate(invalid="ignore"):
        for k in (1, 2, 3, 4):
            tuples = np.array(list(itertools.product(range(len(cands)), repeat=k)))      # 8^k x k
            cs = [np.repeat(cands[tuples[:, i]], len(xs)) for i in range(k)]
            x = np.tile(xs, len(tuples))
            a, b = _sequential(x, cs), _max_form(x, cs)
            total += len(x)
            bad = np.flatnonzero(a.view(u) != b.view(u))
            assert bad.size == 0, (k, x[bad[:4]], [c[bad[:4]] for c in cs])
    assert total == 65520


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_negative_zero_candidate_breaks_it(dtype):
    """Why such operands take the compare form: the maximum of (+0, -0) has an ambiguous sign."""
    x = np.array([-1.0], dtype=dtype)
    u = np.uint32 if dtype == np.float32 else np.uint64
    seq = {tuple(_sequential(x, [np.array([a], dtype=dtype), np.array([b], dtype=dtype)]).view(u))
           for a, b in ((0.0, -0.0), (-0.0, 0.0))}
    assert len(seq) == 2          # the sequential fold keeps the FIRST zero: no order-free maximum can follow both
