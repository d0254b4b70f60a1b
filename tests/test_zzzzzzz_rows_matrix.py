"""Every instantiation of the register-held rows kernels -- k_std_rows
(center, zscore, normalize's mean baseline), k_detrend_rows, k_norm_rows and
k_q_rows: element type x vector width x {wave, block} per row -- driven
through the backend entry points on raw buffers, on the float64 numpy
executors and, marked gpu, on the HIP kernels.

rows_matrix_cases holds the stated census, the case tables and the checks.
Every launch records the instantiation its own arguments select; the last test
holds the recorded set to the stated one, so it needs the tests before it to
have run on the same executor.  dst lies between guard regions over a byte
pattern: pad columns and guards must keep their bytes, and rows that are not
taken must leave all of dst as it was.

The module is named to be collected after every other one.
"""
import numpy as np
import pytest

import rows_matrix_cases as M
import standardize_cases as S

EXECUTORS = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
_EX = {}


def _executor(name):
    if name not in _EX:
        if name == "gpu":
            import torch
            if not torch.cuda.is_available():
                pytest.skip("no GPU")
        _EX[name] = M.Executor(name)
    return _EX[name]


def _orders(dtype, plan):
    return (1, 3, 5, 8) if plan == "block" and dtype in ("float32", "float64") else (1, 8)


# --------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("ex", EXECUTORS)
@pytest.mark.parametrize("plan", M.PLANS)
@pytest.mark.parametrize("dtype", M.TYPES + ("bool",))
def test_matrix(dtype, plan, ex):
    """One case per vector width of the type: all slots but the last full, the
    last held by five lanes; tail blocks beside the permuted ones."""
    M.fresh(("matrix", dtype, plan))
    ex = _executor(ex)
    for c in M.matrix_cases(dtype, plan):
        res = M.run_case(ex, c, M.data(dtype, c.O, c.R), _orders(dtype, plan))
        assert all(r is not None for r in res.values()), c


# --------------------------------------------------------------- 2. the limits
@pytest.mark.parametrize("ex", EXECUTORS)
@pytest.mark.parametrize("plan", M.PLANS)
@pytest.mark.parametrize("dtype", M.NARROW_TYPES)
def test_limits(dtype, plan, ex):
    """R = 64 x held and 256 x held exactly, once per (item size, vec): every
    slot full.  One vector more than 256 x held: not taken, dst untouched."""
    M.fresh(("limits", dtype, plan))
    ex = _executor(ex)
    for c in M.limit_cases(dtype, plan):
        res = M.run_case(ex, c, M.data(dtype, c.O, c.R))
        assert all((r is None) == (c.kind == "over") for r in res.values()), c


# ------------------------------------------------- 3. why the vector narrowed
@pytest.mark.parametrize("ex", EXECUTORS)
@pytest.mark.parametrize("plan", M.PLANS)
@pytest.mark.parametrize("dtype,vec", [(t, v) for t in M.NARROW_TYPES for v in M.VECS[np.dtype(t).itemsize][:-1]])
def test_narrowed(dtype, vec, plan, ex):
    """A narrower vector forced by the source pitch, the destination pitch, a
    source offset and a destination offset, at an R that allows the widest:
    each within the bounds (run_case), and within them of the aligned call's
    values -- exact operations equal."""
    M.fresh(("narrowed", dtype, vec, plan))
    ex = _executor(ex)
    aligned, ways = M.narrow_cases(dtype, plan)[M.VECS[np.dtype(dtype).itemsize].index(vec)]
    x = M.data(dtype, aligned.O, aligned.R)
    base = M.run_case(ex, aligned, x)
    for way, c in ways:
        assert c.vec == vec, c
        # (the quantile kernel sees the source only)
        res = M.run_case(ex, c, x, quantiles=way.startswith("src"))
        for op, got in res.items():
            assert got is not None and base[op] is not None, (c, op)
            if op in ("center", "zscore", "mean") or op[0] == "detrend":
                bound = M.bound_of(x, op)
                err = np.abs(got.astype(np.longdouble) - base[op].astype(np.longdouble))
                assert np.all(err <= bound), (c, op, float((err / bound).max()))
            else:
                M.exact(got, base[op], "%s %s against the aligned call" % (c, op))
    oes = S.out_dtype(dtype).itemsize
    assert [w for w, _ in ways] == [w for w in M.WAYS if not (w == "dst_ptr" and vec * oes % 16 == 0)]


# ------------------------------------------------------ 4. the truth is numpy's
@pytest.mark.parametrize("dtype", M.TYPES + ("bool",))
def test_truth_is_numpys(dtype):
    """The longdouble truths of center and zscore on the wave cases against
    numpy's own float64 x - x.mean() and its quotient by x.std(), within the
    same bounds: the module's truth is tied to numpy, not only to itself."""
    M.fresh(("matrix", dtype, "wave"))
    for c in M.matrix_cases(dtype, "wave"):
        x = M.data(dtype, c.O, c.R)
        v = x.astype(np.float64)
        cen = v - v.mean(axis=1, keepdims=True)
        for scale, mine in ((0, cen), (1, cen / v.std(axis=1, keepdims=True))):
            t, bound = S.truth_and_bound(x, 1, scale)
            err = np.abs(mine.astype(np.longdouble) - t)
            print("%s (%d, %d) %s: |numpy - truth| / bound = %.3g"
                  % (dtype, c.O, c.R, ("center", "zscore")[scale], float((err / bound).max())))
            assert np.all(err <= bound), (c, scale)


# -------------------------------------------------------------- 5. the census
@pytest.mark.parametrize("ex", EXECUTORS)
def test_census(ex):
    """The instantiations the tests above launched, worked out from each
    launch's own arguments, are the stated ones: no case table silently misses
    a kernel.  Prints each family's worst error / bound ratio."""
    ex = _executor(ex)
    for family in M.FAMILIES:
        seen, want = M.CENSUS[ex.name][family], M.stated(family)
        print("%s %s: %d of %d instantiations in %d launches, worst error / bound = %.3g"
              % (ex.name, family, len(seen & want), len(want), M.RAN[ex.name], M.RATIOS[ex.name][family]))
    for family in M.FAMILIES:
        seen, want = M.CENSUS[ex.name][family], M.stated(family)
        assert seen == want, (family, "not reached", sorted(want - seen, key=str), "not stated",
                              sorted(seen - want, key=str))
    assert len(M.stated("std")) == len(M.stated("detrend")) == len(M.stated("norm")) == 70
    assert len(M.stated("quantile")) == 26
