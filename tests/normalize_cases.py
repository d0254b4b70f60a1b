"""Shared by the normalize() tests: the truth -- for 'percentile' the numpy
restatement, compared bit for bit; for 'mean' a longdouble value and the bound
it is met within --, the plan of bm_normalize_rows worked out from the kernel
code (bolt_amd/csrc/bm_quantile.hip, bm_standardize.hip), and a numpy executor
with bm_normalize_rows next to the standardize and quantile entry points, so
the orchestration the HIP backend takes runs on the CPU.
"""
import numpy as np

import cpu_backend as C
import quantile_cases as Q
import standardize_cases as S
from standardize_cases import axes_of, out_dtype, rand  # noqa: F401  (rand: the records' data)

METHODS = ("percentile", "mean")
NORM_MEAN, NORM_RANK = 0, 1  # BM_NORM_MEAN, BM_NORM_RANK

# bm_normalize_rows takes what bm_standardize_rows takes, for either baseline:
# the vector is the widest of 16 B / item, at most 8 elements, that divides R
# and both pitches; a thread holds min(8 vec, 32) elements; wave per row up to
# 64 x that, block per row up to 256 x that with at least 256 rows
rows_plan = S.rows_plan


def _spread(b, x, axis, kshape):
    """A baseline of the kept axes' shape -> broadcastable against ``x``."""
    b = np.asarray(b).reshape(kshape)
    for a in sorted(set(a % x.ndim for a in axes_of(x, axis))):
        b = np.expand_dims(b, a)
    return b


def percentile_baseline(x, axis, perc):
    """(b, g): the float64 ``perc``-th percentile of every record, 'linear' --
    lo + (hi - lo) g from the sorted rows with pos = (perc / 100)(n - 1), g == 0
    giving lo, three separately rounded operations, a record holding a NaN
    giving NaN -- spread over x's shape, and g."""
    srt, kshape = Q.sorted_rows(x, axis)
    fl, ce, g = Q.position(np.float64(perc) / 100, srt.shape[-1])
    lo = srt[..., fl].astype(np.float64)
    with np.errstate(all="ignore"):
        if g != 0.0:
            d = srt[..., ce].astype(np.float64) - lo
            t = d * g
            b = lo + t
        else:
            b = lo
    if x.dtype.kind == "f":
        b = np.where(np.isnan(srt[..., -1]), np.nan, b)
    return _spread(b, x, axis, kshape), g


def percentile_truth(x, axis, perc, offset):
    """((x as float64 - b) / (b + offset)) rounded once to the result dtype: what every route evaluates."""
    b, _ = percentile_baseline(x, axis, perc)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - b
        den = b + np.float64(offset)
        return (d / den).astype(out_dtype(x.dtype))


def check_percentile(r, b, x, axis, perc=20, offset=0.1, tag=""):
    """``r`` = b.normalize(axis, 'percentile', perc, offset): the array's properties, then bit for bit
    (but for the sign of a zero and a NaN's payload, quantile_cases.same)."""
    tag = "%s percentile %r offset %r" % (tag, perc, offset)
    _check_array(r, b, x, tag)
    got, want = r.toarray(), percentile_truth(x, axis, perc, offset)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape)
    if not Q.same(got, want):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).reshape(-1))
        raise AssertionError("%s: %d of %d differ, first at %d: got %r, want %r"
                             % (tag, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))
    return got


def mean_truth_and_bound(x, axis, offset):
    """(truth t, bound) in longdouble, m the record's mean:
    |got - t| <= 2 eps(out) |t| + 1e-12 max|x_record| (1 + |t|) / |m + offset| + smallest_subnormal(out).
    1e-12 is the project's float64 parity rtol on the mean in the data's units
    (golden_cases.stat_close), carried through dt/dm = -(1 + t) / (m + offset);
    2 eps the allowance for the final rounding (the three float64 roundings
    before it are far below), the subnormal term the output format's floor."""
    ax = axes_of(x, axis)
    v = x.astype(np.longdouble)
    m = v.mean(axis=ax, keepdims=True)
    big = np.abs(v).max(axis=ax, keepdims=True)
    fi = np.finfo(out_dtype(x.dtype))
    with np.errstate(all="ignore"):
        t = (v - m) / (m + np.longdouble(offset))
        floor = 1e-12 * big * (1 + np.abs(t)) / np.abs(m + np.longdouble(offset))
    return t, 2 * np.longdouble(fi.eps) * np.abs(t) + floor + np.longdouble(fi.smallest_subnormal)


def check_mean(r, b, x, axis, offset=0.1, tag=""):
    """``r`` = b.normalize(axis, 'mean', offset=offset) against the longdouble truth;
    prints the worst error / bound ratio before asserting."""
    tag = "%s mean offset %r" % (tag, offset)
    _check_array(r, b, x, tag)
    got = r.toarray()
    t, bound = mean_truth_and_bound(x, axis, offset)
    assert got.dtype == out_dtype(x.dtype) and got.shape == x.shape, (tag, got.dtype, got.shape)
    assert np.isfinite(t).all(), tag  # no record whose mean is -offset or NaN outside the dedicated tests
    err = np.abs(got.astype(np.longdouble) - t)
    ratio = float((err / bound).max()) if err.size else 0.0
    print("%s: max error / bound = %.3g" % (tag, ratio))
    assert np.all(err <= bound), (tag, ratio)
    return got


def check_both(b, x, axis, tag="", perc=20, offset=0.1):
    check_percentile(b.normalize(axis=axis, method="percentile", perc=perc, offset=offset), b, x, axis, perc, offset,
                     tag)
    check_mean(b.normalize(axis=axis, method="mean", offset=offset), b, x, axis, offset, tag)


def _check_array(r, b, x, tag):
    assert type(r) is type(b), tag
    assert r.shape == b.shape == x.shape and r.split == b.split, (tag, r.shape, r.split)
    assert r.dtype == out_dtype(x.dtype), (tag, r.dtype)
    assert r.context is b.context and r._npartitions == b._npartitions, tag


def fused_backend():
    """The standardize and quantile numpy executors in one, plus bm_normalize_rows (include/bolt_mi355x.h)."""

    class NormalizeCpuBackend(type(S.fused_backend()), type(Q.fused_backend())):
        def normalize_rows(self, src, code, O, R, src_pitch, baseline, rank, frac, offset, dst, out_code, dst_pitch):
            dt = np.dtype(C._CODES[code])
            assert src_pitch >= R and dst_pitch >= R and np.dtype(C._CODES[out_code]) == out_dtype(dt)
            assert baseline in (NORM_MEAN, NORM_RANK) and np.isfinite(offset)
            if O == 0 or R == 0:
                return True
            if baseline == NORM_RANK:
                assert 0.0 <= frac < 1.0 and 0 <= rank and rank + (1 if frac != 0.0 else 0) < R
            if rows_plan(dt.itemsize, O, R, src_pitch, dst_pitch) is None:
                return False
            kdt = np.dtype(np.uint8) if dt == np.bool_ else dt
            x = src.numpy().view(kdt)[:O * src_pitch].reshape(O, src_pitch)[:, :R]
            v = x.astype(np.float64)
            with np.errstate(all="ignore"):
                if baseline == NORM_MEAN:
                    b = v.mean(axis=1)
                else:
                    srt = np.sort(Q.keys_of(x), axis=1)
                    b = Q.unkeys(srt[:, rank], kdt).astype(np.float64)
                    if frac != 0.0:
                        d = Q.unkeys(srt[:, rank + 1], kdt).astype(np.float64) - b
                        t = d * frac
                        b = b + t
                    if dt.kind == "f":
                        b = np.where(np.isnan(x).any(axis=1), np.nan, b)
                d = v - b[:, None]
                den = b[:, None] + np.float64(offset)
                self._out(d / den, dst, out_code, O, R, dst_pitch)
            return True

    return NormalizeCpuBackend()
