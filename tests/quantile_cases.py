"""Shared by the quantile() / percentile() / median() tests: the truth (numpy's
own order statistics for 'lower' / 'higher', the restated formula for
'linear'), the data, and a numpy executor with bm_quantile_rows /
bm_quantile_select, so the orchestration the HIP backend takes (pitches,
permuted layouts, batches of ranks, rank slabs) runs on the CPU.
"""
import numpy as np

import cpu_backend as C
from standardize_cases import axes_of, out_dtype, rand, rows_plan  # noqa: F401  (rand: the records' data)

METHODS = ("linear", "lower", "higher")
MAX_RANKS = 8        # BM_QUANTILE_MAX_RANKS: a 'linear' quantile with g != 0 takes two
QG = 1.0 / np.pi     # a q with g != 0 for every n > 1 used here (asserted by rows_of's callers)
QS = (0.0, 1.0, 0.5, 0.1, QG)


def rows_of(x, axis):
    """``x`` with the kept axes first (ascending) and the reduced ones
    flattened into the last -> (rows array, kept shape)."""
    ax = sorted(set(a % x.ndim for a in axes_of(x, axis)))
    kept = [i for i in range(x.ndim) if i not in ax]
    kshape = tuple(x.shape[i] for i in kept)
    return np.transpose(x, kept + ax).reshape(kshape + (-1,)), kshape


def position(q, n):
    """pos = q (n - 1) in float64 -> (floor, ceil, g)."""
    pos = np.float64(q) * (n - 1)
    fl = np.floor(pos)
    return int(fl), int(np.ceil(pos)), float(pos - fl)


_SORTED = {}


def sorted_rows(x, axis):
    """np.sort of rows_of (NaNs last), computed once per array and axis and never written to."""
    key = (id(x), str(axis))
    hit = _SORTED.get(key)
    if hit is None or hit[0] is not x:
        rows, kshape = rows_of(x, axis)
        srt = np.sort(rows.view(np.uint8) if x.dtype == np.bool_ else rows, axis=-1)
        srt.setflags(write=False)
        if len(_SORTED) > 8:
            _SORTED.clear()
        hit = _SORTED[key] = (x, srt, kshape)
    return hit[1], hit[2]


def truth(x, q, axis, method):
    """The expected result for one scalar ``q``.  'lower' / 'higher':
    np.quantile(x, q, axis, method=...) itself (bool through its uint8 bytes:
    numpy has no bool quantile; float16 widened to float32 and the selected
    element narrowed again, both exact: numpy forms q (n - 1) in the array's
    dtype, which for float16 rows of 2048 values or more is not an index any
    more -- q = 1 of 9000 values asks for element 9000).  'linear': the restatement -- lo / hi picked
    from the sorted rows, lo + (hi - lo) * g in float64 with g == 0 giving lo,
    rounded once to the statistics dtype; a row holding a NaN gives NaN."""
    ax = tuple(sorted(set(a % x.ndim for a in axes_of(x, axis))))
    if method != "linear":
        if x.dtype == np.bool_:
            return np.asarray(np.quantile(x.view(np.uint8), q, axis=ax, method=method)).astype(np.bool_)
        with np.errstate(all="ignore"):
            if x.dtype == np.float16:
                return np.asarray(np.quantile(x.astype(np.float32), q, axis=ax, method=method)).astype(np.float16)
            return np.asarray(np.quantile(x, q, axis=ax, method=method))
    srt, kshape = sorted_rows(x, axis)
    fl, ce, g = position(q, srt.shape[-1])
    lo = srt[..., fl].astype(np.float64)
    with np.errstate(all="ignore"):
        if g != 0.0:
            hi = srt[..., ce].astype(np.float64)
            d = hi - lo
            t = d * g
            val = lo + t
        else:
            val = lo
        if x.dtype.kind == "f":
            val = np.where(np.isnan(srt[..., -1]), np.nan, val)
        return np.asarray(val).astype(out_dtype(x.dtype)).reshape(kshape)


def numpy_f64_bound(x, q, axis):
    """(np.quantile(x as float64, q), 4 * spacing(max(|lo|, |hi|))): numpy's
    own 'linear' result and the bound either formula stays inside (both round
    at most three operations on magnitudes of at most twice that maximum)."""
    ax = tuple(sorted(set(a % x.ndim for a in axes_of(x, axis))))
    srt, kshape = sorted_rows(x, axis)
    fl, ce, g = position(q, srt.shape[-1])
    big = np.maximum(np.abs(srt[..., fl].astype(np.float64)), np.abs(srt[..., ce].astype(np.float64)))
    with np.errstate(all="ignore"):
        ref = np.asarray(np.quantile(x.astype(np.float64), q, axis=ax))
        return ref.reshape(kshape), (4 * np.spacing(big)).reshape(kshape)


def same(got, want):
    """Bit for bit but for the sign of a zero (numpy's sort leaves the order of
    -0.0 and +0.0 open) and a NaN's payload."""
    return np.array_equal(got, want, equal_nan=True) if want.dtype.kind == "f" else np.array_equal(got, want)


def check(b, x, q, axis, method, tag=""):
    """b.quantile(q) for one scalar q against the truth -> the result as an ndarray."""
    want = truth(x, q, axis, method)
    got = np.asarray(b.quantile(q, axis=axis, method=method))
    if got.ndim == 0 and want.size == 1:
        got = got.reshape(want.shape)  # toscalar() of a one-element result, as the statistics give it
    tag = "%s q=%r %s" % (tag, q, method)
    assert got.dtype == want.dtype, (tag, got.dtype, want.dtype)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not same(got, want):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).reshape(-1))
        raise AssertionError("%s: %d of %d differ, first at %d: got %r, want %r"
                             % (tag, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))
    if method == "linear" and got.dtype == np.float64:
        ref, bound = numpy_f64_bound(x, q, axis)
        ok = np.isfinite(bound) & np.isfinite(ref)
        err = np.abs(got - ref)[ok]
        print("%s: max |got - np.quantile| / bound = %.3g" % (tag, float((err / bound[ok]).max()) if err.size else 0.0))
        assert np.all(err <= bound[ok]), tag
    return got


def check_all(b, x, axis, tag="", qs=QS):
    n = rows_of(x, axis)[0].shape[-1]
    assert n <= 1 or position(QG, n)[2] != 0.0
    for method in METHODS:
        for q in qs:
            check(b, x, q, axis, method, tag)


# ---- order-preserving keys, as bm_quantile.hip forms them ----
def keys_of(x):
    """x's elements as unsigned keys of their width whose integer order is the
    elements' order (floats: IEEE, -0.0 before +0.0; NaNs at the ends)."""
    dt = x.dtype
    u = np.ascontiguousarray(x).view("u%d" % dt.itemsize)
    sign = u.dtype.type(1 << (8 * dt.itemsize - 1))
    if dt.kind == "f":
        return np.where(u & sign, ~u, u | sign)
    if dt.kind == "i":
        return u ^ sign
    return u


def unkeys(k, dt):
    sign = k.dtype.type(1 << (8 * dt.itemsize - 1))
    if dt.kind == "f":
        u = np.where(k & sign, k ^ sign, ~k)
    elif dt.kind == "i":
        u = k ^ sign
    else:
        u = k
    return np.ascontiguousarray(u).view(dt)


def fused_backend():
    """CpuBackend plus bm_quantile_rows / bm_quantile_select (include/bolt_mi355x.h) in numpy."""

    class QuantileCpuBackend(C.CpuBackend):
        calls = None  # {"rows": taken calls, "select": calls}, set by a test that counts

        def _quantiles(self, src, code, O, R, pitch, ranks, frac, out, out_code):
            dt = np.dtype(C._CODES[code])
            odt = np.dtype(C._CODES[out_code])
            assert pitch >= R and 1 <= len(ranks) == len(frac) <= MAX_RANKS
            assert len(ranks) + sum(1 for g in frac if g != 0.0) <= MAX_RANKS
            assert all(0.0 <= g < 1.0 for g in frac)
            assert odt == dt or (odt == out_dtype(dt))
            assert odt == out_dtype(dt) or all(g == 0.0 for g in frac)
            if O == 0 or R == 0:
                return
            assert all(0 <= r and r + (1 if g != 0.0 else 0) < R for r, g in zip(ranks, frac))
            kdt = np.dtype(np.uint8) if dt == np.bool_ else dt
            x = src.numpy().view(kdt)[:O * pitch].reshape(O, pitch)[:, :R]
            srt = np.sort(keys_of(x), axis=1)
            nan = np.isnan(x).any(axis=1) if dt.kind == "f" else np.zeros(O, dtype=bool)
            res = out.numpy().view(odt)[:len(ranks) * O].reshape(len(ranks), O)
            for k, (r, g) in enumerate(zip(ranks, frac)):
                lo = unkeys(srt[:, r], kdt)
                if odt == dt and g == 0.0:
                    val = lo.view(dt)
                else:
                    val = lo.astype(np.float64)
                    if g != 0.0:
                        with np.errstate(all="ignore"):
                            d = unkeys(srt[:, r + 1], kdt).astype(np.float64) - val
                            t = d * g
                            val = val + t
                if dt.kind == "f":
                    val = np.where(nan, np.nan, val)
                res[k] = val.astype(odt)

        def quantile_rows(self, src, code, O, R, pitch, ranks, frac, out, out_code):
            es = np.dtype(C._CODES[code]).itemsize
            if O and R and rows_plan(es, O, R, pitch, pitch) is None:
                return False
            self._quantiles(src, code, O, R, pitch, ranks, frac, out, out_code)
            if self.calls is not None:
                self.calls["rows"] += 1
            return True

        def quantile_select(self, src, code, O, R, pitch, ranks, frac, out, out_code, workspace=None):
            self._quantiles(src, code, O, R, pitch, ranks, frac, out, out_code)
            if self.calls is not None:
                self.calls["select"] += 1

    return QuantileCpuBackend()
