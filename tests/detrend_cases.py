"""Shared by the detrend() tests: the longdouble truth and the bound it is met
within, an independent polyfit residual to check the truth against, the plan
of bm_detrend_rows worked out from the kernel code (bolt_amd/csrc/
bm_detrend.hip: bm_standardize_rows' plan), and a numpy executor with
bm_detrend_rows / bm_detrend_apply next to the standardize and co-moment entry
points, so the orchestration the HIP backend takes runs on the CPU.
"""
import zlib

import numpy as np

import comoment_cases as CM
import cpu_backend as C
import standardize_cases as S
from standardize_cases import axes_of, out_dtype, rand  # noqa: F401  (rand: the records' data)

MAX_ORDER = 8  # BM_DETREND_MAX_ORDER

# bm_detrend_rows takes what bm_standardize_rows takes (bm_detrend.hip: the
# same pick_vec, lane_vecs and kBlockMinRows): the vector is the widest of
# 16 B / item, at most 8 elements, that divides R and both pitches; a thread
# holds min(8 vec, 32) elements; wave per row up to 64 x that, block per row up
# to 256 x that with at least 256 rows
rows_plan = S.rows_plan


def gram(n, order, dtype, recip=False):
    """p_1..p_order, the discrete orthonormal polynomials on n positions, as an
    (order, n) table of ``dtype``: t_r = r - (n-1)/2,
    b_k = (k/2) sqrt((n-k)(n+k) / (4k^2-1)), p_0 = 1/sqrt(n), p_1 = t p_0 / b_1,
    p_{k+1} = (t p_k - b_k p_{k-1}) / b_{k+1}.  ``recip``: multiply by 1/b_k
    instead of dividing, as the kernel does."""
    ft = np.dtype(dtype).type
    nn = ft(n)
    t = np.arange(n).astype(ft) - (nn - ft(1)) / ft(2)
    k = np.arange(0, order + 2).astype(ft)
    with np.errstate(all="ignore"):
        b = k / ft(2) * np.sqrt((nn - k) * (nn + k) / (ft(4) * k * k - ft(1)))   # b[k], k = 1..order used
    div = (lambda a, c: a * (ft(1) / c)) if recip else (lambda a, c: a / c)
    tab = np.empty((order, n), dtype=ft)
    pm = np.full(n, ft(1) / np.sqrt(nn), dtype=ft)
    pk = div(t * pm, b[1])
    tab[0] = pk
    for q in range(1, order):
        pn = div(t * pk - b[q] * pm, b[q + 1])
        pm, pk = pk, pn
        tab[q] = pk
    return tab


def _records(v, ax):
    """``v`` with the axes ``ax`` (ascending) moved last and flattened in C
    order -> (records (..., n), the inverse to put a result of that shape back)."""
    ax = tuple(sorted(a % v.ndim for a in ax))
    kept = [i for i in range(v.ndim) if i not in ax]
    moved = np.transpose(v, kept + list(ax))
    mshape = moved.shape
    rec = moved.reshape(mshape[:len(kept)] + (-1,))

    def back(y):
        return np.transpose(y.reshape(mshape), np.argsort(kept + list(ax)))
    return rec, back


def residual(v, axis, order, dtype=np.longdouble, recip=False):
    """Every record of ``v`` over ``axis`` minus its least-squares polynomial of
    degree ``order`` (and its mean), in ``dtype``, by the projection onto gram()."""
    rec, back = _records(np.asarray(v).astype(dtype), axes_of(v, axis))
    n = rec.shape[-1]
    with np.errstate(all="ignore"):
        d = rec - rec.mean(axis=-1, keepdims=True)
        if order >= 1:
            P = gram(n, order, dtype, recip)
            fit = np.zeros_like(d)
            for k in range(order):
                c = (d * P[k]).sum(axis=-1, keepdims=True)
                fit = fit + c * P[k]
            d = d - fit
    return back(d)


_TRUTHS = {}


def truth_and_bound(x, axis, order):
    """(truth, bound) in longdouble:
    |got - truth| <= 2 eps(out) |truth| + 1e-12 max|x_record| + smallest_subnormal(out),
    standardize_cases.truth_and_bound's for center.  Computed once per input
    and shared by the executors the tests run on."""
    key = (x.dtype.str, x.shape, str(axis), order, zlib.crc32(np.ascontiguousarray(x).tobytes()))
    hit = _TRUTHS.get(key)
    if hit is None:
        ax = axes_of(x, axis)
        t = residual(x, axis, order)
        with np.errstate(all="ignore"):
            big = np.abs(x.astype(np.longdouble)).max(axis=ax, keepdims=True)
        fi = np.finfo(out_dtype(x.dtype))
        with np.errstate(all="ignore"):
            bound = 2 * np.longdouble(fi.eps) * np.abs(t) + 1e-12 * big + np.longdouble(fi.smallest_subnormal)
        hit = (t, bound)
        if x.size <= 1 << 18:   # (the few larger ones, 32 bytes an element, are worked out again)
            _TRUTHS[key] = hit
    return hit


def polyfit_residual(x, order):
    """The rows of the 2-d ``x`` minus numpy's own least-squares polynomial of
    degree ``order`` over the abscissa scaled to [-1, 1]: independent of gram()."""
    from numpy.polynomial import polynomial as P
    n = x.shape[1]
    ts = np.linspace(-1.0, 1.0, n)
    v = x.astype(np.float64)
    coef = P.polyfit(ts, v.T, order)
    return v - P.polyval(ts, coef).reshape(x.shape)


def check_values(got, x, axis, order, tag="", finite=True):
    """``got`` (ndarray) against the truth; prints the worst error / bound ratio before asserting."""
    t, bound = truth_and_bound(x, axis, order)
    assert got.dtype == out_dtype(x.dtype), (tag, got.dtype)
    assert got.shape == x.shape, (tag, got.shape)
    if finite:
        assert np.isfinite(t).all(), tag
    err = np.abs(got.astype(np.longdouble) - t)
    ok = (err <= bound) | (np.isnan(t) & np.isnan(got))
    with np.errstate(all="ignore"):
        r = np.where(np.isfinite(t), err / bound, 0)
    ratio = float(r.max()) if err.size else 0.0
    print("%s detrend order %d: max error / bound = %.3g" % (tag, order, ratio))
    assert np.all(ok), (tag, order, ratio)
    return got


def check_array(r, b, x, axis, order, tag="", finite=True):
    """The result array ``r`` of ``b.detrend(axis, order)``: type, shape, split, dtype, context, values."""
    assert type(r) is type(b), tag
    assert r.shape == b.shape == x.shape and r.split == b.split, (tag, r.shape, r.split)
    assert r.dtype == out_dtype(x.dtype), (tag, r.dtype)
    assert r.context is b.context and r._npartitions == b._npartitions, tag
    return check_values(r.toarray(), x, axis, order, tag, finite)


def fused_backend():
    """The standardize and co-moment numpy executors in one, plus bm_detrend_rows /
    bm_detrend_apply (include/bolt_mi355x.h) in numpy float64."""

    class DetrendCpuBackend(type(S.fused_backend()), type(CM.fused_backend())):
        def detrend_rows(self, src, code, O, R, src_pitch, order, dst, out_code, dst_pitch):
            dt = np.dtype(C._CODES[code])
            assert src_pitch >= R and dst_pitch >= R and np.dtype(C._CODES[out_code]) == out_dtype(dt)
            assert 1 <= order <= MAX_ORDER and (R == 0 or order < R)
            if O == 0 or R == 0:
                return True
            if rows_plan(dt.itemsize, O, R, src_pitch, dst_pitch) is None:
                return False
            kdt = np.dtype(np.uint8) if dt == np.bool_ else dt
            x = src.numpy().view(kdt)[:O * src_pitch].reshape(O, src_pitch)[:, :R]
            self._out(residual(x, 1, order, np.float64, recip=True), dst, out_code, O, R, dst_pitch)
            return True

        def detrend_apply(self, src, code, O, R, I, src_pitch, mean, coef, basis, order, dst, out_code, dst_pitch):
            dt = np.dtype(C._CODES[code])
            assert src_pitch >= R and dst_pitch >= R and (I == 1 or src_pitch == dst_pitch == R)
            assert np.dtype(C._CODES[out_code]) == out_dtype(dt)
            assert 1 <= order <= MAX_ORDER   # (R may be a rank's slab of a longer record: order >= R is fine)
            if O == 0 or R == 0 or I == 0:
                return
            a = src.numpy().view(np.uint8 if dt == np.bool_ else dt)
            if I == 1:
                x = a[:O * src_pitch].reshape(O, src_pitch)[:, :R].reshape(O, R, 1)
            else:
                x = a[:O * R * I].reshape(O, R, I)
            m = mean.numpy().view(np.float64)[:O * I].reshape(O, 1, I)
            c = coef.numpy().view(np.float64)[:order * O * I].reshape(order, O, 1, I)
            p = basis.numpy().view(np.float64)[:order * R].reshape(order, 1, R, 1)
            with np.errstate(all="ignore"):
                y = x.astype(np.float64) - m
                fit = c[0] * p[0]
                for k in range(1, order):
                    fit = fit + c[k] * p[k]
                y = y - fit
            self._out(y.reshape(O, R * I), dst, out_code, O, R * I, dst_pitch if I == 1 else None)

    return DetrendCpuBackend()
